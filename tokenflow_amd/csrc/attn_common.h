// Extended attention: what the streaming kernels share -- the parameter blocks, the LDS tile geometry, the device helpers
// and the launch helpers.  Included by ext_attn.hip (through the kernel headers) only.
#pragma once

#include <stdlib.h>

#include <type_traits>

#include "attn_fused.h"
#include "tf_common.h"

// Binades by which a query's softmax reference point may trail its running maximum (kernels without the score bound)
#ifndef TF_ATTN_LAG
#define TF_ATTN_LAG 8.0f
#endif

namespace {

template <int DH, int KT = 64>   // KT = keys per staged tile (one barrier interval): 64 everywhere; a parameter for ext_attn_kernel only
struct AttnCfg {
    static constexpr int KS = (DH + 15) / 16;   // QK^T k-steps over the head dim
    static constexpr int DKP = KS * 16;         // head dim padded for QK^T (zero columns)
    static constexpr int KROW = DKP + 8;        // K row stride in LDS (elements)
    static constexpr int MT = (DH + 31) / 32;   // PV M-tiles over the head dim
    static constexpr int VROWS = MT * 32;       // V^T rows in LDS (rows >= DH stay constant)
    static constexpr int VROW = KT + 8;         // V^T row stride in LDS (elements)
    static constexpr int PPR = DH / 8;          // 16-B pieces per K row
    static constexpr int VPR = KT / 8;          // 16-B pieces per V^T row
    static constexpr int SUB = KT / 64;         // 64-key sub-tiles per staged tile
    static constexpr int K_ELEMS = KT * KROW;
    static constexpr int V_ELEMS = VROWS * VROW;
    static constexpr int npk(int nt) { return (KT * PPR + nt - 1) / nt; }   // K pieces per thread
    static constexpr int npv(int nt) { return (DH * VPR + nt - 1) / nt; }   // V^T pieces per thread
    static constexpr size_t lds_bytes(int nb) { return 2 * (size_t)(K_ELEMS + nb * V_ELEMS) * 2; }
};

enum { MODE_ALL = 0, MODE_SOURCE = 1, MODE_DUAL = 2, MODE_MV4 = 3 };
static inline const char* mode_name(int mode) {
    return mode == MODE_ALL ? "ALL" : mode == MODE_DUAL ? "DUAL" : mode == MODE_MV4 ? "MV4" : "SOURCE";
}

// Head dims whose streaming kernels use the Cauchy-Schwarz score bound |q.k| <= |q| max|k| (per-block key norms from the
// pre-pass) to skip the per-tile maximum: Dh = 40 since round 2, Dh = 64 since round 6 (Dh = 80 measured no gain,
// profiles/r06_attn_d80_bound_ab.txt).
constexpr bool attn_has_bound(int dh) { return dh == 40 || dh == 64; }

struct AttnParams {
    const void* q;
    const void* k;
    const void* vt;
    const float* knorm2;  // [3][H][K*Spad/64] max |k|^2 per 64-key block, Dh = 40 kernels only (from vt_pack_kernel)
    void* out;
    int K, Kq, q_frame0, S, H, Spad, nQT, inject, fold;   // fold: TF_ATTN_FOLD_SCALE (Dh = 40 only)
    int part;  // 0 = all three branches, TF_ATTN_BANK_ONLY, TF_ATTN_SOURCE_ONLY
    int out_f32;       // TF_ATTN_OUT_F32: `out` is float (the normalised fp32 accumulator, no 16-bit rounding)
    int nseg;          // > 1: every bank problem is split into nseg runs of bank frames (small grids, see split_plan)
    int bit_stable;    // TF_ATTN_NO_SPLIT: kernel choice and arithmetic are functions of the shape alone
    int Kb;            // frames of the V^T image and of the key norm table (their row strides).  = K in a one-call launch; a run
                       // launch (tf_ext_attn_run) has K = the run's frames, Kb = the whole bank, and k / vt / knorm2 pointing at
                       // the run's first frame
    int pslots;        // partial-result slots per (bank, query frame, head, query) row: nseg in the split form, 0 when the launch
                       // writes the final output; a run launch: the slots of ALL runs (partials points at this run's first slot)
    int run;           // host only: a run launch (partials always, no merge, the ping-pong kernel's partial form)
    int* run_hdr;      // host only: where the pre-pass leaves the number of slots this run filled (read by the runs merge)
    int mix;           // TF_ATTN_HINT_MIX: the mixed-MFMA-shape form (Dh = 40) whatever the launch size, where the frames
                       // admit the interleaved kernel (S % 64 == 0, S >= 256); no effect on ragged frames
    float* partials;   // [2 banks][Kq][H][S][pslots][Dh + 8] fp32: unnormalised O, l, log2-domain shift  // K bank frames; queries = frames q_frame0 .. +Kq
    int64_t ld;      // token stride of k and v
    int64_t ld_q;    // token stride of q (its own: a rank's q may be a column slab of the fused projection while the
                     // bank arrives from a collective as dense slabs)
    // branch / frame strides in elements (dense tensors: frame = S*ld, branch = frames*S*ld; out: S*H*Dh, Kq*S*H*Dh).
    // A caller whose q / k / v arrive from a collective reads them in the layout the collective delivers and has
    // the output written in the layout the next collective sends (tf_ext_attn_fwd_strided, sharded.py).
    int64_t q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, o_fs;
    float c;  // scale * log2(e)
    // host only, multi-edit batches (tf_ext_attn_fwd_edits): the composing call has packed V^T for all branches already /
    // the bank launch is the four-bank shared-softmax form (MODE_MV4) / the DUAL form at any S (the odd edit beside it)
    int no_pack, mv4, force_dual;
    // MODE_MV4: branches between the uncond branches of the launch's two edits (2 = adjacent edits); its banks 2 and 3 are the
    // branches b + gap and b + gap + 1 of the V^T image and of the output (the masked multi-edit call pairs injecting edits
    // that need not be neighbours)
    int gap;
};

// Sliding-window keyframe bank (tf_ext_attn_fwd_windows): the launch's parameter block with the window table behind it.  A type
// of its own, so that every other launch keeps its parameter block and its code; the table rides in the kernel arguments (a
// workgroup reads its query frame's entry with one scalar load), there is no device table, no copy and no sync.
struct AttnParamsWin : AttnParams {
    unsigned win[TF_MAX_WINDOW_FRAMES];   // query frame i: first bank frame of its window | frames of the window << 16
};
template <typename P>
constexpr bool is_win = std::is_same<P, AttnParamsWin>::value;

// Windowed launches, key range of a bank problem: run `seg` of the nseg runs of query frame f's WINDOW.  A window shorter than
// nseg frames leaves some runs empty (n_fr = 0).
__device__ __forceinline__ void window_range(const AttnParamsWin& p, int f, int seg, int nseg, int& f_lo, int& n_fr) {
    const unsigned w = p.win[f];
    const int lo = (int)(w & 0xffffu), n = (int)(w >> 16);
    f_lo = lo + (seg * n) / nseg;
    n_fr = lo + ((seg + 1) * n) / nseg - f_lo;
}

// Windowed split form, an empty run: the neutral partial result (O = 0, l = 0, shift = -inf: weight 0 in attn_merge_kernel)
// for the `rows` queries from q0 on, in each of the nb banks from `bank` on.
__device__ __forceinline__ void write_empty_run(const AttnParams& p, int bank, int nb, int f, int h, int seg, int q0, int rows,
                                                int DH, int nthreads) {
    const int PS = DH + 8;
    for (int id = threadIdx.x; id < nb * rows * PS; id += nthreads) {
        const int vb = id / (rows * PS), r = (id / PS) % rows, c = id % PS;
        if (q0 + r >= p.S) continue;
        const int64_t R = (((int64_t)(bank + vb) * p.Kq + f) * p.H + h) * p.S + q0 + r;
        p.partials[(R * p.pslots + seg) * PS + c] = c == DH + 1 ? -INFINITY : 0.f;
    }
}

// Frame-set keyframe bank (tf_ext_attn_fwd_frame_sets): the launch's parameter block with one 64-bit member mask per query
// frame behind it -- bit j of set[i]: the bank branches of query frame i read the keys of bank frame j.  A type of its own
// again (every plain and windowed launch keeps its parameter block and its code); the table rides in the kernel arguments,
// a workgroup reads its query frame's mask with one scalar load.
struct AttnParamsSet : AttnParams {
    uint64_t set[TF_MAX_WINDOW_FRAMES];
};
template <typename P>
constexpr bool is_set = std::is_same<P, AttnParamsSet>::value;

// Frame-set launches, key frames of a bank problem: run `seg` of nseg takes members [seg n / nseg, (seg + 1) n / nseg) of the
// ascending member list of query frame f's set (n = its popcount); returned as a mask, n_fr = its members.  A set shorter than
// nseg leaves some runs empty.  Everything here depends on kernel arguments and the workgroup index only: scalar code.
__device__ __forceinline__ uint64_t set_run(const AttnParamsSet& p, int f, int seg, int nseg, int& n_fr) {
    uint64_t m = p.set[f];
    const int n = __builtin_popcountll(m);
    const int lo = (seg * n) / nseg, hi = ((seg + 1) * n) / nseg;
    for (int i = 0; i < lo; ++i) m &= m - 1;   // drop the members in front of the run
    uint64_t rest = m;
    for (int i = lo; i < hi; ++i) rest &= rest - 1;   // ... and those behind it
    n_fr = hi - lo;
    return m & ~rest;
}

// Frame-set launches: the frame side of a tile cursor.  A streaming kernel moves its K and its V^T tile pointer by a constant
// at every frame boundary; over a frame set the boundary step is "jump to the next member": hop() returns the bank frames
// skipped on the way there, the caller adds that many frame strides on top of its wrap offset.  The K and the V^T cursor
// advance at different pipeline stages, so each carries a walk of its own; wave-uniform (scalar registers: the remaining
// mask and the frame the cursor stands in).
struct SetWalk {
    uint64_t rest;   // members behind the current one
    int cur;         // bank frame of the current member
    __device__ __forceinline__ void init(uint64_t run) {
        cur = __builtin_ctzll(run);
        rest = run & (run - 1);
    }
    __device__ __forceinline__ int hop() {
        // behind the last member there is nothing to jump to: the pointer moves on by one frame and is never read again
        const int next = rest ? __builtin_ctzll(rest) : cur + 1;
        const int skip = next - cur - 1;
        rest &= rest - 1;
        cur = next;
        return skip;
    }
};

// Score bound of a frame-set problem: max |k|^2 over the 64-key blocks of the MEMBER frames only (not of the span from the
// first to the last member: a superset would give another shift than the frame's own call on the gathered members takes; the
// maximum over the same values in another order is the same number).  `base` = the norm row of the problem's (branch, head).
__device__ __forceinline__ float set_knorm2(const float* base, uint64_t run, int ppf, int lane) {
    float kn2 = 0.f;
    for (uint64_t m = run; m; m &= m - 1) {
        const float* part = base + (int64_t)__builtin_ctzll(m) * ppf;
        for (int i = lane; i < ppf; i += 64) kn2 = fmaxf(kn2, part[i]);
    }
    return kn2;
}

// max over the two lanes (l, l ^ 32) that share a query: v_permlane32_swap instead of an LDS round trip
__device__ __forceinline__ float max_with_lane_xor32(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// Row stride (elements) of the V^T scratch: K*Spad positions + 64 elements of padding.  K*Spad*2 bytes is a
// large power of two at the BASELINE shapes (64 KiB at cfg2 level 0); the rows d = 0..Dh-1 of one V^T tile
// would then all map to the same memory channel and the tile loads serialise.  The 128-byte skew spreads them.
__host__ __device__ __forceinline__ int64_t vt_row_stride(int K, int Spad) { return (int64_t)K * Spad + 64; }

static inline size_t vt_bytes(int K, int Spad, int H, int Dh, int branches = 3) {
    return (size_t)branches * H * Dh * (size_t)vt_row_stride(K, Spad) * 2;
}

// 4 consecutive output features of one query: rounded to the 16-bit I/O type, or, with TF_ATTN_OUT_F32, the
// normalised fp32 accumulator itself (the caller's `out` is then float [3,Kq,S,H*Dh])
template <typename E, typename V4>
__device__ __forceinline__ void store_out4(void* out, int64_t elem_off, f32x4 x, int out_f32) {
    if (out_f32) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + elem_off) = x;
    } else {
        V4 w;
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = (E)x[i];
        *reinterpret_cast<u32x2*>(reinterpret_cast<E*>(out) + elem_off) = __builtin_bit_cast(u32x2, w);
    }
}

// Plan-token mark of a launch that leaves partial results for tf_ext_attn_runs_merge (a run call's SOURCE launch writes the
// final output and carries no mark)
template <int MODE>
static inline const char* run_mark(const AttnParams& p) { return (p.run && MODE != MODE_SOURCE) ? ",run" : ""; }

// A windowed launch (AttnParamsWin) exists for the launches that hold bank problems and that a windowed call can reach: the
// ALL and DUAL forms (tf_ext_attn_fwd_windows) and the four-bank form of a pair of injecting edits
// (tf_ext_attn_fwd_windows_edits: the four banks of a workgroup read the SAME window, their query frame's).  Its source-only
// launches are the plain ones (a source problem reads its own frame whatever the windows); the run forms take no windows.
// Plan token: the plain launch's with ",win" appended.
template <typename P, int MODE, bool RUN = false>
constexpr bool win_launch = is_win<P> && (MODE == MODE_ALL || MODE == MODE_DUAL || MODE == MODE_MV4) && !RUN;

// A frame-set launch (AttnParamsSet) likewise: the ALL and DUAL forms (tf_ext_attn_fwd_frame_sets) and the four-bank form of a
// pair of injecting edits (tf_ext_attn_fwd_frame_sets_edits: the four banks of a workgroup walk the SAME member frames, their
// query frame's set, and take every hop together).  Plan token: the plain launch's with ",set" appended.
template <typename P, int MODE, bool RUN = false>
constexpr bool set_launch = is_set<P> && (MODE == MODE_ALL || MODE == MODE_DUAL || MODE == MODE_MV4) && !RUN;

// The parameter block a launch hands its kernel: the caller's where the launch has a windowed / frame-set instantiation, the
// plain one otherwise; and the mark its plan token carries
template <typename P, int MODE, bool RUN = false>
using launch_params_t = std::conditional_t<win_launch<P, MODE, RUN> || set_launch<P, MODE, RUN>, P, AttnParams>;
template <typename P>
static inline const char* table_mark() { return is_win<P> ? ",win" : is_set<P> ? ",set" : ""; }

}  // namespace
