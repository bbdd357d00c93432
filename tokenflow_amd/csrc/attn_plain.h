// Extended attention, the plain streaming kernel: one 32-query tile per wave, 64-key tiles, QK^T -> softmax -> P.V back to
// back (structure and MFMA mapping: the head of ext_attn.hip).  Included by ext_attn.hip only.
#pragma once

#include "attn_common.h"

namespace {

// QT   = 32-query tiles per wave: always 1.  KT = keys per staged tile: always 64.  Both stay template parameters, pinned
//        by the static_assert below: writing the kernel without its one-trip loops over them changes hipcc's code for
//        every instantiation (VGPRs -4 .. +6, code size -0.8 .. +2.3 %; profiles/r17_attn_refactor_codegen.md)
// NW   = waves per workgroup (4 or 8): a workgroup covers 32*QT*NW queries of one (branch, frame, head)
//        and shares every staged K / V^T tile among them
// MODE = MODE_ALL:    every (branch, frame, head, query tile) problem, bank problems first
//        MODE_SOURCE: only the source-branch problems
//        MODE_DUAL:   q/k injection active -- uncond and cond share q, k, the scores and P
//                     (tokenflow_utils.py:124-130), so ONE workgroup computes both: QK^T and the softmax
//                     once, two P.V products against the two V banks (NB = 2).
//        MODE_MV4:    multi-edit batch under injection (Dh = 40, 64): the uncond and cond branches of TWO edits share the
//                     source q and k, so one workgroup does QK^T and the softmax once and FOUR P.V products (NB = 4)
//                     against the banks of branches b, b + 1, b + gap, b + gap + 1 of the V^T image (p.gap = 2: neighbouring
//                     edits; the masked multi-edit call pairs the INJECTING edits, whatever lies between them).
//                     Dh = 40: the packed image (PACK below).  Dh = 64: four 64-row banks side by side, 8 M-tiles, one row
//                     sum for all four (no ones row), the scores taken per 32-key half (HALF below).
//                     Over a frame set (P = AttnParamsSet) the K cursor and all four V^T cursors hop together in stage_load;
//                     everything else that looks at a tile's position -- the ragged masking, the HALF steps, the PACK image
//                     -- works on the tile index INSIDE its frame (tt_cur, ld_tt), which a hop does not touch.
// MINW = min waves per SIMD for the register allocator
// FQ   = fold the softmax scale into Q (see FOLD below; opt-in, TF_ATTN_FOLD_SCALE); false = the default, fp32
//        scaling of the scores as the reference does (tokenflow_utils.py:173-175 `* self.scale` on the bmm output)
// SB   = single LDS buffer (two barriers per tile) instead of two: half the LDS per workgroup.  For head dim 160, where
//        the double-buffered tiles (89 KB) allow ONE workgroup per CU and a wave waits alone for every 1 KB fragment
template <typename T, int DH, int QT, int NW, int MODE, int MINW, int KT, bool FQ, bool SB = false, typename P = AttnParams>
__global__ __launch_bounds__(64 * NW, MINW) void ext_attn_kernel(P p) {
    static_assert(QT == 1 && KT == 64, "launch_one instantiates one query tile per wave and 64-key tiles only");
    typedef AttnCfg<DH, KT> C;
    typedef typename T::elem E;
    typedef typename T::vec8 vec8;
    typedef typename T::vec4 vec4;
    constexpr int NT = 64 * NW;
    constexpr int NB = MODE == MODE_DUAL ? 2 : MODE == MODE_MV4 ? 4 : 1;   // V banks handled by this workgroup
    constexpr bool SHARED = MODE == MODE_DUAL || MODE == MODE_MV4;          // one softmax feeds NB P.V products
    static_assert(MODE != MODE_MV4 || DH == 40 || DH == 64, "the four-bank form exists at head dims 40 and 64");
    constexpr int NPK = C::npk(NT), NPV = C::npv(NT);
    constexpr int NBUFS = SB ? 1 : 2;
    // PACK (dual-V at Dh = 40): the two banks' V^T rows share ONE LDS image of 3 M-tiles -- rows 0-39 uncond,
    // 40-79 cond, row 80 = 1.0 (the common denominator row), 81-95 zero -- instead of two images of 2 M-tiles
    // with 24 idle rows each: 12 instead of 16 P.V MFMAs per 64-key tile (18 instead of 22 with QK^T).
    // Four banks: rows 0-159 the banks, row 160 = 1.0, 161-191 zero -- 6 M-tiles, 24 P.V MFMAs for four outputs.
    constexpr bool PACK = SHARED && DH == 40;
    constexpr int NG = (NB * DH + 1 + 31) / 32;                // PACK: M-tiles of the packed image (3 / 6)
    constexpr int VIMG_ROWS = PACK ? NG * 32 : NB * C::VROWS;  // V^T rows of one LDS buffer
    constexpr int VB_ROWS = PACK ? DH : C::VROWS;              // row offset between the banks inside it
    constexpr int BUF_ELEMS = C::K_ELEMS + VIMG_ROWS * C::VROW;
    // When the head dim is not a multiple of 32 the last PV M-tile has unused rows: row DH of the
    // V^T image is set to 1.0, so that accumulator row collects sum_k P[k] -- the softmax
    // denominator comes out of the MFMA for free, summed over the SAME rounded P as the numerator.
    // At the other head dims (64) the VALU sums the rounded P too (l_run): see the tile loop.
    constexpr bool ONES = (DH % 32) != 0;
    constexpr int ONES_R = ((DH % 32) & 3) + 4 * ((DH % 32) >> 3);  // C/D register of row DH%32 (lane half 0)
    static_assert(!ONES || ((DH % 32) & 4) == 0, "row DH must live in lane half 0");
    // FOLD (head dims with spare QK^T columns, i.e. Dh = 40): the softmax's scale AND shift ride in the MFMA.
    //   * Q fragments hold q * (scale*log2 e), rounded to the MFMA input type once per kernel;
    //   * the first pad column of the K image (column Dh) is 1.0 and the matching pad element of the Q
    //     fragment holds -shift, so the accumulator comes out as  s*c - shift  and P = exp2(acc) directly:
    //     no v_fma per score (32 of ~87 VALU instructions per 32x64 tile; the kernel is VALU-issue bound).
    //   The shift is a per-query running value, representable in the input type, moved only when a tile's
    //   maximum exceeds it by more than FOLD_T (and always on the first tile); softmax is invariant to the
    //   shift, numerator and denominator see the same P, so no accuracy is traded for the deferral.
    //   What IS traded: q*c is rounded to 16 bit once, a relative error <= 2^-9 per element that perturbs each
    //   score by ~2^-9/sqrt(3) * c * sqrt(sum_d (q_d k_d)^2) -- the size class of the P rounding for ordinary
    //   scores, but 3-12x the whole error budget on peaked softmaxes (logit std 4-16, profiles/r02_fold_accuracy.txt):
    //   NOT the default; TF_ATTN_FOLD_SCALE opts in.
    constexpr bool FOLD = FQ && ONES && (C::DKP > DH);
    constexpr int SH_T = DH / 16, SH_HI = (DH % 16) / 8;   // k-step and lane half that hold column Dh
    //   Most tiles never look at their maximum: |acc + shift| = |q'.k| <= |q'| max_k|k| (Cauchy-Schwarz; the
    //   key norm bound comes with the vt_pack_kernel pre-pass), so while  |q'| |k|max - shift <= FOLD_T  no
    //   score of any tile can exceed the threshold and the max3 chain + permlane (16 of ~66 VALU per tile)
    //   is skipped; a query whose bound is loose falls back to the per-tile maximum.  exp2 of FOLD_T must
    //   stay inside the input type's range (the row sum is accumulated in fp32): 2^60 for bf16, 2^14 for f16
    //   (f16 tops out at 65504; on N(0,1) data the f16 bound is usually too loose to skip anything, and a
    //   per-tile bound from the block's own max |k| measured slower than the fallback it avoids).
    //   Measured (MI355X, cfg2 level 0): -6.5 % kernel time for +7..15 us in the pre-pass.
    constexpr float FOLD_T = std::is_same<E, _Float16>::value ? 14.0f : 60.0f;
    // BOUND (Dh = 40, both scalings): the Cauchy-Schwarz score bound described above lets a wave skip the per-tile
    // maximum.  With fp32 scaling the running "maximum" m_run becomes a deferred shift exactly as in the folded
    // form: it is set from the first tile's maximum and moved only when a tile maximum exceeds it by more than
    // FOLD_T binades; P = exp2((s - m_run) c) may then exceed 1 (<= 2^FOLD_T), numerator and denominator see the
    // same P.  Saves the 16 v_max3 + permlane of most tiles and most O rescales.
    //   Measured (round 2, cfg2 level 0, fp32 scaling): 4.25 -> 4.03 ms with the bound; the folded form is 3.58 ms.
    constexpr bool BOUND = attn_has_bound(DH);
    constexpr bool HALF = MODE == MODE_MV4 && DH == 64;   // scores per 32-key half (see the tile loop)

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    auto sK = [&](int buf) { return reinterpret_cast<E*>(smem) + buf * BUF_ELEMS; };
    auto sV = [&](int buf, int vb) {
        return reinterpret_cast<E*>(smem) + buf * BUF_ELEMS + C::K_ELEMS + vb * VB_ROWS * C::VROW;
    };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hi = lane >> 5;
    const int l31 = lane & 31;
    const int K = p.K, Kq = p.Kq, S = p.S, H = p.H;

    // ---- problem decode
    const int h = blockIdx.x % H;
    int u = blockIdx.x / H;
    int b, f, qt;  // f = query frame, local index in [0, Kq)
    int seg = 0;   // run of bank frames this workgroup covers (split form: the bank problems come nseg times)
    const int nseg = MODE == MODE_SOURCE ? 1 : p.nseg;
    if constexpr (MODE == MODE_ALL) {   // bank problems (uncond, cond) first, then the short source ones
        const int nbank = 2 * Kq * p.nQT * nseg;
        if (u < nbank) {
            seg = u % nseg;
            u /= nseg;
            b = 1 + u / (Kq * p.nQT);
            u -= (b - 1) * Kq * p.nQT;
        } else {
            u -= nbank;
            b = 0;
        }
    } else if constexpr (SHARED) {
        b = 1;
        seg = u % nseg;
        u /= nseg;
    } else {
        b = 0;
    }
    f = u / p.nQT;
    qt = u - f * p.nQT;
    const int bq = (p.inject && b > 0) ? 0 : b;  // branch whose q and k are used (tokenflow_utils.py:124-130)
    const bool split = p.pslots > 0 && b > 0;
    int f_lo = b == 0 ? p.q_frame0 + f : (seg * K) / nseg;
    int n_fr = b == 0 ? 1 : ((seg + 1) * K) / nseg - f_lo;
    if constexpr (is_win<P>) {   // a bank problem reads its query frame's window of the bank
        if (b > 0) window_range(p, f, seg, nseg, f_lo, n_fr);
        if (n_fr == 0) {   // a window shorter than the split: this run holds no frame (never in the four-bank form, whose
                           // launches are one-pass: nseg = 1 and a window holds at least its own frame)
            write_empty_run(p, b - 1, NB, f, h, seg, qt * (32 * QT * NW), 32 * QT * NW, DH, NT);
            return;
        }
    }
    [[maybe_unused]] uint64_t run = 0;   // frame-set launches: the member frames of this problem (see set_run, SetWalk)
    if constexpr (is_set<P>) {   // a bank problem reads the member frames of its query frame's set, in ascending order
        run = (uint64_t)1 << f_lo;   // (a source problem: its own frame)
        if (b > 0) {
            run = set_run(p, f, seg, nseg, n_fr);
            if (n_fr == 0) {   // a set shorter than the split: this run holds no member (never in the four-bank form, whose
                               // launches are one-pass: nseg = 1 and a set holds at least its own frame)
                write_empty_run(p, b - 1, NB, f, h, seg, qt * (32 * QT * NW), 32 * QT * NW, DH, NT);
                return;
            }
            f_lo = __builtin_ctzll(run);
        }
    }
    const int tpf = (S + KT - 1) / KT;  // staged tiles per frame
    const int ntiles = n_fr * tpf;
    const bool ragged = (S % KT) != 0;

    const E* qg = reinterpret_cast<const E*>(p.q);
    const E* kg = reinterpret_cast<const E*>(p.k) + bq * p.k_bs + h * DH;
    const int64_t vt_row = vt_row_stride(p.Kb, p.Spad);
    // branch of V bank vb relative to b: consecutive branches, except that the second edit of a four-bank launch starts
    // p.gap branches behind the first (gap = 2: neighbours)
    auto bank_off = [&](int vb) { return (MODE == MODE_MV4 && vb >= 2) ? vb + (p.gap - 2) : vb; };
    const E* vg[NB];
#pragma unroll
    for (int vb = 0; vb < NB; ++vb)
        vg[vb] = reinterpret_cast<const E*>(p.vt) + ((int64_t)((b + bank_off(vb)) * H + h) * DH) * vt_row;

    // ---- LDS pads, written once and never staged over: K columns DH..DKP-1 = 0,
    //      V^T rows DH..VROWS-1 = 0 except row DH = 1 (denominator row) when ONES.
    if constexpr (C::DKP > DH) {
        for (int id = tid; id < NBUFS * KT * (C::DKP - DH); id += NT) {
            const int bufi = id / (KT * (C::DKP - DH));
            const int r = (id / (C::DKP - DH)) % KT, cidx = id % (C::DKP - DH);
            sK(bufi)[r * C::KROW + DH + cidx] = (E)((FOLD && cidx == 0) ? 1.f : 0.f);
        }
    }
    if constexpr (PACK) {
        for (int id = tid; id < NBUFS * (VIMG_ROWS - NB * DH) * KT; id += NT) {
            const int bufi = id / ((VIMG_ROWS - NB * DH) * KT);
            const int r = (id / KT) % (VIMG_ROWS - NB * DH), cidx = id % KT;
            sV(bufi, 0)[(NB * DH + r) * C::VROW + cidx] = (E)(r == 0 ? 1.f : 0.f);
        }
    } else if constexpr (C::VROWS > DH) {
        for (int id = tid; id < NBUFS * NB * (C::VROWS - DH) * KT; id += NT) {
            const int bv = id / ((C::VROWS - DH) * KT);
            const int r = (id / KT) % (C::VROWS - DH), cidx = id % KT;
            sV(bv / NB, bv % NB)[(DH + r) * C::VROW + cidx] = (E)((ONES && r == 0) ? 1.f : 0.f);
        }
    }

    // ---- Q fragments (B operand of S^T = K Q^T), resident for the whole kernel
    int q_row[QT];
    bool q_ok[QT];
    vec8 qf[QT][C::KS];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        q_row[qi] = qt * (32 * QT * NW) + (wave * QT + qi) * 32 + l31;
        q_ok[qi] = q_row[qi] < S;
        const E* qp = qg + bq * p.q_bs + f * p.q_fs + (int64_t)(q_ok[qi] ? q_row[qi] : S - 1) * p.ld_q + h * DH;
#pragma unroll
        for (int t = 0; t < C::KS; ++t) {
            const int col = 16 * t + 8 * hi;
            qf[qi][t] = __builtin_bit_cast(vec8, col < DH ? ld16(qp + col) : u32x4{0, 0, 0, 0});
            if constexpr (FOLD) {   // q * (scale*log2 e), rounded once to the MFMA input type
#pragma unroll
                for (int j = 0; j < 8; ++j) qf[qi][t][j] = (E)((float)qf[qi][t][j] * p.c);
            }
        }
    }
    float s_bound[QT] = {};   // BOUND: upper bound of q.k*c (log2 units) over every key of the bank (1.001 covers fp32 rounding)
    if constexpr (BOUND) {
        const int ppf = p.Spad / 64;   // 64-key blocks per frame; this problem sees frames f_lo .. f_lo + n_fr - 1
        const float* part = p.knorm2 + ((int64_t)(bq * H + h) * p.Kb + f_lo) * ppf;
        float kn2 = 0.f;
        if constexpr (is_set<P>) kn2 = set_knorm2(part - (int64_t)f_lo * ppf, run, ppf, lane);   // the member frames' blocks only
        else
            for (int i = lane; i < n_fr * ppf; i += 64) kn2 = fmaxf(kn2, part[i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) kn2 = fmaxf(kn2, __shfl_xor(kn2, o));
        const float kn = __builtin_sqrtf(kn2) * 1.001f;
#pragma unroll
        for (int qi = 0; qi < QT; ++qi) {
            float q2 = 0.f;
#pragma unroll
            for (int t = 0; t < C::KS; ++t)
#pragma unroll
                for (int j = 0; j < 8; ++j) q2 = fmaf((float)qf[qi][t][j], (float)qf[qi][t][j], q2);
            q2 += __shfl_xor(q2, 32);   // the two lanes of a query hold disjoint halves of its columns
            s_bound[qi] = __builtin_sqrtf(q2) * kn * (FOLD ? 1.f : p.c);   // log2 units in both forms
        }
    }

    // ---- staging: per-thread piece offsets are loop-invariant; a tile only moves uniform base pointers
    // The loads are branch-free (one straight-line path, no exec masking): a lane without a piece re-loads
    // the last piece, a row past S is clamped by a select.  Any control flow around the loads makes the
    // compiler merge the two definitions of the staging registers with v_mov copies, and those copies
    // need the data: an s_waitcnt vmcnt(0) right behind the loads that exposes the full L2 latency on
    // every tile (measured ~0.8 ms of a 4.2 ms launch).
    u32x4 rk[NPK], rv[NB][NPV];
    int k_row[NPK], k_col[NPK], k_goff[NPK], k_loff[NPK], v_goff[NPV], v_loff[NPV];
#pragma unroll
    for (int i = 0; i < NPK; ++i) {
        const int id = min(tid + NT * i, KT * C::PPR - 1);
        k_row[i] = id / C::PPR;
        k_col[i] = (id - k_row[i] * C::PPR) * 8;
        k_goff[i] = k_row[i] * (int)p.ld + k_col[i];
        k_loff[i] = k_row[i] * C::KROW + k_col[i];
    }
#pragma unroll
    for (int i = 0; i < NPV; ++i) {
        const int id = min(tid + NT * i, DH * C::VPR - 1);
        v_goff[i] = (id / C::VPR) * (int)vt_row + (id % C::VPR) * 8;
        v_loff[i] = (id / C::VPR) * C::VROW + (id % C::VPR) * 8;
    }
    // Tile cursors (see ext_attn_pp_kernel): uniform pointer bumps, no division per tile.
    const int k_wrap = S - (tpf - 1) * KT, v_wrap = p.Spad - (tpf - 1) * KT;
    const int64_t k_wrap_off = p.k_fs - (int64_t)(tpf - 1) * KT * p.ld;   // last tile of a frame -> first tile of the next
    const E* k_next = kg + f_lo * p.k_fs;
    const E* v_next[NB];
#pragma unroll
    for (int vb = 0; vb < NB; ++vb) v_next[vb] = vg[vb] + (int64_t)f_lo * p.Spad;
    int ld_tt = 0;
    [[maybe_unused]] SetWalk walk{};   // frame-set launches: K and V^T move together here, one walk serves both
    if constexpr (is_set<P>) walk.init(run);
    auto stage_load = [&]() {
        const bool wrap = ld_tt == tpf - 1;
        const int rlim = wrap ? k_wrap - 1 : KT - 1;   // last valid key row of this tile (rows past S are masked later)
        const int clamp_off = rlim * (int)p.ld;
#pragma unroll
        for (int i = 0; i < NPK; ++i) rk[i] = ld16(k_next + (k_row[i] <= rlim ? k_goff[i] : clamp_off + k_col[i]));
#pragma unroll
        for (int vb = 0; vb < NB; ++vb) {
#pragma unroll
            for (int i = 0; i < NPV; ++i) rv[vb][i] = ld16(v_next[vb] + v_goff[i]);
            v_next[vb] += wrap ? v_wrap : KT;
        }
        k_next += wrap ? k_wrap_off : (int64_t)KT * p.ld;
        if constexpr (is_set<P>) {
            if (wrap) {   // the next member frame: the frames between it and this one are skipped
                const int skip = walk.hop();
                k_next += (int64_t)skip * p.k_fs;
#pragma unroll
                for (int vb = 0; vb < NB; ++vb) v_next[vb] += (int64_t)skip * p.Spad;
            }
        }
        ld_tt = wrap ? 0 : ld_tt + 1;
    };
    auto stage_write = [&](int buf) {
        E* kb = sK(buf);
#pragma unroll
        for (int i = 0; i < NPK; ++i)
            if (tid + NT * i < KT * C::PPR) st16(kb + k_loff[i], rk[i]);
#pragma unroll
        for (int vb = 0; vb < NB; ++vb) {
            E* vbp = sV(buf, vb);
#pragma unroll
            for (int i = 0; i < NPV; ++i)
                if (tid + NT * i < DH * C::VPR) st16(vbp + v_loff[i], rv[vb][i]);
        }
    };

    f32x16 o[NB][QT][C::MT];
    float m_run[QT], l_run[QT];  // running max of the RAW scores (scale > 0); this lane's share of the denominator
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        m_run[qi] = FOLD ? 0.f : -INFINITY;   // FOLD: the current shift
        l_run[qi] = 0.f;
#pragma unroll
        for (int vb = 0; vb < NB; ++vb)
#pragma unroll
            for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[vb][qi][mt][r] = 0.f;
    }
    const float c = p.c;
    const f32x2 c2 = {c, c};

    stage_load();
    __syncthreads();  // pad fill visible before anything reads; staging regions are disjoint from the pads
    stage_write(0);
    __syncthreads();

    int tt_cur = 0;   // tile index within the frame of the tile being computed
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = SB ? 0 : tile & 1;
        const bool has_next = tile + 1 < ntiles;
        if (has_next) stage_load();

#pragma unroll
        for (int sub = 0; sub < C::SUB; ++sub) {
            const int key0 = tt_cur * KT + sub * 64;  // first key (within the frame) of this 64-key sub-tile
            if (C::SUB > 1 && ragged && key0 >= S) break;   // nothing but padding left in this tile
            if constexpr (HALF) {
                // Four banks at Dh = 64: 128 accumulator registers.  The scores are taken per 32-key half -- QK^T, softmax and the
                // two P.V k-steps of one half before the next -- so 16 score and 8 P registers are live instead of 32 and 16.
                // Every half is a step of the online softmax of its own (reference point and row sum as below, BOUND form).
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    f32x16 sh;
#pragma unroll
                    for (int r = 0; r < 16; ++r) sh[r] = 0.f;
#pragma unroll
                    for (int t = 0; t < C::KS; ++t) {
                        const E* krow = sK(buf) + (sub * 64 + kt * 32 + l31) * C::KROW + 8 * hi;
                        sh = T::mfma32(__builtin_bit_cast(vec8, ld16(krow + 16 * t)), qf[0][t], sh);
                    }
                    if (ragged && key0 + kt * 32 + 32 > S) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (key0 + kt * 32 + cd_row(r, hi) >= S) sh[r] = -INFINITY;
                    }
                    static_assert(BOUND && !FOLD && !ONES && QT == 1, "the half-tile steps are written for the Dh = 64 bound form");
                    // (a second half that lies wholly in the padding never looks: it has no maximum, and P = 0 whatever the reference.
                    // The test is uniform and costs nothing -- and without it hipcc's register allocation of this kernel spills)
                    if (__any(s_bound[0] - m_run[0] * c > FOLD_T) && !(ragged && key0 + kt * 32 >= S)) {
                        float mx = sh[0];
#pragma unroll
                        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sh[r]);
                        mx = max_with_lane_xor32(mx);
                        const bool over = (mx - m_run[0]) * c > FOLD_T;
                        if (__any(over)) {
                            const float m_new = over ? mx : m_run[0];
                            const float alpha = __builtin_amdgcn_exp2f((m_run[0] - m_new) * c);  // exp2(-inf) = 0 on the first half
                            m_run[0] = m_new;
                            l_run[0] *= alpha;
#pragma unroll
                            for (int vb = 0; vb < NB; ++vb)
#pragma unroll
                                for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                                    for (int r = 0; r < 16; ++r) o[vb][0][mt][r] *= alpha;
                        }
                    }
                    const float mc = m_run[0] * c;
                    const f32x2 mc2 = {mc, mc};
                    vec8 ph[2];
                    float lsum = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const f32x2 x = f32x2{sh[r], sh[r + 1]} * c2 - mc2;
                        const float p0 = __builtin_amdgcn_exp2f(x[0]);
                        const float p1 = __builtin_amdgcn_exp2f(x[1]);
                        // the denominator is summed from the ROUNDED P, the values the P.V MFMA multiplies: with a reference
                        // point below the maximum (lag, deferred shift) the largest P is no power of two, and only a common
                        // rounding of numerator and denominator cancels in a peaked softmax
                        const E e0 = (E)p0, e1 = (E)p1;
                        lsum += (float)e0 + (float)e1;
                        ph[r >> 3][r & 7] = e0;
                        ph[r >> 3][(r & 7) + 1] = e1;
                    }
                    l_run[0] += lsum;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks)   // k-step outermost: round-robin over the 8 accumulators
#pragma unroll
                        for (int vb = 0; vb < NB; ++vb)
#pragma unroll
                            for (int mt = 0; mt < C::MT; ++mt) {
                                const E* vrow = sV(buf, vb) + (mt * 32 + l31) * C::VROW + sub * 64 + 8 * hi;
                                o[vb][0][mt] = T::mfma32(__builtin_bit_cast(vec8, ld16(vrow + 16 * (2 * kt + ks))), ph[ks],
                                                         o[vb][0][mt]);
                            }
                }
                continue;
            }
            // Program order per tile: QK(q0) QK(q1) | softmax(q0) PV(q0) | softmax(q1) PV(q1).
            // MFMAs execute asynchronously behind the in-order issue, so the softmax VALU of one query
            // tile runs while the matrix pipe works on the other one's QK^T / P.V.
            f32x16 s[QT][2];  // S^T tiles: 64 keys x 32 queries each
#pragma unroll
            for (int qi = 0; qi < QT; ++qi)
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[qi][kt][r] = 0.f;
            // k-step outermost: consecutive MFMAs hit DIFFERENT accumulators (two MFMAs on the same accumulator
            // with other instructions between them cost ~43 extra cycles, MI355X_MICROARCH.md cycle constants)
#pragma unroll
            for (int t = 0; t < C::KS; ++t)
#pragma unroll
                for (int qi = 0; qi < QT; ++qi)
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt) {
                        const E* krow = sK(buf) + (sub * 64 + kt * 32 + l31) * C::KROW + 8 * hi;
                        s[qi][kt] = T::mfma32(__builtin_bit_cast(vec8, ld16(krow + 16 * t)), qf[qi][t], s[qi][kt]);
                    }
            if (ragged && key0 + 64 > S) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (key0 + kt * 32 + cd_row(r, hi) >= S) {
#pragma unroll
                            for (int qi = 0; qi < QT; ++qi) s[qi][kt][r] = -INFINITY;
                        }
            }

#pragma unroll
            for (int qi = 0; qi < QT; ++qi) {
                // ---- online softmax (lane-local; the two lanes of a query share m)
                auto tile_max = [&]() {
                    float mx = s[qi][0][0];
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[qi][kt][r]);
                    return max_with_lane_xor32(mx);
                };
                vec8 pf[4];
                if constexpr (FOLD) {
                    // s already is  score*c - shift.  Move the shift only when needed (wave-uniform branches).
                    const bool first = tile == 0 && sub == 0;
                    float delta = 0.f;
                    float mx = 0.f;
                    const bool look = !BOUND || first || __any(s_bound[qi] - m_run[qi] > FOLD_T);
                    if (look) mx = tile_max();
                    if (look && (first || __any(mx > FOLD_T))) {
                        const float sh_old = m_run[qi];          // m_run holds the current shift (0 before tile 0)
                        const float sh_new = (first || mx > FOLD_T) ? (float)(E)(sh_old + mx) : sh_old;
                        delta = sh_new - sh_old;
                        // first tile: O is still zero, and exp2(-delta) overflows to +inf when every score of the
                        // tile is far below zero (0 * inf = NaN) -- nothing to rescale there
                        const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-delta);
                        m_run[qi] = sh_new;
                        if (hi == SH_HI) qf[qi][SH_T][0] = (E)(-sh_new);
#pragma unroll
                        for (int vb = 0; vb < NB; ++vb)
#pragma unroll
                            for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                                for (int r = 0; r < 16; ++r) o[vb][qi][mt][r] *= alpha;
#pragma unroll
                        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) s[qi][kt][r] -= delta;
                    }
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            pf[kt * 2 + (r >> 3)][r & 7] = (E)__builtin_amdgcn_exp2f(s[qi][kt][r]);
                } else {
                    bool move;      // wave-uniform: some query's shift / running maximum changes on this tile
                    float m_new;
                    if constexpr (BOUND) {
                        // m_run = deferred shift (raw-score units; -inf before the first tile, so the first tile
                        // always looks and always moves).  No tile can overflow while (bound - shift) <= FOLD_T.
                        const bool look = __any(s_bound[qi] - m_run[qi] * c > FOLD_T);
                        move = false;
                        m_new = m_run[qi];
                        if (look) {
                            const float mx = tile_max();
                            const bool over = (mx - m_run[qi]) * c > FOLD_T;
                            move = __any(over);
                            if (over) m_new = mx;
                        }
                    } else {
                        // reference point = running maximum with a lag of 8 binades (see ext_attn_il_kernel): per-query
                        // decision, alpha == 1 exactly for a query whose reference stays
                        const float mx = tile_max();
                        const bool over = mx > m_run[qi] + TF_ATTN_LAG / c;
                        move = __any(over);
                        m_new = over ? mx : m_run[qi];
                    }
                    if (move) {
                        const float alpha = __builtin_amdgcn_exp2f((m_run[qi] - m_new) * c);  // exp2(-inf) = 0 on tile 0
                        m_run[qi] = m_new;
                        if constexpr (!ONES) l_run[qi] *= alpha;
#pragma unroll
                        for (int vb = 0; vb < NB; ++vb)
#pragma unroll
                            for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                                for (int r = 0; r < 16; ++r) o[vb][qi][mt][r] *= alpha;
                    }
                    const float mc = m_run[qi] * c;
                    const f32x2 mc2 = {mc, mc};
                    float lsum = 0.f;
#pragma unroll
                    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                        for (int r = 0; r < 16; r += 2) {
                            // v_pk_fma_f32: 16 instead of 32 VALU per tile (two scalar v_fma measured +16 % kernel time)
                            const f32x2 x = f32x2{s[qi][kt][r], s[qi][kt][r + 1]} * c2 - mc2;
                            const float p0 = __builtin_amdgcn_exp2f(x[0]);
                            const float p1 = __builtin_amdgcn_exp2f(x[1]);
                            const E e0 = (E)p0, e1 = (E)p1;
                            if constexpr (!ONES) lsum += (float)e0 + (float)e1;   // the rounded P, as the ones row sums it
                            pf[kt * 2 + (r >> 3)][r & 7] = e0;
                            pf[kt * 2 + (r >> 3)][(r & 7) + 1] = e1;
                        }
                    if constexpr (!ONES) l_run[qi] += lsum;
                }
                // ---- O^T += V^T . P  (once per V bank)
                if constexpr (PACK) {   // NG M-tiles over the packed image: accumulators o[0][.][0], o[0][.][1], o[1][.][0] ...
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                        for (int g = 0; g < NG; ++g) {
                            const E* vrow = sV(buf, 0) + (g * 32 + l31) * C::VROW + sub * 64 + 8 * hi;
                            o[g >> 1][qi][g & 1] = T::mfma32(__builtin_bit_cast(vec8, ld16(vrow + 16 * ks)), pf[ks],
                                                             o[g >> 1][qi][g & 1]);
                        }
                } else {
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks)   // k-step outermost: round-robin over the NB * MT accumulators
#pragma unroll
                        for (int vb = 0; vb < NB; ++vb)
#pragma unroll
                            for (int mt = 0; mt < C::MT; ++mt) {
                                const E* vrow = sV(buf, vb) + (mt * 32 + l31) * C::VROW + sub * 64 + 8 * hi;
                                o[vb][qi][mt] = T::mfma32(__builtin_bit_cast(vec8, ld16(vrow + 16 * ks)), pf[ks],
                                                          o[vb][qi][mt]);
                            }
                }
            }

        }

        if constexpr (SB) {
            if (has_next) {
                __syncthreads();   // every wave is done reading the tile before it is overwritten
                stage_write(0);
            }
        } else if (has_next) {
            stage_write(buf ^ 1);
        }
        tt_cur = tt_cur == tpf - 1 ? 0 : tt_cur + 1;
        __syncthreads();
    }

    // ---- epilogue: normalise, round, store 4 consecutive d (8 B) per register group
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        float l_tot;
        if constexpr (PACK) {
            // the ones row NB*DH of the image: two banks, row 80 = row 16 of the third M-tile, register 8; four banks, row 160 =
            // row 0 of the sixth M-tile, register 0 -- lane half 0 in both
            constexpr int LG = (NB * DH) / 32, LR = (NB * DH) % 32;
            static_assert((LR & 4) == 0, "the ones row must live in lane half 0");
            l_tot = __shfl(o[LG >> 1][qi][LG & 1][(LR & 3) + 4 * (LR >> 3)], l31);
        } else if constexpr (ONES)
            l_tot = __shfl(o[0][qi][C::MT - 1][ONES_R], l31);  // row DH lives in lane half 0 of the last M-tile
        else
            l_tot = l_run[qi] + __shfl_xor(l_run[qi], 32);
        const float inv_l = 1.0f / l_tot;
        if (split) {
            // split form: this workgroup saw only a run of the bank's frames -- leave the unnormalised O, the
            // denominator and the shift (log2 domain) for attn_merge_kernel
            if (q_ok[qi]) {
                constexpr int PS = DH + 8;
                const float lshift = FOLD ? m_run[qi] : m_run[qi] * c;
                // (four banks: the second edit's rows lie p.gap branches behind the first's, in that edit's own partial region)
                auto row_ptr = [&](int vb) {
                    const int64_t R = (((int64_t)(b - 1 + bank_off(vb)) * Kq + f) * H + h) * S + q_row[qi];
                    return p.partials + (R * p.pslots + seg) * PS;
                };
                if constexpr (PACK) {
#pragma unroll
                    for (int g = 0; g < NG; ++g)
#pragma unroll
                        for (int rg = 0; rg < 4; ++rg) {
                            const int R = g * 32 + 8 * rg + 4 * hi;
                            if (R < NB * DH) {
                                const int vb = R / DH;
                                f32x4 w;
#pragma unroll
                                for (int i = 0; i < 4; ++i) w[i] = o[g >> 1][qi][g & 1][rg * 4 + i];
                                *reinterpret_cast<f32x4*>(row_ptr(vb) + (R - vb * DH)) = w;
                            }
                        }
                } else {
#pragma unroll
                    for (int vb = 0; vb < NB; ++vb)
#pragma unroll
                        for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                            for (int rg = 0; rg < 4; ++rg) {
                                const int d0 = mt * 32 + 8 * rg + 4 * hi;
                                if (d0 < DH) {
                                    f32x4 w;
#pragma unroll
                                    for (int i = 0; i < 4; ++i) w[i] = o[vb][qi][mt][rg * 4 + i];
                                    *reinterpret_cast<f32x4*>(row_ptr(vb) + d0) = w;
                                }
                            }
                }
                if (hi == 0) {
#pragma unroll
                    for (int vb = 0; vb < NB; ++vb) {
                        row_ptr(vb)[DH] = l_tot;
                        row_ptr(vb)[DH + 1] = lshift;
                    }
                }
            }
        } else if (PACK && q_ok[qi]) {
            const int64_t op0 = b * p.o_bs + f * p.o_fs + (int64_t)q_row[qi] * (H * DH) + h * DH;
            const int64_t branch = p.o_bs;
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int R = g * 32 + 8 * rg + 4 * hi;    // image row of this group of 4 (never straddles a bank)
                    if (R < NB * DH) {
                        const int vb = R / DH;
                        f32x4 w;
#pragma unroll
                        for (int i = 0; i < 4; ++i) w[i] = o[g >> 1][qi][g & 1][rg * 4 + i] * inv_l;
                        store_out4<E, vec4>(p.out, op0 + bank_off(vb) * branch + (R - vb * DH), w, p.out_f32);
                    }
                }
        } else if (q_ok[qi]) {
#pragma unroll
            for (int vb = 0; vb < NB; ++vb) {
                const int64_t op = (b + bank_off(vb)) * p.o_bs + f * p.o_fs + (int64_t)q_row[qi] * (H * DH) + h * DH;
#pragma unroll
                for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                    for (int rg = 0; rg < 4; ++rg) {
                        const int d0 = mt * 32 + 8 * rg + 4 * hi;
                        if (d0 < DH) {
                            f32x4 w;
#pragma unroll
                            for (int i = 0; i < 4; ++i) w[i] = o[vb][qi][mt][rg * 4 + i] * inv_l;
                            store_out4<E, vec4>(p.out, op + d0, w, p.out_f32);
                        }
                    }
            }
        }
    }
}

// Plan token: the `1` behind the head dim is the number of query tiles per wave; the token grammar is pinned by
// tests/golden/kernel_plans.json.
template <typename T, int DH, int NW, int MODE, int MINW, bool FQ = true, bool SB = false, typename P>
int launch_one(const P& p_in, hipStream_t st) {
    launch_params_t<P, MODE> p = p_in;   // the kernel's parameter block
    typedef AttnCfg<DH> C;
    constexpr size_t lds = ((MODE == MODE_DUAL && DH == 40)  ? 2 * (size_t)(C::K_ELEMS + 96 * C::VROW) * 2    // PACK
                            : (MODE == MODE_MV4 && DH == 40) ? 2 * (size_t)(C::K_ELEMS + 192 * C::VROW) * 2   // PACK, four banks
                                                             : C::lds_bytes(MODE == MODE_DUAL ? 2 : MODE == MODE_MV4 ? 4 : 1)) / (SB ? 2 : 1);
    if (tf_plan_note("one<%d,1,%d,%s,%d,fq%d%s%s>%s", DH, NW, mode_name(MODE), MINW, FQ ? 1 : 0, SB ? ",sb" : "", run_mark<MODE>(p),
                     table_mark<decltype(p)>()))
        return 0;
    auto kern = ext_attn_kernel<T, DH, 1, NW, MODE, MINW, 64, FQ, SB, decltype(p)>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    p.nQT = (p.S + 32 * NW - 1) / (32 * NW);
    const int per_branch = p.Kq * p.nQT * p.H;
    // bank problems are decoded first: a bank-only launch simply stops before the source problems
    const int ns = MODE == MODE_SOURCE ? 1 : p.nseg;
    const unsigned grid = (unsigned)(MODE == MODE_ALL ? (2 * ns + (p.part == TF_ATTN_BANK_ONLY ? 0 : 1)) * per_branch
                                                      : ns * per_branch);
    // Run launches: the one staging site inside the loop is `if (has_next) stage_load()`, has_next = tile + 1 < ntiles, and the
    // prologue loads tile 0; rows past S of a short last tile are clamped to the frame's last key.  No fetch passes the run's
    // last tile, in the caller's k or in the V^T image.
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), lds, st, p);
    TF_LAUNCH_CHECK("tf_ext_attn_fwd");
    return 0;
}

}  // namespace
