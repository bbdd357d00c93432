// Extended attention, the half-tile interleaved streaming kernel (register-staged or LDS-DMA tiles, optional mixed MFMA
// shapes).  Included by ext_attn.hip only.
#pragma once

#include "attn_common.h"

namespace {

// Half-tile interleaved variant (fp32 score scaling): Dh = 40 (the cfg2 / cfg3 level-0 form) and 80.
//
// The plain kernel runs QK^T -> softmax (64 VALU) -> P.V of one 64-key tile back to back: inside a wave the matrix
// pipe idles during the softmax and the VALU during the MFMAs, and the overlap that independent waves on a SIMD
// provide stops at ~49 % matrix-pipe utilisation at Dh = 40 -- and does not exist at all where the
// registers of the larger head dims leave two waves per SIMD.
// Here ONE query tile per wave is software-pipelined over 32-key half tiles, so that every stretch of the
// instruction stream has INDEPENDENT matrix and vector work, issued alternately (one MFMA, its share of the softmax,
// pinned by sched_barrier(0)):
//     phase 1 of tile t:  O += V0(t) P0(t)  and  S0(t+1) = K0(t+1) Q   (2 MT + KS MFMAs)  ||  P1(t)   = exp2(S1(t) c - m c)
//     phase 2 of tile t:  O += V1(t) P1(t)  and  S1(t+1) = K1(t+1) Q                       ||  P0(t+1) = exp2(S0(t+1) c - m c)
// (7 MFMAs per phase at Dh = 40, 11 at 80, against the same 8 softmax units of 2 fma + 2 exp + 1 cvt.)
// Same LDS images as the plain kernel, K staged one tile earlier (as in the ping-pong kernel): top of iteration t
// writes K(t+1) and V(t) from registers loaded an iteration before, one barrier, then the two phases.
// Online softmax: Dh = 40 uses the score bound (BOUND: a half tile looks at its maximum only when the bound does not
// exclude an overflow); the other head dims take the half tile's maximum every time (they are matrix-bound).  When
// the shift moves, O -- which by then includes the P.V of the half tile that ran beside the softmax, computed against
// the OLD shift -- is rescaled at the END of the phase, before any P at the new shift is multiplied in
// (cdna_hip_programming.md T13: scale everything still at the old maximum exactly once).
// Scope: S a multiple of 64, MODE_ALL / MODE_SOURCE problems (the dual-V form has its own kernel); the split form
// of small grids (runs of bank frames + attn_merge_kernel) as in ext_attn_kernel.
template <int MT, int KS, bool NEXT>
struct IlSchedule {   // MFMA order of one phase: QK^T k-steps (one accumulator chain) alternate with the P.V MFMAs
    static constexpr int N = (NEXT ? KS : 0) + 2 * MT;   // (M-tile round-robin, 2 k-steps): never two MFMAs on one
    int is_pv[N] = {}, a[N] = {}, b[N] = {};              // accumulator next to each other
    constexpr IlSchedule() {
        int i = 0, qk = 0, pv = 0;
        while (i < N) {
            if (NEXT && qk < KS) {
                is_pv[i] = 0, a[i] = qk, b[i] = 0;
                ++qk, ++i;
            }
            if (pv < 2 * MT) {
                is_pv[i] = 1, a[i] = pv % MT, b[i] = pv / MT;   // a = M-tile, b = 16-key k-step of the half
                ++pv, ++i;
            }
        }
    }
};

// MIXED MFMA shapes (Dh = 40, one bank, round 6): QK^T stays 32x32x16 (K = 48), P.V runs as 16x16x32 MFMAs over
// THREE 16-row M-tiles (rows 0-47 of the same V^T image: 40 features, the ones row, 7 zero rows) and the two 16-query halves
// of the wave's tile: 6 short MFMAs (16 clocks each) per 32-key half instead of 4 long ones -- 192 instead of 224 matrix-pipe
// clocks per phase.  A step's fragment is read once per M-tile (fidx: the step whose LDS fragment this step multiplies).
template <int NT, int KS, bool NEXT>
struct IlScheduleMix {   // NT = 16-row M-tiles of P.V (3 at Dh = 40: 48 rows; 4 at Dh = 64)
    static constexpr int N = (NEXT ? KS : 0) + 2 * NT;
    int is_pv[N] = {}, a[N] = {}, b[N] = {}, fidx[N] = {};   // P.V: a = M-tile, b = 16-query half; QK^T: a = k-step
    constexpr IlScheduleMix() {
        int i = 0;
        if (NEXT) {
            // QK0 PV00 PV01 | QK1 PV10 PV11 | QK2 PV20 PV21 ...: the QK^T chain's links lie two short MFMAs (32 clocks) apart
            for (int d = 0; d < NT; ++d) {
                if (d < KS) {
                    is_pv[i] = 0, a[i] = d, fidx[i] = i;
                    ++i;
                }
                is_pv[i] = 1, a[i] = d, b[i] = 0, fidx[i] = i;
                is_pv[i + 1] = 1, a[i + 1] = d, b[i + 1] = 1, fidx[i + 1] = i;
                i += 2;
            }
            for (int t = NT; t < KS; ++t) {
                is_pv[i] = 0, a[i] = t, fidx[i] = i;
                ++i;
            }
        } else {
            // PV00 PV10 PV01 PV11 | PV20 PV21 | PV30 PV31: the first two steps own their fragments (cross-phase prefetch hands over two)
            const int dd[4] = {0, 1, 0, 1}, tt[4] = {0, 0, 1, 1}, ff[4] = {0, 1, 0, 1};
            for (i = 0; i < 4; ++i) is_pv[i] = 1, a[i] = dd[i], b[i] = tt[i], fidx[i] = ff[i];
            for (int d = 2; d < NT; ++d) {
                is_pv[i] = 1, a[i] = d, b[i] = 0, fidx[i] = i;
                is_pv[i + 1] = 1, a[i + 1] = d, b[i + 1] = 1, fidx[i + 1] = i;
                i += 2;
            }
        }
    }
};

// DMA != 0 (non-PACK forms): K and V^T tiles go global -> LDS by `global_load_lds_dwordx4` instead of through registers: no
// staging VGPRs, no ds_write pass.  The DMA writes lane-linearly (wave-uniform LDS base + lane * 16 B per instruction, a
// "piece" of 1 KB), the per-lane SOURCE address is free, so any LDS image whose 16-B slots are filled piece by piece works.
//   DMA = 2 (round 6): the PADDED images of the register-staged form (row strides of an odd number of 16-B slots), so every
//           fragment address stays "per-lane base + immediate".  A lane whose slot is row padding fetches slot 0 of its row
//           (finite data: the K pad columns meet zero columns of Q, the V^T pad columns are never read); the lanes of a last,
//           partial piece past the end of the image are masked off (the constant rows behind it must survive).
//   DMA = 3: the same staging with the mixed MFMA shapes above.
//   (DMA = 1, round 5's dense XOR-swizzled images, cost an address computation per fragment read and measured 0.5 % slower
//   than register staging, profiles/r05_attn_il40_dma_ab.txt: gone.)
// A tile is issued right behind the barrier that frees its buffer and drained (vmcnt(0)) in front of the next one: the same
// distance the register staging had.
template <typename T, int DH, int NW, int MODE, int MINW, int DMA = 0, typename P = AttnParams>
__global__ __launch_bounds__(64 * NW, MINW) void ext_attn_il_kernel(P p) {
    typedef AttnCfg<DH> C;
    typedef typename T::elem E;
    typedef typename T::vec8 vec8;
    typedef typename T::vec4 vec4;
    constexpr int NT = 64 * NW;
    // MODE_DUAL (q/k injection, Dh = 40): uncond and cond share q, k, the scores and P; the two banks' V^T rows are
    // packed into ONE LDS image of 3 M-tiles (rows 0-39 uncond, 40-79 cond, row 80 the common ones row) exactly as in
    // ext_attn_kernel's PACK form, so the only differences to the single-bank kernel are the number of staged V^T rows
    // (VR), the number of P.V M-tiles (MT) and the epilogue's row -> (bank, feature) decode.
    constexpr bool PACK = MODE == MODE_DUAL;
    static_assert(DMA == 0 || DMA == 2 || DMA == 3, "register staging, LDS-DMA, or LDS-DMA with mixed MFMA shapes");
    constexpr bool MIX = DMA == 3;   // DMA = 3: the DMA = 2 staging + mixed MFMA shapes, see IlScheduleMix
    static_assert(!MIX ||((DH == 40 || DH == 64) && !PACK), "mixed MFMA shapes: Dh = 40 or 64, one bank");
    constexpr int NT16 = DH == 40 ? 3 : (DH + 15) / 16;   // MIX: 16-row M-tiles of P.V (Dh = 40: features + the ones row + 7 zero rows)
    static_assert(!PACK || DH == 40 || DH == 64 || DH == 80,
                  "the packed dual-V image: Dh = 40 (3 M-tiles, ones row 80), Dh = 64 (4 full M-tiles) or Dh = 80 (5 full M-tiles)");
    constexpr int VR = PACK ? 2 * DH : DH;              // staged V^T rows per tile
    constexpr int MT = PACK ? (2 * DH + 31) / 32 : C::MT;   // P.V M-tiles
    constexpr int KROW = C::KROW, VROW = C::VROW;       // LDS row strides (elements)
    constexpr int K_ELEMS = 64 * KROW;
    constexpr int V_ELEMS = MT * 32 * VROW;
    constexpr int NPK = C::npk(NT), NPV = (VR * 8 + NT - 1) / NT;
    constexpr int BUF_ELEMS = K_ELEMS + V_ELEMS;
    constexpr bool ONES = (VR % 32) != 0;   // denominator from the MFMA (row VR of the V^T image = 1.0)
    constexpr int ONES_R = ((VR % 32) & 3) + 4 * ((VR % 32) >> 3);
    static_assert(!ONES || ((VR % 32) & 4) == 0, "the ones row must live in lane half 0");
    constexpr bool BOUND = attn_has_bound(DH);   // needs the key norms of the pre-pass
    constexpr float BOUND_T = std::is_same<E, _Float16>::value ? 14.0f : 60.0f;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    auto sK = [&](int buf) { return reinterpret_cast<E*>(smem) + buf * BUF_ELEMS; };
    auto sV = [&](int buf) { return reinterpret_cast<E*>(smem) + buf * BUF_ELEMS + K_ELEMS; };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hi = lane >> 5;
    const int l31 = lane & 31;
    const int K = p.K, Kq = p.Kq, S = p.S, H = p.H;

    const int h = blockIdx.x % H;
    int u = blockIdx.x / H;
    int b, f, qt;
    int seg = 0;   // split form (small grids): run of bank frames this workgroup covers, see ext_attn_kernel
    const int nseg = MODE == MODE_SOURCE ? 1 : p.nseg;
    if constexpr (MODE == MODE_ALL) {
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
    } else if constexpr (MODE == MODE_DUAL) {
        b = 1;
        seg = u % nseg;
        u /= nseg;
    } else {
        b = 0;
    }
    f = u / p.nQT;
    qt = u - f * p.nQT;
    const int bq = (p.inject && b > 0) ? 0 : b;
    const bool split = p.pslots > 0 && b > 0;
    int f_lo = b == 0 ? p.q_frame0 + f : (seg * K) / nseg;
    int n_fr = b == 0 ? 1 : ((seg + 1) * K) / nseg - f_lo;
    if constexpr (is_win<P>) {   // a bank problem reads its query frame's window of the bank
        if (b > 0) window_range(p, f, seg, nseg, f_lo, n_fr);
        if (n_fr == 0) {   // a window shorter than the split: this run holds no frame
            write_empty_run(p, b - 1, PACK ? 2 : 1, f, h, seg, qt * (32 * NW), 32 * NW, DH, NT);
            return;
        }
    }
    [[maybe_unused]] uint64_t run = 0;   // frame-set launches: the member frames of this problem (see set_run, SetWalk)
    if constexpr (is_set<P>) {   // a bank problem reads the member frames of its query frame's set, in ascending order
        run = (uint64_t)1 << f_lo;   // (a source problem: its own frame)
        if (b > 0) {
            run = set_run(p, f, seg, nseg, n_fr);
            if (n_fr == 0) {   // a set shorter than the split: this run holds no member
                write_empty_run(p, b - 1, PACK ? 2 : 1, f, h, seg, qt * (32 * NW), 32 * NW, DH, NT);
                return;
            }
            f_lo = __builtin_ctzll(run);
        }
    }
    const int tpf = S >> 6;
    const int ntiles = n_fr * tpf;

    const E* qg = reinterpret_cast<const E*>(p.q);
    const E* kg = reinterpret_cast<const E*>(p.k) + bq * p.k_bs + h * DH;
    const int64_t vt_row = vt_row_stride(p.Kb, p.Spad);
    const E* vg = reinterpret_cast<const E*>(p.vt) + ((int64_t)(b * H + h) * DH) * vt_row;

    // ---- LDS init: zero everything (pads; the V^T rows past DH), then the denominator row DH of both V^T images
    for (int id = tid; id < 2 * BUF_ELEMS / 8; id += NT) st16(reinterpret_cast<E*>(smem) + id * 8, u32x4{0, 0, 0, 0});
    __syncthreads();
    if constexpr (ONES)
        for (int id = tid; id < 2 * 64; id += NT) sV(id >> 6)[VR * VROW + (id & 63)] = (E)1.f;

    // ---- Q fragments
    const int q_row = qt * (32 * NW) + wave * 32 + l31;
    const bool q_ok = q_row < S;
    vec8 qf[C::KS];
    {
        const E* qp = qg + bq * p.q_bs + f * p.q_fs + (int64_t)(q_ok ? q_row : S - 1) * p.ld_q + h * DH;
#pragma unroll
        for (int t = 0; t < C::KS; ++t) {
            const int col = 16 * t + 8 * hi;
            qf[t] = __builtin_bit_cast(vec8, col < DH ? ld16(qp + col) : u32x4{0, 0, 0, 0});
        }
    }
    const float c = p.c;
    // score bound (log2 units) over every key this problem sees: |q| max|k| c  (see BOUND in ext_attn_kernel)
    float s_bound = 0.f;
    if constexpr (BOUND) {
        const int ppf = p.Spad / 64;
        const float* part = p.knorm2 + ((int64_t)(bq * H + h) * p.Kb + f_lo) * ppf;
        float kn2 = 0.f;
        if constexpr (is_set<P>) kn2 = set_knorm2(part - (int64_t)f_lo * ppf, run, ppf, lane);   // the member frames' blocks only
        else
            for (int i = lane; i < n_fr * ppf; i += 64) kn2 = fmaxf(kn2, part[i]);
#pragma unroll
        for (int o_ = 32; o_ > 0; o_ >>= 1) kn2 = fmaxf(kn2, __shfl_xor(kn2, o_));
        float q2 = 0.f;
#pragma unroll
        for (int t = 0; t < C::KS; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j) q2 = fmaf((float)qf[t][j], (float)qf[t][j], q2);
        q2 += __shfl_xor(q2, 32);
        s_bound = __builtin_sqrtf(q2) * __builtin_sqrtf(kn2) * 1.001f * c;
    }

    // ---- staging: 16-B pieces of K and of V^T per thread and tile (branch-free, see ext_attn_kernel)
    u32x4 rk[NPK], rv[NPV];
    int k_goff[NPK], k_loff[NPK], v_goff[NPV], v_loff[NPV];
#pragma unroll
    for (int i = 0; i < NPK; ++i) {
        const int id = min(tid + NT * i, 64 * C::PPR - 1);
        k_goff[i] = (id / C::PPR) * (int)p.ld + (id % C::PPR) * 8;
        k_loff[i] = (id / C::PPR) * KROW + (id % C::PPR) * 8;
    }
#pragma unroll
    for (int i = 0; i < NPV; ++i) {
        const int id = min(tid + NT * i, VR * 8 - 1);
        const int row = id >> 3;   // image row: bank row / DH (the next branch's rows lie H*DH image rows further), feature row % DH
        v_goff[i] = ((row / DH) * H * DH + row % DH) * (int)vt_row + (id & 7) * 8;
        v_loff[i] = row * VROW + (id & 7) * 8;
    }
    const int v_wrap = p.Spad - (tpf - 1) * 64;
    const int64_t k_wrap_off = p.k_fs - (int64_t)(tpf - 1) * 64 * p.ld;
    const E* k_next = kg + f_lo * p.k_fs;
    const E* v_next = vg + (int64_t)f_lo * p.Spad;
    int k_tt = 0, v_tt = 0;
    [[maybe_unused]] SetWalk k_walk{}, v_walk{};   // frame-set launches: the member frame each cursor stands in
    if constexpr (is_set<P>) k_walk.init(run), v_walk.init(run);
    // (a frame boundary of a frame-set launch, below: on to the next member frame, over the frames between it and this one)
    auto load_k = [&]() {
#pragma unroll
        for (int i = 0; i < NPK; ++i) rk[i] = ld16(k_next + k_goff[i]);
        const bool wrap = k_tt == tpf - 1;
        k_next += wrap ? k_wrap_off : (int64_t)64 * p.ld;
        if constexpr (is_set<P>) {
            if (wrap) k_next += (int64_t)k_walk.hop() * p.k_fs;
        }
        k_tt = wrap ? 0 : k_tt + 1;
    };
    auto load_v = [&]() {
#pragma unroll
        for (int i = 0; i < NPV; ++i) rv[i] = ld16(v_next + v_goff[i]);
        const bool wrap = v_tt == tpf - 1;
        v_next += wrap ? v_wrap : 64;
        if constexpr (is_set<P>) {
            if (wrap) v_next += (int64_t)v_walk.hop() * p.Spad;
        }
        v_tt = wrap ? 0 : v_tt + 1;
    };
    auto write_k = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NPK; ++i)
            if (tid + NT * i < 64 * C::PPR) st16(sK(buf) + k_loff[i], rk[i]);
    };
    auto write_v = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NPV; ++i)
            if (tid + NT * i < VR * 8) st16(sV(buf) + v_loff[i], rv[i]);
    };
    // DMA forms: a tile = NKP 1-KB pieces of the K image + NVP of the V^T image; wave w issues pieces w, w + NW, .. of each.
    // Per-lane source offsets are unsigned BYTE offsets from the wave-uniform tile pointers, so that the DMA takes the
    // SGPR-base + 32-bit-VGPR-offset form (no 64-bit address pair per lane)
    constexpr int K_IMG = 64 * KROW * 2, V_IMG = VR * VROW * 2;   // staged bytes of one K / V^T image
    constexpr int NKP = DMA ? (K_IMG + 1023) / 1024 : 0, NVP = DMA ? (V_IMG + 1023) / 1024 : 0;
    constexpr int NKS = DMA ? (NKP + NW - 1) / NW : 1, NVS = DMA ? (NVP + NW - 1) / NW : 1;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* glb_ptr;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    uint32_t dk_goff[NKS], dv_goff[NVS];
    bool dk_ok[NKS], dv_ok[NVS];   // this lane's slot lies inside the image (false only in a last, partial piece)
    if constexpr (DMA != 0) {
#pragma unroll
        for (int n = 0; n < NKS; ++n) {
            const int o = (wave_u + NW * n) * 1024 + lane * 16;
            const int row = min(o / (2 * KROW), 63);
            const int pc = (o - row * 2 * KROW) >> 4;          // 16-B slot of the LDS row this lane fills
            dk_ok[n] = o < K_IMG;
            dk_goff[n] = (uint32_t)(row * (int)p.ld + ((pc < DH / 8 ? pc : 0) << 3)) * 2u;
        }
#pragma unroll
        for (int n = 0; n < NVS; ++n) {
            const int o = (wave_u + NW * n) * 1024 + lane * 16;
            const int row = min(o / (2 * VROW), VR - 1);
            const int sl = (o - row * 2 * VROW) >> 4;
            dv_ok[n] = o < V_IMG;
            // image row -> V^T row: bank row / DH (the next branch's rows lie H*DH V^T rows further), feature row % DH
            const int vrow = PACK ? (row / DH) * H * DH + row % DH : row;
            // (MIX: the mixed form's V^T reads have 2-way bank conflicts; a slot swizzle that removes them measured 1 % slower,
            // profiles/r06_attn_d40_mix_ab.txt section 8: the LDS is not what this kernel waits for)
            dv_goff[n] = (uint32_t)(vrow * (int)vt_row + ((sl < 8 ? sl : 0) << 3)) * 2u;
        }
    }
    auto dma_k = [&](int buf) {      // the next K tile -> Kbuf[buf]
#pragma unroll
        for (int n = 0; n < NKS; ++n) {
            const int q = wave_u + NW * n;
            if (NKP % NW == 0 || q < NKP) {
                uint32_t off = dk_goff[n];
                asm volatile("" : "+v"(off));   // keeps the zero-extension next to the add: SGPR base + 32-bit VGPR offset form
                if (K_IMG % 1024 == 0 || dk_ok[n])
                    __builtin_amdgcn_global_load_lds((glb_ptr)(reinterpret_cast<const char*>(k_next) + off),
                                                     (lds_ptr)(sK(buf) + q * 512), 16, 0, 0);
            }
        }
        const bool wrap = k_tt == tpf - 1;
        k_next += wrap ? k_wrap_off : (int64_t)64 * p.ld;
        if constexpr (is_set<P>) {
            if (wrap) k_next += (int64_t)k_walk.hop() * p.k_fs;
        }
        k_tt = wrap ? 0 : k_tt + 1;
    };
    auto dma_v = [&](int buf) {      // the next V^T tile -> Vbuf[buf]
#pragma unroll
        for (int n = 0; n < NVS; ++n) {
            const int q = wave_u + NW * n;
            if (NVP % NW == 0 || q < NVP) {
                uint32_t off = dv_goff[n];
                asm volatile("" : "+v"(off));
                if (V_IMG % 1024 == 0 || dv_ok[n])
                    __builtin_amdgcn_global_load_lds((glb_ptr)(reinterpret_cast<const char*>(v_next) + off),
                                                     (lds_ptr)(sV(buf) + q * 512), 16, 0, 0);
            }
        }
        const bool wrap = v_tt == tpf - 1;
        v_next += wrap ? v_wrap : 64;
        if constexpr (is_set<P>) {
            if (wrap) v_next += (int64_t)v_walk.hop() * p.Spad;
        }
        v_tt = wrap ? 0 : v_tt + 1;
    };
    auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

    f32x16 o[MT], s[2];
    f32x4 o16[NT16][2]; // MIX: O^T as [16-row M-tile][16-query half]: lane l = query l & 15 of the half, rows 4 (l >> 4) + i
    vec8 pf[2][2];      // P of the two 32-key halves, two 16-key k-steps each (MIX: after p_relayout, the two 16-query halves)
    float m_run = -INFINITY;   // BOUND: deferred shift; else the lagged running maximum (raw-score units)
    const float lag = TF_ATTN_LAG / c;   // raw-score units
    // !ONES (Dh = 64: both P.V M-tiles are full, no spare row for the denominator): the row sum on the MATRIX pipe.  The 32 v_add of
    // a tile were 2.0 of the loop's 7.8 VALU instructions per MFMA, on an issue port that is the kernel's limiter
    // (profiles/r06_d64_accounting.md); v_mfma_f32_4x4x4 with A = ones adds the 4 rounded P values of a lane's register pair
    // to a lane-local fp32 sum -- 8 short MFMAs (8 clocks of the pipe each) per tile, and the denominator sums exactly the
    // rounded P the numerator multiplies.
    constexpr bool LSUM_MFMA = !ONES;
    f32x4 lacc = {0.f, 0.f, 0.f, 0.f};
    vec4 ones4;
#pragma unroll
    for (int j = 0; j < 4; ++j) ones4[j] = (E)1.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[mt][r] = 0.f;
#pragma unroll
    for (int d = 0; d < NT16; ++d)
#pragma unroll
        for (int t = 0; t < 2; ++t) o16[d][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[kt][ks][j] = (E)0.f;
    // MIX: P of half X from the 32x32 accumulator layout (lane = query l & 31; pf[X][0] = accumulator registers 0-7, pf[X][1] =
    // 8-15) to the 16x16x32 B layout (lane = query l & 15 of a 16-query half, 8 keys per 16-lane row).  v_permlane16_swap
    // exchanges the odd 16-lane rows of its first operand with the even rows of its second: afterwards pf[X][0] holds, in
    // rows 0 / 1 / 2 / 3, registers 0-7 | 8-15 of lane half 0 and 0-7 | 8-15 of lane half 1 of queries 0-15, pf[X][1] the same of
    // queries 16-31 -- the k order (row g: accumulator registers 8 (g & 1) .. +7 of lane half g >> 1) is the one the V^T
    // fragment read of the mixed form uses.
    auto p_relayout = [&](auto x_c) {
        constexpr int X = decltype(x_c)::value;
        u32x4 a = __builtin_bit_cast(u32x4, pf[X][0]), b2 = __builtin_bit_cast(u32x4, pf[X][1]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const auto r = __builtin_amdgcn_permlane16_swap(a[i], b2[i], false, false);
            a[i] = r[0];
            b2[i] = r[1];
        }
        pf[X][0] = __builtin_bit_cast(vec8, a);
        pf[X][1] = __builtin_bit_cast(vec8, b2);
    };
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    // decision part of the online softmax of half X: returns alpha (1 = no move) and leaves m_run updated
    auto sm_decide = [&](auto x_c, bool& move) -> float {
        constexpr int X = decltype(x_c)::value;
        move = false;
        float alpha = 1.f;
        auto half_max = [&]() {
            float mx = s[X][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[X][r]);
            return max_with_lane_xor32(mx);
        };
        if constexpr (BOUND) {
            if (__any(s_bound - m_run * c > BOUND_T)) {
                const float mx = half_max();
                const bool over = (mx - m_run) * c > BOUND_T;
                if (__any(over)) {
                    move = true;
                    const float m_new = over ? mx : m_run;
                    alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);   // exp2(-inf) = 0 on the first half tile (O is 0)
                    m_run = m_new;
                }
            }
        } else {
            // m_run = the query's reference point: it follows the running maximum with a lag of TF_ATTN_LAG binades (P <= 2^8,
            // in range for f16 too).  With the exact maximum a wave of 32 queries rescaled O on ~40 % of its half tiles
            // (some query almost always sees a new maximum); per-query decision: alpha = 1 exactly where it did not move.
            const float mx = half_max();
            const bool over = mx > m_run + lag;   // -inf + lag = -inf: the first half tile always sets the reference
            if (__any(over)) {
                move = true;
                const float m_new = over ? mx : m_run;
                alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
                m_run = m_new;
            }
        }
        return alpha;
    };
    auto rescale = [&](float alpha) {
        if constexpr (MIX) {
            // alpha belongs to query l & 31; O^T holds queries l & 15 (half 0) and 16 + (l & 15) (half 1): one row swap delivers both
            const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(alpha), __float_as_uint(alpha), false, false);
            const float a0 = __uint_as_float(r[0]), a1 = __uint_as_float(r[1]);
#pragma unroll
            for (int d = 0; d < NT16; ++d) {
                o16[d][0] *= a0;
                o16[d][1] *= a1;
            }
            return;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[mt][r] *= alpha;
    };
    // one softmax unit: two scores of half X -> P (8 units per half).  Beside MFMAs hipcc emits most of these
    // multiply-adds as two scalar v_fma instead of one v_pk_fma_f32 -- rightly: forcing the packed form (inline asm)
    // measured +8 % (4.30 vs 3.97 ms), the packed f32 VALU delays the MFMAs issued around it.
    auto sm_unit = [&](auto x_c, int un, f32x2 c2, f32x2 mc2) {
        constexpr int X = decltype(x_c)::value;
        const int r = un * 2;
        const f32x2 x = f32x2{s[X][r], s[X][r + 1]} * c2 - mc2;
        const float p0 = __builtin_amdgcn_exp2f(x[0]), p1 = __builtin_amdgcn_exp2f(x[1]);
        if constexpr (LSUM_MFMA) {
            // the register pair (4 values of P) completed by the PREVIOUS two units goes onto the lane's running sum: one unit
            // late, so that the conversion that wrote the pair is not the instruction in front of the MFMA that reads it
            // (VALU write -> MFMA read wait states); the last pair of a half is added behind the phase's last step
            if (un >= 2 && !(un & 1)) {
                const vec8 v = pf[X][(un - 2) >> 2];
                lacc = T::mfma4(ones4, ((un - 2) & 2) ? v.hi : v.lo, lacc);
            }
        }
        pf[X][r >> 3][r & 7] = (E)p0;
        pf[X][r >> 3][(r & 7) + 1] = (E)p1;
    };

    // One phase: the MFMAs of P.V half Hh of the current tile (V^T buffer vbuf) and -- NEXT -- of QK^T half Hh of the
    // next tile (K buffer kbuf), interleaved in program order with the softmax of half 1 - Hh (SM: there is one).
    constexpr int PF = 2;   // fragment reads run PF steps ahead of their MFMA (register-staged Dh = 40 with 3: 132 VGPRs)
    // LDS fragment i of the MFMA sequence of phase (Hh, NEXT): a P.V fragment of V^T buffer vbuf or a QK^T fragment of K buffer kbuf
    auto frag = [&](auto h_c, auto next_c, int i, int vbuf, int kbuf) -> vec8 {
        constexpr int Hh = decltype(h_c)::value;
        if constexpr (MIX) {
            constexpr IlScheduleMix<NT16, C::KS, decltype(next_c)::value> schm{};
            if (schm.is_pv[i])   // 16 rows x 32 keys of M-tile a: lane row g reads the image columns of k-step g & 1, lane half g >> 1
                return __builtin_bit_cast(vec8, ld16(sV(vbuf) + (schm.a[i] * 16 + (lane & 15)) * VROW + Hh * 32 +
                                                     16 * ((lane >> 4) & 1) + 8 * hi));
            return __builtin_bit_cast(vec8, ld16(sK(kbuf) + (Hh * 32 + l31) * KROW + 8 * hi + 16 * schm.a[i]));
        }
        constexpr IlSchedule<MT, C::KS, decltype(next_c)::value> sch{};
        if (sch.is_pv[i]) {
            const E* vbase = sV(vbuf) + l31 * VROW + Hh * 32 + 8 * hi;
            return __builtin_bit_cast(vec8, ld16(vbase + sch.a[i] * 32 * VROW + 16 * sch.b[i]));
        }
        return __builtin_bit_cast(vec8, ld16(sK(kbuf) + (Hh * 32 + l31) * KROW + 8 * hi + 16 * sch.a[i]));
    };
    // XPF (cross-phase prefetch): the first PF fragments of a phase that follows another one WITHOUT a barrier between them
    // (the second phase of a tile: same buffers) are read during the last steps of its predecessor and handed over in
    // fr_carry -- a phase otherwise opens with PF reads and a full LDS round trip in front of its first MFMA.
    vec8 fr_carry[PF];
    auto phase = [&](auto h_c, auto next_c, auto sm_c, auto pre_in_c, auto pre_out_c, int vbuf, int kbuf) {
        constexpr int Hh = decltype(h_c)::value;
        constexpr int X = 1 - Hh;
        constexpr bool NEXT = decltype(next_c)::value, SM = decltype(sm_c)::value;
        constexpr bool PRE_IN = decltype(pre_in_c)::value;     // fragments 0 .. PF-1 arrive in fr_carry
        constexpr bool PRE_OUT = decltype(pre_out_c)::value;   // the following phase (half 1 - Hh, same NEXT, same buffers) gets its first PF
        constexpr std::conditional_t<MIX, IlScheduleMix<NT16, C::KS, NEXT>, IlSchedule<MT, C::KS, NEXT>> sch{};
        constexpr int NM = sch.N;
        static_assert(PF <= NM, "prefetch distance beyond one phase");
        bool move = false;
        float alpha = 1.f;
        f32x2 c2 = {c, c}, mc2 = {0.f, 0.f};
        if constexpr (SM) {
            alpha = sm_decide(std::integral_constant<int, X>{}, move);
            const float mc = m_run * c;
            mc2 = f32x2{mc, mc};
            // the matrix-pipe denominator holds sums at the OLD shift only (every earlier half tile, the other half of this tile
            // included) and takes this phase's P -- at the NEW shift -- as the phase goes: rescale it NOW, before the first of
            // them is added.  (O is rescaled at the END of the phase: its P.V of this phase still multiplies P at the old shift.)
            if constexpr (LSUM_MFMA)
                if (move) lacc *= alpha;
        }
        vec8 fr[NM];
#pragma unroll
        for (int i = 0; i < PF; ++i) fr[i] = PRE_IN ? fr_carry[i] : frag(h_c, next_c, i, vbuf, kbuf);
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            if constexpr (MIX) {
                // a step reads its own fragment only (fidx == i); the first PF steps of every mixed schedule own theirs
                if (i + PF < NM) {
                    if (sch.fidx[i + PF] == i + PF) fr[i + PF] = frag(h_c, next_c, i + PF, vbuf, kbuf);
                } else if constexpr (PRE_OUT) {
                    fr_carry[i + PF - NM] = frag(std::integral_constant<int, X>{}, next_c, i + PF - NM, vbuf, kbuf);
                }
            } else {
                if (i + PF < NM) fr[i + PF] = frag(h_c, next_c, i + PF, vbuf, kbuf);
                else if constexpr (PRE_OUT) fr_carry[i + PF - NM] = frag(std::integral_constant<int, X>{}, next_c, i + PF - NM, vbuf, kbuf);
            }
            if constexpr (MIX) {
                if (sch.is_pv[i])
                    o16[sch.a[i]][sch.b[i]] = T::mfma16(fr[sch.fidx[i]], pf[Hh][sch.b[i]], o16[sch.a[i]][sch.b[i]]);
                else
                    s[Hh] = T::mfma32(fr[i], qf[sch.a[i]], sch.a[i] == 0 ? zero : s[Hh]);
            } else if (sch.is_pv[i]) {
                o[sch.a[i]] = T::mfma32(fr[i], pf[Hh][sch.b[i]], o[sch.a[i]]);
            } else {
                s[Hh] = T::mfma32(fr[i], qf[sch.a[i]], sch.a[i] == 0 ? zero : s[Hh]);
            }
            if constexpr (SM) {
#pragma unroll
                for (int un = (i * 8) / NM; un < ((i + 1) * 8) / NM; ++un)
                    sm_unit(std::integral_constant<int, X>{}, un, c2, mc2);
            }
            // The non-mixed forms pin every step (1 MFMA : its share of the softmax): without the pins they lose 1-2 % at every head
            // dim (profiles/r06_attn_d40_mix_ab.txt, nosb rows).  The mixed form is faster when hipcc places the softmax itself
            // (it moves the six short P.V MFMAs to the front of the phase, beside the multiply-adds, and the exponentials beside the
            // three long QK^T MFMAs): 3.53 against 3.63 ms pinned, 3.65 the non-mixed kernel.
            if constexpr (!MIX) __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (SM) {
            // P of half X must exist HERE (keeps the register-only softmax from sinking towards its consumer)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) asm volatile("" : "+v"(pf[X][ks]));
            if constexpr (LSUM_MFMA) lacc = T::mfma4(ones4, pf[X][1].hi, lacc);   // the last pair of the half (units 6, 7)
            if constexpr (MIX) {   // (behind the denominator's last pair: it sums the lane's OWN P values)
                p_relayout(std::integral_constant<int, X>{});
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) asm volatile("" : "+v"(pf[X][ks]));
            }
            // the shift moved: O (now including this phase's P.V, computed against the old shift) -- and the part of
            // the denominator accumulated so far, all of it at the old shift -- is rescaled before any P at the new
            // shift is multiplied in / added
            if (move) rescale(alpha);
        }
    };
    typedef std::integral_constant<int, 0> H0;
    typedef std::integral_constant<int, 1> H1;
    typedef std::true_type Yes;
    typedef std::false_type No;

    // ---- prologue: K(0) -> Kbuf[0]; S(0) = K(0) Q; P0(0); registers <- K(1), V(0)
    if constexpr (DMA != 0) {
        __syncthreads();        // LDS init done before the first DMA lands
        dma_k(0);               // K(0)
        dma_wait();
        __syncthreads();
    } else {
        load_k();
        __syncthreads();            // LDS init done before the first staging write
        write_k(0);
        if (ntiles > 1) load_k();   // K(1)
        load_v();                   // V(0)
        __syncthreads();
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const E* krow = sK(0) + (kt * 32 + l31) * KROW + 8 * hi;
#pragma unroll
        for (int t = 0; t < C::KS; ++t)
            s[kt] = T::mfma32(__builtin_bit_cast(vec8, ld16(krow + 16 * t)), qf[t], t == 0 ? zero : s[kt]);
    }
    {
        bool move;
        (void)sm_decide(H0{}, move);       // first half tile: sets the shift; O and l are zero, nothing to rescale
        const float mc = m_run * c;
        const f32x2 c2 = {c, c}, mc2 = {mc, mc};
#pragma unroll
        for (int un = 0; un < 8; ++un) sm_unit(H0{}, un, c2, mc2);
        if constexpr (LSUM_MFMA) lacc = T::mfma4(ones4, pf[0][1].hi, lacc);
        if constexpr (MIX) p_relayout(H0{});
    }

    // All tiles but the last: every phase also runs the QK^T half of the NEXT tile.  The last tile is peeled (no
    // branch on "is there a next tile" inside the loop: the two shapes of the body would otherwise make the
    // compiler keep two copies of the O accumulators and copy between them).
    if constexpr (DMA != 0) {
        // Kbuf[1] and Vbuf[0] hold nothing yet: K(1), V(0) may be issued at once (every wave is past the LDS init)
        if (ntiles > 1) dma_k(1);
        dma_v(0);
    }
    for (int t = 0; t + 1 < ntiles; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        if constexpr (DMA != 0) {
            dma_wait();                   // this wave's pieces of K(t+1), V(t) have landed ...
            __syncthreads();              // ... everybody's have; every wave has left iteration t-1, whose phases were the
            __builtin_amdgcn_sched_barrier(0);   // last readers of Kbuf[cur] (K(t)) and Vbuf[nxt] (V(t-1)): free to refill
            if (t + 2 < ntiles) dma_k(cur);      // K(t+2)
            dma_v(nxt);                          // V(t+1)
            phase(H0{}, Yes{}, Yes{}, No{}, Yes{}, cur, nxt);
            phase(H1{}, Yes{}, Yes{}, Yes{}, No{}, cur, nxt);
            continue;
        }
        // Kbuf[nxt] held K(t-1) (last read by QK(t-1) in iteration t-2), Vbuf[cur] held V(t-2) (last read in iteration
        // t-2): every wave has passed the barrier of iteration t-1, which follows iteration t-2 -> free to overwrite.
        write_k(nxt);                 // K(t+1)
        write_v(cur);                 // V(t)
        if (t + 2 < ntiles) load_k(); // K(t+2)
        load_v();                     // V(t+1)
        __syncthreads();              // K(t+1), V(t) visible to all waves
        __builtin_amdgcn_sched_barrier(0);
        phase(H0{}, Yes{}, Yes{}, No{}, Yes{}, cur, nxt);   // O += V0(t) P0(t), S0(t+1)   ||  P1(t)
        phase(H1{}, Yes{}, Yes{}, Yes{}, No{}, cur, nxt);   // O += V1(t) P1(t), S1(t+1)   ||  P0(t+1)
    }
    {
        const int cur = (ntiles - 1) & 1;
        if constexpr (DMA != 0) dma_wait();
        else write_v(cur);            // V(n-1)
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        phase(H0{}, No{}, Yes{}, No{}, Yes{}, cur, cur);    // O += V0 P0   ||  P1
        phase(H1{}, No{}, No{}, Yes{}, No{}, cur, cur);     // O += V1 P1
    }

    // ---- epilogue
    if constexpr (MIX) {
        // O^T[16 d + 4 g + i][16 t + (l & 15)] = o16[d][t][i], g = l >> 4; the ones row (40 = 16 * 2 + 4 * 2 + 0) is register 0 of
        // M-tile 2 in the lanes of row g = 2
        const int g = lane >> 4, n16 = lane & 15;
        float l_t[2];
        if constexpr (ONES) {
#pragma unroll
            for (int t = 0; t < 2; ++t) l_t[t] = __shfl(o16[2][t][0], 32 + n16);
        } else {   // Dh = 64: the matrix-pipe denominator of query l & 31 (both lane halves hold a part)
            const float lq = lacc[0] + __shfl_xor(lacc[0], 32);
#pragma unroll
            for (int t = 0; t < 2; ++t) l_t[t] = __shfl(lq, 16 * t + n16);
        }
        if (split) {
            constexpr int PS = DH + 8;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int qr = qt * (32 * NW) + wave * 32 + 16 * t + n16;
                if (qr < S) {
                    const int64_t R = (((int64_t)(b - 1) * Kq + f) * H + h) * S + qr;
                    float* row = p.partials + (R * p.pslots + seg) * PS;
#pragma unroll
                    for (int d = 0; d < NT16; ++d)
                        if (16 * d + 4 * g < DH) *reinterpret_cast<f32x4*>(row + 16 * d + 4 * g) = o16[d][t];
                    if (g == 0) row[DH] = l_t[t];
                }
            }
            if (hi == 0 && q_ok) {   // the shift is this lane's own query's (l & 31)
                const int64_t R = (((int64_t)(b - 1) * Kq + f) * H + h) * S + q_row;
                p.partials[(R * p.pslots + seg) * PS + DH + 1] = m_run * c;
            }
        } else {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int qr = qt * (32 * NW) + wave * 32 + 16 * t + n16;
                if (qr < S) {
                    const float inv = 1.0f / l_t[t];
                    const int64_t op = b * p.o_bs + f * p.o_fs + (int64_t)qr * (H * DH) + h * DH;
#pragma unroll
                    for (int d = 0; d < NT16; ++d)
                        if (16 * d + 4 * g < DH) store_out4<E, vec4>(p.out, op + 16 * d + 4 * g, o16[d][t] * inv, p.out_f32);
                }
            }
        }
        return;
    }
    float l_tot;
    if constexpr (ONES)
        l_tot = __shfl(o[MT - 1][ONES_R], l31);   // row VR of the V^T image is 1.0: sum of P from the MFMA
    else
        l_tot = lacc[0] + __shfl_xor(lacc[0], 32);
    const float inv_l = 1.0f / l_tot;
    if (split) {
        // split form: unnormalised O, denominator and shift (log2 domain) of this run of frames for attn_merge_kernel
        if (q_ok) {
            constexpr int PS = DH + 8;
            auto row_ptr = [&](int vb) {
                const int64_t R = (((int64_t)(b - 1 + vb) * Kq + f) * H + h) * S + q_row;
                return p.partials + (R * p.pslots + seg) * PS;
            };
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int r0 = mt * 32 + 8 * rg + 4 * hi;   // image row of this group of 4 (never straddles a bank)
                    if (r0 < VR) {
                        const int vb = r0 / DH;
                        f32x4 w;
#pragma unroll
                        for (int i = 0; i < 4; ++i) w[i] = o[mt][rg * 4 + i];
                        *reinterpret_cast<f32x4*>(row_ptr(vb) + (r0 - vb * DH)) = w;
                    }
                }
            if (hi == 0) {
#pragma unroll
                for (int vb = 0; vb < (PACK ? 2 : 1); ++vb) {
                    row_ptr(vb)[DH] = l_tot;
                    row_ptr(vb)[DH + 1] = m_run * c;
                }
            }
        }
    } else if (q_ok) {
        const int64_t op = b * p.o_bs + f * p.o_fs + (int64_t)q_row * (H * DH) + h * DH;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int r0 = mt * 32 + 8 * rg + 4 * hi;
                if (r0 < VR) {
                    const int vb = r0 / DH;
                    f32x4 w;
#pragma unroll
                    for (int i = 0; i < 4; ++i) w[i] = o[mt][rg * 4 + i] * inv_l;
                    store_out4<E, vec4>(p.out, op + vb * p.o_bs + (r0 - vb * DH), w, p.out_f32);
                }
            }
    }
}

template <typename T, int DH, int NW, int MODE, int MINW, int DMA = 0, typename P>
int launch_il(const P& p_in, hipStream_t st) {
    launch_params_t<P, MODE> p = p_in;   // the kernel's parameter block
    typedef AttnCfg<DH> C;
    constexpr size_t lds = MODE == MODE_DUAL ? 2 * (size_t)(C::K_ELEMS + ((2 * DH + 31) / 32) * 32 * C::VROW) * 2   // packed dual-V image
                                             : C::lds_bytes(1);
    if (tf_plan_note("il<%d,%d,%s,%d,%d%s>%s", DH, NW, mode_name(MODE), MINW, DMA, run_mark<MODE>(p), table_mark<decltype(p)>()))
        return 0;
    auto kern = ext_attn_il_kernel<T, DH, NW, MODE, MINW, DMA, decltype(p)>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    p.nQT = (p.S + 32 * NW - 1) / (32 * NW);
    const int per_branch = p.Kq * p.nQT * p.H;
    const unsigned grid = (unsigned)(MODE == MODE_ALL    ? (2 * p.nseg + (p.part == TF_ATTN_BANK_ONLY ? 0 : 1)) * per_branch
                                     : MODE == MODE_DUAL ? p.nseg * per_branch
                                                         : per_branch);
    // Run launches (p.K = the run's frames): a problem stages tiles 0 .. ntiles-1 of ITS frames and nothing else.  K(t+2) is
    // fetched under `t + 2 < ntiles`, K(1) under `ntiles > 1`, V(t+1) inside the loop over `t + 1 < ntiles` -- register staging
    // and LDS-DMA alike, the last tile is peeled and fetches nothing; S % 64 == 0 here, so every tile lies inside one frame of
    // the caller's k and inside the frame's Spad positions of the V^T image.  No fetch passes the run's last tile.
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), lds, st, p);
    TF_LAUNCH_CHECK("tf_ext_attn_fwd");
    return 0;
}

}  // namespace
