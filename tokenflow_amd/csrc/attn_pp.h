// Extended attention, the ping-pong streaming kernel (head dim 64, ragged frames of S >= 512): two query tiles per wave, the
// softmax of one interleaved in program order with the MFMAs of the other.  Included by ext_attn.hip only.
#pragma once

#include "attn_common.h"

namespace {

// MFMA issue order of one ping-pong region: round-robin over the independent accumulators
// (MT P.V chains over 4 k-steps, 2 QK^T chains over KS k-steps).  Two MFMAs on the SAME accumulator with
// other instructions issued between them cost ~+43 cycles (MI355X_MICROARCH.md, cycle constants), so
// consecutive steps must always hit different accumulators.
template <int MT, int KS>
struct PpSchedule {
    static constexpr int N = 4 * MT + 2 * KS;
    int is_pv[N] = {}, chain[N] = {}, kstep[N] = {};
    constexpr PpSchedule() {
        int i = 0;
        for (int r = 0; r < (KS > 4 ? KS : 4); ++r) {
            for (int mt = 0; mt < MT; ++mt)
                if (r < 4) {
                    is_pv[i] = 1;
                    chain[i] = mt;
                    kstep[i] = r;
                    ++i;
                }
            for (int kt = 0; kt < 2; ++kt)
                if (r < KS) {
                    is_pv[i] = 0;
                    chain[i] = kt;
                    kstep[i] = r;
                    ++i;
                }
        }
    }
};

// ---------------------------------------------------------------------------------------------
// Ping-pong variant (head dim 64, whose registers allow two query tiles per wave).
//
// A wave issues in order: a run of back-to-back MFMAs blocks its own VALU until the last one has
// issued, so softmax and matrix work of ONE query tile can never overlap inside a wave.  Here every
// wave owns two query tiles, streams A and B, half a tile apart:
//     R1(t):  exp/round P_A(t)   (VALU)   ||   O_B += V(t-1) P_B(t-1),  S_B(t) = K(t) Q_B     (MFMA)
//     R2(t):  exp/round P_B(t)   (VALU)   ||   O_A += V(t) P_A(t),      S_A(t+1) = K(t+1) Q_A (MFMA)
// and inside a region the instruction stream is forced (sched_group_barrier) to alternate
// 1 MFMA : ~4 VALU/TRANS : 1 LDS fragment read, i.e. the VALU work of one stream rides in the issue
// gaps of the other stream's MFMAs.  K(t) lives in Kbuf[t&1], V(t) in Vbuf[t&1]; K(t+1) and V(t) are
// written at the top of R1(t) from registers loaded one iteration earlier; ONE barrier per tile
// (between R1 and R2) orders all LDS hazards (see the per-line comments).
// Problems: every (branch, frame, head, query tile) one, bank problems first (the ALL form); fp32 score scaling; two waves
// per SIMD.  No score bound: the two query tiles per wave leave no registers for it (250 VGPRs; with the bound 256 and spills
// inside the loop: 898 against 971 TF/s at cfg4 level 0, profiles/r06_attn_d64_ab.txt).
// RUN (tf_ext_attn_run): bank problems only; the epilogue leaves the unnormalised O, the denominator and the shift in the
// run's partial-result slot (one slot: this kernel has no split form) instead of the output.  A template parameter, not a
// run-time one: the kernel sits at 250 VGPRs and the one-call instantiation must not change.
template <typename T, bool RUN = false, typename P = AttnParams>
__global__ __launch_bounds__(256, 2) void ext_attn_pp_kernel(P p) {
    constexpr int DH = 64;
    typedef AttnCfg<DH> C;
    // the kernel relies on it: no pad columns of K to keep zero, both P.V M-tiles full (no ones row: the denominator is a
    // lane-local sum of P)
    static_assert(C::DKP == DH && DH % 32 == 0, "the ping-pong kernel is written for head dim 64");
    typedef typename T::elem E;
    typedef typename T::vec8 vec8;
    typedef typename T::vec4 vec4;
    constexpr int NT = 256;
    constexpr int NPK = C::npk(NT), NPV = C::npv(NT);
    constexpr int BUF_ELEMS = C::K_ELEMS + C::V_ELEMS;
    constexpr int NMFMA = 2 * C::KS + 4 * C::MT;   // MFMAs per region: one QK^T (64 keys) + one P.V

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    auto sK = [&](int buf) { return reinterpret_cast<E*>(smem) + buf * BUF_ELEMS; };
    auto sV = [&](int buf) { return reinterpret_cast<E*>(smem) + buf * BUF_ELEMS + C::K_ELEMS; };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hi = lane >> 5;
    const int l31 = lane & 31;
    const int K = p.K, Kq = p.Kq, S = p.S, H = p.H;

    const int h = blockIdx.x % H;
    int u = blockIdx.x / H;
    int b, f, qt;
    const int nbank = 2 * Kq * p.nQT;
    if (u < nbank) {
        b = 1 + u / (Kq * p.nQT);
        u -= (b - 1) * Kq * p.nQT;
    } else {
        u -= nbank;
        b = 0;
    }
    f = u / p.nQT;
    qt = u - f * p.nQT;
    const int bq = (p.inject && b > 0) ? 0 : b;
    int f_lo = b == 0 ? p.q_frame0 + f : 0;
    int n_fr = b == 0 ? 1 : K;
    if constexpr (is_win<P>) {   // a bank problem reads its query frame's window of the bank (this kernel has no split form)
        if (b > 0) window_range(p, f, 0, 1, f_lo, n_fr);
    }
    [[maybe_unused]] uint64_t run = 0;   // frame-set launches: the member frames of this problem (see set_run, SetWalk)
    if constexpr (is_set<P>) {   // a bank problem reads the member frames of its query frame's set, in ascending order
        run = (uint64_t)1 << f_lo;   // (a source problem: its own frame)
        if (b > 0) {
            run = set_run(p, f, 0, 1, n_fr);   // (no split form: a set holds at least its own frame)
            f_lo = __builtin_ctzll(run);
        }
    }
    const int tpf = (S + 63) >> 6;
    const int ntiles = n_fr * tpf;
    const bool ragged = (S & 63) != 0;

    const E* qg = reinterpret_cast<const E*>(p.q);
    const E* kg = reinterpret_cast<const E*>(p.k) + bq * p.k_bs + h * DH;
    const int64_t vt_row = vt_row_stride(p.Kb, p.Spad);
    const E* vg = reinterpret_cast<const E*>(p.vt) + ((int64_t)(b * H + h) * DH) * vt_row;

    // ---- LDS init: everything zero (the pipeline touches Kbuf[1] / Vbuf[1] before they are staged:
    //      P_B(-1) = 0 times V must not meet NaN bits)
    for (int id = tid; id < 2 * BUF_ELEMS / 8; id += NT) st16(reinterpret_cast<E*>(smem) + id * 8, u32x4{0, 0, 0, 0});
    __syncthreads();

    // ---- Q fragments of both streams
    int q_row[2];
    bool q_ok[2];
    vec8 qf[2][C::KS];
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        q_row[qi] = qt * 256 + (wave * 2 + qi) * 32 + l31;
        q_ok[qi] = q_row[qi] < S;
        const E* qp = qg + bq * p.q_bs + f * p.q_fs + (int64_t)(q_ok[qi] ? q_row[qi] : S - 1) * p.ld_q + h * DH;
#pragma unroll
        for (int t = 0; t < C::KS; ++t) {
            const int col = 16 * t + 8 * hi;
            qf[qi][t] = __builtin_bit_cast(vec8, col < DH ? ld16(qp + col) : u32x4{0, 0, 0, 0});
        }
    }

    // ---- staging registers: rk = K(t+1), rv = V(t) while iteration t starts
    // (loads branch-free for the reason given in ext_attn_kernel)
    u32x4 rk[NPK], rv[NPV];
    int k_row[NPK], k_col[NPK], k_goff[NPK], k_loff[NPK], v_goff[NPV], v_loff[NPV];
#pragma unroll
    for (int i = 0; i < NPK; ++i) {
        const int id = min(tid + NT * i, 64 * C::PPR - 1);
        k_row[i] = id / C::PPR;
        k_col[i] = (id - k_row[i] * C::PPR) * 8;
        k_goff[i] = k_row[i] * (int)p.ld + k_col[i];
        k_loff[i] = k_row[i] * C::KROW + k_col[i];
    }
#pragma unroll
    for (int i = 0; i < NPV; ++i) {
        const int id = min(tid + NT * i, DH * 8 - 1);
        v_goff[i] = (id >> 3) * (int)vt_row + (id & 7) * 8;
        v_loff[i] = (id >> 3) * C::VROW + (id & 7) * 8;
    }
    // Tile cursors: K rows and V^T positions of consecutive tiles are 64 apart, except at a frame
    // boundary of a ragged S (the frame's last tile is short in K, padded to Spad in V^T).  Uniform
    // pointer bumps instead of a tile -> (frame, tile-in-frame) division per load.
    const int k_wrap = S - (tpf - 1) * 64, v_wrap = p.Spad - (tpf - 1) * 64;
    const int64_t k_wrap_off = p.k_fs - (int64_t)(tpf - 1) * 64 * p.ld;
    const E* k_next = kg + f_lo * p.k_fs;   // first row of the next K tile to load
    const E* v_next = vg + (int64_t)f_lo * p.Spad;
    int k_tt = 0, v_tt = 0;                            // its tile index within the frame
    [[maybe_unused]] SetWalk k_walk{}, v_walk{};       // frame-set launches: the member frame each cursor stands in
    if constexpr (is_set<P>) k_walk.init(run), v_walk.init(run);
    auto load_k = [&]() {
        const bool wrap = k_tt == tpf - 1;
        const int rlim = wrap ? k_wrap - 1 : 63;
        const int clamp_off = rlim * (int)p.ld;
#pragma unroll
        for (int i = 0; i < NPK; ++i) rk[i] = ld16(k_next + (k_row[i] <= rlim ? k_goff[i] : clamp_off + k_col[i]));
        k_next += wrap ? k_wrap_off : (int64_t)64 * p.ld;
        if constexpr (is_set<P>) {
            if (wrap) k_next += (int64_t)k_walk.hop() * p.k_fs;   // on to the next member frame
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
        E* kb = sK(buf);
#pragma unroll
        for (int i = 0; i < NPK; ++i)
            if (tid + NT * i < 64 * C::PPR) st16(kb + k_loff[i], rk[i]);
    };
    auto write_v = [&](int buf) {
        E* vb = sV(buf);
#pragma unroll
        for (int i = 0; i < NPV; ++i)
            if (tid + NT * i < DH * 8) st16(vb + v_loff[i], rv[i]);
    };

    f32x16 o[2][C::MT], s[2][2];
    vec8 pf[2][4];
    float m_run[2], l_run[2];
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        m_run[qi] = -INFINITY;
        l_run[qi] = 0.f;
#pragma unroll
        for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[qi][mt][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[qi][ks][j] = (E)0.f;
    }
    const float c = p.c;

    // S^T (64 keys x 32 queries) of stream qi from K buffer `buf`
    auto qk = [&](auto qi_c, int buf) {
        constexpr int qi = decltype(qi_c)::value;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[qi][kt][r] = 0.f;
            const E* krow = sK(buf) + (kt * 32 + l31) * C::KROW + 8 * hi;
#pragma unroll
            for (int t = 0; t < C::KS; ++t)
                s[qi][kt] = T::mfma32(__builtin_bit_cast(vec8, ld16(krow + 16 * t)), qf[qi][t], s[qi][kt]);
        }
    };
    // O^T += V^T . P of stream qi from V buffer `buf`
    auto pv = [&](auto qi_c, int buf) {
        constexpr int qi = decltype(qi_c)::value;
#pragma unroll
        for (int mt = 0; mt < C::MT; ++mt) {
            const E* vrow = sV(buf) + (mt * 32 + l31) * C::VROW + 8 * hi;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                o[qi][mt] = T::mfma32(__builtin_bit_cast(vec8, ld16(vrow + 16 * ks)), pf[qi][ks], o[qi][mt]);
        }
    };
    // first half of the online softmax: mask, row max, (rare) rescale.  Returns m*c.
    auto sm_head = [&](auto qi_c, int tile) -> float {   // tile = index within the frame
        constexpr int qi = decltype(qi_c)::value;

        if (ragged) {
            const int tt = tile - (tile / tpf) * tpf;
            if (tt == tpf - 1) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (tt * 64 + kt * 32 + cd_row(r, hi) >= S) s[qi][kt][r] = -INFINITY;
            }
        }
        float mx = s[qi][0][0];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[qi][kt][r]);
        mx = max_with_lane_xor32(mx);
        const bool over = mx > m_run[qi] + TF_ATTN_LAG / c;   // lagged reference point (see ext_attn_il_kernel), per query
        if (__any(over)) {
            const float m_new = over ? mx : m_run[qi];
            const float alpha = __builtin_amdgcn_exp2f((m_run[qi] - m_new) * c);
            m_run[qi] = m_new;
            l_run[qi] *= alpha;
#pragma unroll
            for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[qi][mt][r] *= alpha;
        }
        return m_run[qi] * c;
    };
    // One overlapped region: stream X finishes its softmax (P = exp2(s*c - m*c), rounded to the MFMA
    // input type) on the VALU while stream Y = 1-X runs O_Y += V P_Y (vbuf) and S_Y = K Q_Y (kbuf) on
    // the matrix pipe.  The region is cut into NMFMA steps, each = { LDS fragment read for step i+2,
    // MFMA i, its share of the 16 (pk_fma, 2 exp, cvt_pk) softmax units }, and a sched_barrier(0)
    // after every step pins that order: the wave's in-order issue then alternates matrix and vector work.
    auto region = [&](auto x_c, float mc, int vbuf, int kbuf) {
        constexpr int X = decltype(x_c)::value;
        constexpr int Y = 1 - X;
        constexpr PpSchedule<C::MT, C::KS> sch{};
        constexpr int PF = 4;   // fragment reads run PF steps ahead of their MFMA (LDS latency)
        float lsum = 0.f;
        const E* vbase = sV(vbuf) + l31 * C::VROW + 8 * hi;
        const E* kbase = sK(kbuf) + l31 * C::KROW + 8 * hi;
        auto frag = [&](int i) -> vec8 {
            if (sch.is_pv[i]) return __builtin_bit_cast(vec8, ld16(vbase + sch.chain[i] * 32 * C::VROW + 16 * sch.kstep[i]));
            return __builtin_bit_cast(vec8, ld16(kbase + sch.chain[i] * 32 * C::KROW + 16 * sch.kstep[i]));
        };
        vec8 fr[NMFMA];
#pragma unroll
        for (int i = 0; i < PF; ++i) fr[i] = frag(i);
        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NMFMA; ++i) {
            if (i + PF < NMFMA) fr[i + PF] = frag(i + PF);
            if (sch.is_pv[i]) {
                o[Y][sch.chain[i]] = T::mfma32(fr[i], pf[Y][sch.kstep[i]], o[Y][sch.chain[i]]);
            } else {
                s[Y][sch.chain[i]] =
                    T::mfma32(fr[i], qf[Y][sch.kstep[i]], sch.kstep[i] == 0 ? zero : s[Y][sch.chain[i]]);
            }
#pragma unroll
            for (int un = (i * 16) / NMFMA; un < ((i + 1) * 16) / NMFMA; ++un) {
                const int kt = un >> 3, r = (un & 7) * 2;
                // two scalar v_fma_f32, NOT one v_pk_fma_f32: packed f32 VALU beside MFMAs costs ~+22 cycles each
                const float p0 = __builtin_amdgcn_exp2f(fmaf(s[X][kt][r], c, -mc));
                const float p1 = __builtin_amdgcn_exp2f(fmaf(s[X][kt][r + 1], c, -mc));
                const E e0 = (E)p0, e1 = (E)p1;
                lsum += (float)e0 + (float)e1;   // the rounded P: numerator and denominator see the same values
                pf[X][kt * 2 + (r >> 3)][r & 7] = e0;
                pf[X][kt * 2 + (r >> 3)][(r & 7) + 1] = e1;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        l_run[X] += lsum;
        // P_X must exist HERE: an empty asm with the registers as read-write operands keeps the compiler
        // from sinking the (register-only) softmax past the next barrier, next to its consumer
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(pf[X][ks]));
    };
    typedef std::integral_constant<int, 0> A;
    typedef std::integral_constant<int, 1> B;

    // ---- prologue: K(0) -> Kbuf[0]; S_A(0); registers <- K(1), V(0)
    load_k();                   // K(0)
    __syncthreads();            // LDS init done before the first staging write
    write_k(0);
    if (ntiles > 1) load_k();   // K(1)   (with a single tile rk keeps K(0): written to Kbuf[1], read by a dead S_A(1))
    load_v();                   // V(0)
    __syncthreads();
    qk(A{}, 0);

    int tt = 0;   // tile index of t within its frame
    for (int t = 0; t < ntiles; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        // ================= R1(t) =================
        // Kbuf[nxt] held K(t-1) (last read in R1(t-1)), Vbuf[cur] held V(t-2) (last read in R1(t-1)):
        // every wave has passed the barrier of iteration t-1, which follows R1(t-1) -> free to overwrite.
        write_k(nxt);   // K(t+1)
        write_v(cur);   // V(t)
        if (t + 2 < ntiles) load_k();   // K(t+2)
        if (t + 1 < ntiles) load_v();   // V(t+1)
        // P_A(t) (VALU)  ||  O_B += V(t-1) P_B(t-1) from Vbuf[(t-1)&1],  S_B(t) = K(t) Q_B from Kbuf[t&1] (MFMA)
        region(A{}, sm_head(A{}, tt), nxt, cur);
        __syncthreads();   // K(t+1), V(t) visible to all waves; all waves done with R1(t)
        __builtin_amdgcn_sched_barrier(0);
        // ================= R2(t) =================
        // P_B(t) (VALU)  ||  O_A += V(t) P_A(t) from Vbuf[t&1],  S_A(t+1) = K(t+1) Q_A from Kbuf[(t+1)&1]
        // (a dead tile after the last t) (MFMA)
        region(B{}, sm_head(B{}, tt), cur, nxt);
        tt = tt == tpf - 1 ? 0 : tt + 1;
    }
    pv(B{}, (ntiles - 1) & 1);         // drain: O_B += V(n-1) P_B(n-1)

    // ---- epilogue
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        const float l_tot = l_run[qi] + __shfl_xor(l_run[qi], 32);
        if constexpr (RUN) {
            if (q_ok[qi]) {
                constexpr int PS = DH + 8;
                const int64_t R = (((int64_t)(b - 1) * Kq + f) * H + h) * S + q_row[qi];
                float* row = p.partials + R * p.pslots * PS;
#pragma unroll
                for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                    for (int rg = 0; rg < 4; ++rg) {
                        const int d0 = mt * 32 + 8 * rg + 4 * hi;
                        f32x4 w;
#pragma unroll
                        for (int i = 0; i < 4; ++i) w[i] = o[qi][mt][rg * 4 + i];
                        *reinterpret_cast<f32x4*>(row + d0) = w;
                    }
                if (hi == 0) {
                    row[DH] = l_tot;
                    row[DH + 1] = m_run[qi] * c;
                }
            }
            continue;
        }
        const float inv_l = 1.0f / l_tot;
        if (q_ok[qi]) {
            const int64_t op = b * p.o_bs + f * p.o_fs + (int64_t)q_row[qi] * (H * DH) + h * DH;
#pragma unroll
            for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int d0 = mt * 32 + 8 * rg + 4 * hi;
                    f32x4 w;
#pragma unroll
                    for (int i = 0; i < 4; ++i) w[i] = o[qi][mt][rg * 4 + i] * inv_l;
                    store_out4<E, vec4>(p.out, op + d0, w, p.out_f32);
                }
        }
    }
}

// Plan token `pp<64,ALL..>`: the head dim and the problem set the kernel is written for.
template <typename T, bool RUN = false, typename P>
int launch_pp(const P& p_in, hipStream_t st) {
    launch_params_t<P, MODE_ALL, RUN> p = p_in;   // the kernel's parameter block
    constexpr size_t lds = AttnCfg<64>::lds_bytes(1);
    if (tf_plan_note("pp<64,ALL%s>%s", RUN ? ",run" : "", table_mark<decltype(p)>())) return 0;
    auto kern = ext_attn_pp_kernel<T, RUN, decltype(p)>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    p.nQT = (p.S + 255) / 256;
    const int per_branch = p.Kq * p.nQT * p.H;
    // bank problems are decoded first: a bank-only launch simply stops before the source problems
    const unsigned grid = (unsigned)((p.part == TF_ATTN_BANK_ONLY ? 2 : 3) * per_branch);
    // Run launches: K(1) is fetched under `ntiles > 1`, K(t+2) under `t + 2 < ntiles`, V(t+1) under `t + 1 < ntiles`; a short
    // last tile clamps its K rows to the frame's last key.  The dead S_A(n) behind the last tile multiplies what is already in
    // LDS (K(n-1) again) and is never used.  No fetch passes the run's last tile.
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, p);
    TF_LAUNCH_CHECK("tf_ext_attn_fwd");
    return 0;
}

}  // namespace
