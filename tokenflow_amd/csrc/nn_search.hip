// Nearest-neighbour token search for gfx950:
//   idx[p, t] = argmax_j <tgt[t], piv[kf[p], j]> * inv_norm[kf[p], j]
// replaces util.py:61-69 (batch_cosine_sim) + tokenflow_utils.py:335-343 (chunk + argmax)
// of omerbt/TokenFlow.  The [n*S, P*S] similarity matrix never leaves registers.
//
// Structure: a GEMM with an argmax epilogue.  M = pivots (MFMA A operand, rows),
// N = targets (B operand, columns), contraction over D.  With the 32x32 C/D map a
// lane owns ONE target column and 16 pivot rows per tile, so the running
// (max, argmax) over pivots is lane-local; lanes l and l+32 are merged once at the
// end, then the two pivot-half waves through LDS.  A workgroup owns TN targets and
// sweeps ALL S pivots of its keyframe, so there is no cross-workgroup merge.
//   workgroup = 256 threads = 4 waves as 2 (pivot halves) x 2 (target halves)
//   tile      = 128 pivots x TN targets x 64 (D chunk), TN = 64*WN... see below
//   LDS       = double-buffered A/B chunk images, 128-B rows, 16-B slots XOR-swizzled
//               with ((row >> 1) & 7) -> conflict-free ds_read_b128 fragment reads
//   pipeline  = global->register prefetch of chunk i+1 issued before the MFMAs of
//               chunk i, LDS write after them, one barrier per chunk.
// Two kernels share that epilogue:
//   nn_search_rb_kernel<T, DK>  (D = 16*DK <= 320): the wave's 32 target rows live in REGISTERS as
//               MFMA B fragments for the whole kernel (80 VGPRs at D = 320), so only the pivot
//               tiles [32][D] stream through LDS (one ds_read_b128 per MFMA, no target restaging).
//   nn_search_kernel<T, WN>     (any D): both operands staged in 64-wide D chunks.
// Parallelism: grid = (target panels, P keyframes, SPLITS of the pivot range).  With SPLITS > 1
// every workgroup writes its (best score, index) per target to scratch and nn_finalize_kernel
// merges them in ascending split order (strict '>', so the first index still wins on ties).
#include <stdlib.h>

#include <type_traits>

#include "tf_common.h"

namespace {

// byte offset of 16-B piece `piece` of row `row` in a [rows][BK] 16-bit tile, BK = 64, 128 or 256 (D chunk).
// 128-B rows: two rows share a 256-B bank row -> XOR by (row >> 1) & 7; 256-B and 512-B rows: XOR by row & 15
// (16 consecutive rows reading the same piece fall into 16 different 16-B bank groups).
template <int BK>
__device__ __forceinline__ int swz_off(int row, int piece) {
    if constexpr (BK == 64) return row * 128 + ((piece ^ ((row >> 1) & 7)) << 4);
    return row * (BK * 2) + ((piece ^ (row & 15)) << 4);
}

// ---------------------------------------------------------------------------
// inv_norm[r] = 1 / ||piv[r]||_2, one wave per row.
template <typename T>
__global__ __launch_bounds__(256) void pivot_inv_norm_kernel(const typename T::elem* __restrict__ piv,
                                                             float* __restrict__ inv_norm, int64_t rows, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r = wave; r < rows; r += nwaves) {
        const float inv = tf_row_inv_norm<T>(piv + r * D, D, lane);
        if (lane == 0) inv_norm[r] = inv;
    }
}

// ---------------------------------------------------------------------------
// WN = 32-target sub-tiles per wave (1 or 2): workgroup covers TN = 64*WN targets.
// BK = D chunk per barrier interval: 64, or 128 / 256 for small problems (few workgroups, where the per-iteration
//      global-load latency is exposed: halving the iteration count halves the run time).
// TM = pivots per tile: 128, or 64 with BK = 256 (the LDS holds two (TM + TN) x BK stages).
template <typename T, int WN, int BK, int TM, typename CHT = NnChunks>
__global__ __launch_bounds__(256) void nn_search_kernel(const typename T::elem* __restrict__ tgt,
                                                        const typename T::elem* __restrict__ piv,
                                                        const float* __restrict__ inv_norm,
                                                        int32_t* __restrict__ idx_out,
                                                        NnPartial* __restrict__ part_out, int64_t n_tgt, int S,
                                                        int D, int kf0, int kf1, int tiles_per_split, CHT ch) {
    typedef typename T::vec8 vec8;
    constexpr int TN = 64 * WN;
    constexpr int NI = TM / 64;              // 32-pivot sub-tiles per wave
    constexpr int WR = 32 * NI;              // pivot rows per wave half
    constexpr int PPR = BK / 8;              // 16-B pieces per chunk row
    constexpr int A_BYTES = TM * BK * 2;
    constexpr int B_BYTES = TN * BK * 2;
    constexpr int NPA = TM * PPR / 256;      // 16-B pieces per thread, A chunk
    constexpr int NPB = TN * PPR / 256;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    auto sA = [&](int b) { return smem + b * (A_BYTES + B_BYTES); };
    auto sB = [&](int b) { return smem + b * (A_BYTES + B_BYTES) + A_BYTES; };
    float* sInv = reinterpret_cast<float*>(smem + 2 * (A_BYTES + B_BYTES));  // [2][TM]
    float* sBestV = sInv + 2 * TM;                                           // [2][TN]
    int* sBestI = reinterpret_cast<int*>(sBestV + 2 * TN);                   // [2][TN]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1;  // pivot half  (rows wr*WR .. +WR-1 of the tile)
    const int wc = wave & 1;   // target half (cols wc*32*WN .. )
    const int hi = lane >> 5;
    const int l31 = lane & 31;

    const int p = blockIdx.y;
    // chunk of the video this target panel belongs to (0 in the single-chunk call): chunk j matches keyframe
    // slots kf0 + j and kf1 + j; the first chunk of the video has ONE keyframe (tokenflow_utils.py:331-333)
    // (ragged launches, CHT = NnRagged: the chunk comes from the panel prefix table instead of the division)
    const NnPanel pan = nn_panel<TN>(ch, blockIdx.x);
    const int chunk = pan.chunk;
    if (p == 1 && nn_chunk_single(ch, chunk)) return;
    const int kf = (p == 0 ? kf0 : kf1) + chunk;
    const typename T::elem* pv = piv + (int64_t)kf * S * D;
    const float* inv = inv_norm + (int64_t)kf * S;
    const int64_t t0 = pan.t0;
    const int64_t t_end = pan.t_end;   // targets of this chunk: [t_end - its n * S, t_end)

    const int n_mt_all = (S + TM - 1) / TM;
    const int mt0 = blockIdx.z * tiles_per_split;           // this workgroup's slice of the pivot tiles
    const int n_mt = min(tiles_per_split, n_mt_all - mt0);
    const int n_kc = (D + BK - 1) / BK;
    const int total = n_mt * n_kc;

    // per-thread staging pieces: piece id = tid + 256*i -> row = id / PPR, col piece = id % PPR.
    // TWO register sets: the loads of chunk it+2 are issued during chunk it and written to LDS at the end of
    // chunk it+1, so a global-load latency is spread over two iterations (the loop is a serial chain of
    // load -> LDS -> barrier -> MFMA steps; with one set every step paid the full latency, ~1.7 us, which
    // is all the time there is at the small levels).
    u32x4 ra2[2][NPA], rb2[2][NPB];
    float rinv2[2] = {0.f, 0.f};

    auto stage_load = [&](int it, auto SET) {
        constexpr int set = decltype(SET)::value;
        u32x4(&ra)[NPA] = ra2[set];
        u32x4(&rb)[NPB] = rb2[set];
        float& rinv = rinv2[set];
        const int mt = it / n_kc, kc = it - mt * n_kc;
        const int col0 = kc * BK;
        // Branch-free: every lane loads from a valid (clamped) address; columns past D are zeroed when the
        // piece is written to LDS.  A predicated load (col < D ? load : 0) becomes an exec-masked branch per
        // load and makes the compiler drain vmcnt(0) before the next batch -- no load ever overlapped a MFMA.
#pragma unroll
        for (int i = 0; i < NPA; ++i) {
            const int id = tid + 256 * i;
            const int r = id / PPR, pc = id % PPR;
            const int row = min((mt0 + mt) * TM + r, S - 1);   // clamped duplicates can never win (see epilogue)
            const int col = min(col0 + pc * 8, D - 8);
            ra[i] = ld16(pv + (int64_t)row * D + col);
        }
#pragma unroll
        for (int i = 0; i < NPB; ++i) {
            const int id = tid + 256 * i;
            const int r = id / PPR, pc = id % PPR;
            const int64_t row = min(t0 + r, t_end - 1);
            const int col = min(col0 + pc * 8, D - 8);
            rb[i] = ld16(tgt + row * D + col);
        }
        rinv = inv[min((mt0 + mt) * TM + min(tid, TM - 1), S - 1)];
    };
    auto stage_write = [&](int it, auto SET) {
        constexpr int set = decltype(SET)::value;
        u32x4(&ra)[NPA] = ra2[set];
        u32x4(&rb)[NPB] = rb2[set];
        const float rinv = rinv2[set];
        const int mt = it / n_kc, kc = it - mt * n_kc;
        const int b = it & 1;
        const int col0 = kc * BK;
        const u32x4 zero = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < NPA; ++i) {
            const int id = tid + 256 * i;
            st16(sA(b) + swz_off<BK>(id / PPR, id % PPR), col0 + (id % PPR) * 8 < D ? ra[i] : zero);
        }
#pragma unroll
        for (int i = 0; i < NPB; ++i) {
            const int id = tid + 256 * i;
            st16(sB(b) + swz_off<BK>(id / PPR, id % PPR), col0 + (id % PPR) * 8 < D ? rb[i] : zero);
        }
        if (kc == 0 && tid < TM) sInv[(mt & 1) * TM + tid] = rinv;
    };

    f32x16 acc[NI][WN];
    float best_v[WN];
    int best_i[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        best_v[j] = -INFINITY;
        best_i[j] = 0;
    }

    typedef std::integral_constant<int, 0> Set0;
    typedef std::integral_constant<int, 1> Set1;
    stage_load(0, Set0{});
    stage_write(0, Set0{});
    if (total > 1) stage_load(1, Set1{});
    __syncthreads();

    // chunk `it` sits in LDS buffer it & 1; register set (it + 1) & 1 holds chunk it + 1, set it & 1 is free
    auto step = [&](int it, auto CUR, auto NXT) {
        const int mt = it / n_kc, kc = it - mt * n_kc;
        if (it + 2 < total) stage_load(it + 2, CUR);
        if (kc == 0) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        }
        const unsigned char* a = sA(it & 1);
        const unsigned char* b = sB(it & 1);
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            vec8 fa[NI], fb[WN];
#pragma unroll
            for (int i = 0; i < NI; ++i)
                fa[i] = __builtin_bit_cast(vec8, ld16(a + swz_off<BK>(wr * WR + i * 32 + l31, ks * 2 + hi)));
#pragma unroll
            for (int j = 0; j < WN; ++j)
                fb[j] = __builtin_bit_cast(vec8, ld16(b + swz_off<BK>((wc * WN + j) * 32 + l31, ks * 2 + hi)));
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = T::mfma32(fa[i], fb[j], acc[i][j]);
        }
        if (kc == n_kc - 1) {
            // argmax epilogue: rows visited in ascending order, strict '>' keeps the first maximum
            const float* si = sInv + (mt & 1) * TM;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = wr * WR + i * 32 + cd_row(r, hi);
                    const float w = si[rl];
                    const int gi = (mt0 + mt) * TM + rl;
#pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        const float sc = acc[i][j][r] * w;
                        if (sc > best_v[j]) {
                            best_v[j] = sc;
                            best_i[j] = gi;
                        }
                    }
                }
            }
        }
        if (it + 1 < total) stage_write(it + 1, NXT);
        __syncthreads();
    };
    for (int it = 0; it < total; it += 2) {   // unrolled by two so the register sets are compile-time names
        step(it, Set0{}, Set1{});
        if (it + 1 < total) step(it + 1, Set1{}, Set0{});
    }

    // merge lane l with lane l+32 (interleaved row sets): tie -> smaller index
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const float ov = __shfl_xor(best_v[j], 32);
        const int oi = __shfl_xor(best_i[j], 32);
        if (ov > best_v[j] || (ov == best_v[j] && oi < best_i[j])) {
            best_v[j] = ov;
            best_i[j] = oi;
        }
        if (hi == 0) {
            const int col = (wc * WN + j) * 32 + l31;
            sBestV[wr * TN + col] = best_v[j];
            sBestI[wr * TN + col] = best_i[j];
        }
    }
    __syncthreads();
    if (tid < TN) {
        float v0 = sBestV[tid], v1 = sBestV[TN + tid];
        int i0 = sBestI[tid], i1 = sBestI[TN + tid];
        if (v1 > v0 || (v1 == v0 && i1 < i0)) {
            i0 = i1;
            v0 = v1;
        }
        i0 = i0 < S ? i0 : S - 1;  // a clamped duplicate of row S-1 maps back to S-1
        const int64_t t = t0 + tid;
        if (t < t_end) {
            if (part_out)
                part_out[((int64_t)blockIdx.z * gridDim.y + p) * n_tgt + t] = NnPartial{v0, i0};
            else
                idx_out[(int64_t)p * n_tgt + t] = i0;
        }
    }
}

// ---------------------------------------------------------------------------
// LDS-DMA variant for D % 64 == 0, D >= 512 (levels 1-2 of SD: D = 640, 1280) on grids that fill the chip.
// The generic kernel above is LDS-bound there: a wave's 64 x 64 tile reads 4 fragments of 1 KB per 4 MFMAs and
// re-stages (TM + TN) x BK per interval through registers -- 1.5 KB of LDS traffic per MFMA against the 1 KB the LDS
// pipe (128 B/clk per CU) delivers in the 32 clocks an MFMA occupies one of the CU's four matrix pipes (counters:
// profiles/r04_pmc_level1.csv).  Here a wave owns 64 pivots x 128 targets (6 fragment reads per 8 MFMAs) inside a
// 256 x 256 workgroup tile of 8 waves (4 pivot quarters x 2 target halves): 0.75 + 0.25 KB per MFMA.  The 128
// accumulator registers leave no room for two register staging sets (profiles/r04_nn_wide4_ab.txt: spills), so the
// tiles go global -> LDS directly (`global_load_lds_dwordx4`: no staging registers, no ds_write pass).  The DMA
// writes lane-linearly (wave-uniform base + lane * 16 B): the XOR swizzle of the image is applied on the SOURCE side
// (the lane that fills slot s of row r fetches piece s ^ ((r >> 1) & 7) of that row) and on the read side, the same
// involution (swz_off<64>).  Two LDS buffers; the DMA of chunk it+1 is issued before the MFMAs of chunk it and
// drained (vmcnt(0)) in front of the interval's barrier.  The pivots' inverse norms of a tile arrive the same way.
// Arithmetic per (target, pivot) and the first-index rule are those of nn_search_kernel.
// SH (round 6, last session): the wave's 64 x 128 tile as 4 x 8 sub-tiles of v_mfma_f32_16x16x32 instead of 2 x 4 of 32x32x16 -- same
// images, same bytes through the LDS, same matrix-pipe clocks and accumulator registers; the short shape sustains more on these
// power-limited boxes (see nn_search_rbs_kernel).  32 features per MFMA: scores differ from the SH = false kernel's in the last bit.
template <typename T, bool SH = false, typename CHT = NnChunks>
__global__ __launch_bounds__(512, 2) void nn_search_glds_kernel(const typename T::elem* __restrict__ tgt,
                                                                const typename T::elem* __restrict__ piv,
                                                                const float* __restrict__ inv_norm,
                                                                int32_t* __restrict__ idx_out,
                                                                NnPartial* __restrict__ part_out, int64_t n_tgt, int S,
                                                                int D, int kf0, int kf1, int tiles_per_split, CHT ch) {
    typedef typename T::vec8 vec8;
    typedef typename T::elem E;
    constexpr int TM = 256, TN = 256, BK = 64, NI = 2, WN = 4;
    constexpr int A_BYTES = TM * BK * 2, B_BYTES = TN * BK * 2;   // 32 KB each
    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* glb_ptr;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    auto sA = [&](int b) { return smem + b * (A_BYTES + B_BYTES); };
    auto sB = [&](int b) { return smem + b * (A_BYTES + B_BYTES) + A_BYTES; };
    float* sInv = reinterpret_cast<float*>(smem + 2 * (A_BYTES + B_BYTES));   // [2][TM]
    float* sBestV = sInv + 2 * TM;                                            // [4][TN]
    int* sBestI = reinterpret_cast<int*>(sBestV + 4 * TN);                    // [4][TN]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1;   // pivot quarter (rows wr*64 .. +63 of the tile)
    const int wc = wave & 1;    // target half   (cols wc*128 .. +127)
    const int hi = lane >> 5;
    const int l31 = lane & 31;
    const int g = lane >> 4, n16 = lane & 15;   // SH: 16-lane row (k-block of A / B, row group of C), row / column in a sub-tile
    constexpr int NB = SH ? 2 * WN : WN;        // running (max, argmax) pairs per lane: one per target sub-tile

    const int p = blockIdx.y;
    const NnPanel pan = nn_panel<TN>(ch, blockIdx.x);
    const int chunk = pan.chunk;
    if (p == 1 && nn_chunk_single(ch, chunk)) return;
    const int kf = (p == 0 ? kf0 : kf1) + chunk;
    const E* pv = piv + (int64_t)kf * S * D;
    const float* inv = inv_norm + (int64_t)kf * S;
    const int64_t t0 = pan.t0;
    const int64_t t_end = pan.t_end;

    const int n_mt_all = (S + TM - 1) / TM;
    const int mt0 = blockIdx.z * tiles_per_split;
    const int n_mt = min(tiles_per_split, n_mt_all - mt0);
    const int n_kc = D / BK;
    const int total = n_mt * n_kc;

    // DMA pieces of this lane: wave w fills rows (w*4 + j)*8 .. +7 of both images, j = 0..3; lane -> row l/8, slot l%8
    const int sub = lane >> 3, slot = lane & 7;
    const E* b_src[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (wave * 4 + j) * 8 + sub;
        const int64_t row = min(t0 + r, t_end - 1);            // clamped duplicates: never written back
        b_src[j] = tgt + row * D + ((slot ^ ((r >> 1) & 7)) << 3);
    }
    int a_off[4];   // element offset of this lane's piece inside the pivot tile (re-clamped per tile)
    auto set_tile = [&](int mt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = (wave * 4 + j) * 8 + sub;
            const int row = min((mt0 + mt) * TM + r, S - 1);   // clamped duplicates can never win (see epilogue)
            a_off[j] = row * D + ((slot ^ ((r >> 1) & 7)) << 3);
        }
    };
    // DMA pieces j = 0..3 of chunk `it` (one A and one B piece each), issued as one block in front of the k-loop of the
    // chunk in flight.  Spreading them over the k-steps, each pair behind a k-step's 8 MFMAs and pinned there with
    // sched_barriers (TF_TUNE_GLDS_SPREAD_ISSUE), measured 1-4 % slower (profiles/r05_nn_glds_ab.txt): with two waves per
    // SIMD the other wave's MFMAs already cover a wave's issue time, and the pinning costs the compiler its own order.
#ifdef TF_TUNE_GLDS_SPREAD_ISSUE
    constexpr bool SPREAD = true;
#else
    constexpr bool SPREAD = false;
#endif
    auto stage_piece = [&](int it, int j) {
        const int mt = it / n_kc, kc = it - mt * n_kc;
        const int b = it & 1;
        if (j == 0 && kc == 0) {
            set_tile(mt);
            if (wave == 0) {   // the tile's inverse norms: 256 floats = one 1 KB DMA piece
                const int row = min((mt0 + mt) * TM + lane * 4, S - 4);
                __builtin_amdgcn_global_load_lds((glb_ptr)(inv + row), (lds_ptr)(sInv + (mt & 1) * TM), 16, 0, 0);
            }
        }
        const int col = kc * BK;
        __builtin_amdgcn_global_load_lds((glb_ptr)(pv + a_off[j] + col), (lds_ptr)(sA(b) + (wave * 4 + j) * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_ptr)(b_src[j] + col), (lds_ptr)(sB(b) + (wave * 4 + j) * 1024), 16, 0, 0);
    };
    auto stage = [&](int it) {
#pragma unroll
        for (int j = 0; j < 4; ++j) stage_piece(it, j);
    };

    f32x16 acc[NI][WN];
    f32x4 acc16[2 * NI][2 * WN];   // SH
    float best_v[NB];
    int best_i[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        best_v[j] = -INFINITY;
        best_i[j] = 0;
    }

    stage(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int it = 0; it < total; ++it) {
        const int mt = it / n_kc, kc = it - mt * n_kc;
        // buffer (it + 1) & 1 was last read in interval it - 1; every wave has passed the barrier that ended it
        const bool more = it + 1 < total;
        if (!SPREAD && more) stage(it + 1);
        if (kc == 0) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
            for (int i = 0; i < 2 * NI; ++i)
#pragma unroll
                for (int j = 0; j < 2 * WN; ++j) acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const unsigned char* a = sA(it & 1);
        const unsigned char* b = sB(it & 1);
        if constexpr (SH) {
#pragma unroll
            for (int ks = 0; ks < BK / 32; ++ks) {
                vec8 fa[2 * NI], fb[2 * WN];
#pragma unroll
                for (int i = 0; i < 2 * NI; ++i)
                    fa[i] = __builtin_bit_cast(vec8, ld16(a + swz_off<BK>(wr * 64 + i * 16 + n16, ks * 4 + g)));
#pragma unroll
                for (int j = 0; j < 2 * WN; ++j)
                    fb[j] = __builtin_bit_cast(vec8, ld16(b + swz_off<BK>((wc * 2 * WN + j) * 16 + n16, ks * 4 + g)));
#pragma unroll
                for (int i = 0; i < 2 * NI; ++i)
#pragma unroll
                    for (int j = 0; j < 2 * WN; ++j) acc16[i][j] = T::mfma16(fa[i], fb[j], acc16[i][j]);
            }
        } else
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            vec8 fa[NI], fb[WN];
#pragma unroll
            for (int i = 0; i < NI; ++i)
                fa[i] = __builtin_bit_cast(vec8, ld16(a + swz_off<BK>(wr * 64 + i * 32 + l31, ks * 2 + hi)));
#pragma unroll
            for (int j = 0; j < WN; ++j)
                fb[j] = __builtin_bit_cast(vec8, ld16(b + swz_off<BK>((wc * WN + j) * 32 + l31, ks * 2 + hi)));
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = T::mfma32(fa[i], fb[j], acc[i][j]);
            if (SPREAD) {
                __builtin_amdgcn_sched_barrier(0);
                if (more) stage_piece(it + 1, ks);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (kc == n_kc - 1) {
            // argmax epilogue: rows visited in ascending order, strict '>' keeps the first maximum
            const float* si = sInv + (mt & 1) * TM;
            const int last = S - 1 - (mt0 + mt) * TM;   // rows past S are copies of row S - 1: give them ITS inverse norm
            if constexpr (SH) {
#pragma unroll
                for (int i = 0; i < 2 * NI; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rl = wr * 64 + i * 16 + 4 * g + r;   // ascending within the lane
                        const float w = si[min(rl, last)];
                        const int gi = (mt0 + mt) * TM + rl;
#pragma unroll
                        for (int j = 0; j < 2 * WN; ++j) {
                            const float sc = acc16[i][j][r] * w;
                            if (sc > best_v[j]) {
                                best_v[j] = sc;
                                best_i[j] = gi;
                            }
                        }
                    }
            } else
#pragma unroll
            for (int i = 0; i < NI; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = wr * 64 + i * 32 + cd_row(r, hi);
                    const float w = si[min(rl, last)];
                    const int gi = (mt0 + mt) * TM + rl;
#pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        const float sc = acc[i][j][r] * w;
                        if (sc > best_v[j]) {
                            best_v[j] = sc;
                            best_i[j] = gi;
                        }
                    }
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    if constexpr (SH) {   // the four 16-lane rows hold disjoint pivot rows of a target: merge, smaller index on equal scores
#pragma unroll
        for (int j = 0; j < NB; ++j) {
#pragma unroll
            for (int o_ = 16; o_ <= 32; o_ <<= 1) {
                const float ov = __shfl_xor(best_v[j], o_);
                const int oi = __shfl_xor(best_i[j], o_);
                if (ov > best_v[j] || (ov == best_v[j] && oi < best_i[j])) {
                    best_v[j] = ov;
                    best_i[j] = oi;
                }
            }
            if (g == 0) {
                const int col = (wc * NB + j) * 16 + n16;
                sBestV[wr * TN + col] = best_v[j];
                sBestI[wr * TN + col] = best_i[j];
            }
        }
    } else
    // merge lane l with lane l+32 (interleaved row sets): tie -> smaller index
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const float ov = __shfl_xor(best_v[j], 32);
        const int oi = __shfl_xor(best_i[j], 32);
        if (ov > best_v[j] || (ov == best_v[j] && oi < best_i[j])) {
            best_v[j] = ov;
            best_i[j] = oi;
        }
        if (hi == 0) {
            const int col = (wc * WN + j) * 32 + l31;
            sBestV[wr * TN + col] = best_v[j];
            sBestI[wr * TN + col] = best_i[j];
        }
    }
    __syncthreads();
    if (tid < TN) {
        float v0 = sBestV[tid];
        int i0 = sBestI[tid];
#pragma unroll
        for (int q = 1; q < 4; ++q) {   // ascending pivot quarters: strict '>' keeps the first maximum
            const float v1 = sBestV[q * TN + tid];
            const int i1 = sBestI[q * TN + tid];
            if (v1 > v0 || (v1 == v0 && i1 < i0)) {
                i0 = i1;
                v0 = v1;
            }
        }
        i0 = i0 < S ? i0 : S - 1;
        const int64_t t = t0 + tid;
        if (t < t_end) {
            if (part_out)
                part_out[((int64_t)blockIdx.z * gridDim.y + p) * n_tgt + t] = NnPartial{v0, i0};
            else
                idx_out[(int64_t)p * n_tgt + t] = i0;
        }
    }
}

// ---------------------------------------------------------------------------
// Register-B variant for D = 16*DK: one wave = 32 targets whose B fragments stay in registers.
template <typename T, int DK, typename CHT = NnChunks>
__global__ __launch_bounds__(256, 3) void nn_search_rb_kernel(const typename T::elem* __restrict__ tgt,
                                                           const typename T::elem* __restrict__ piv,
                                                           const float* __restrict__ inv_norm,
                                                           int32_t* __restrict__ idx_out,
                                                           NnPartial* __restrict__ part_out, int64_t n_tgt, int S,
                                                           int kf0, int kf1, int tiles_per_split, CHT ch) {
    typedef typename T::elem E;
    typedef typename T::vec8 vec8;
    constexpr int D = 16 * DK;
    constexpr int TMR = 32;                  // pivots per tile
    constexpr int PANEL = 128;               // targets per workgroup
    constexpr int RS = D + 8;                // LDS row stride (elements): odd number of 16-B slots
    constexpr int PPR = D / 8;               // 16-B pieces per row
    constexpr int NP = (TMR * PPR + 255) / 256;
    constexpr int A_ELEMS = TMR * RS;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    auto sA = [&](int b) { return reinterpret_cast<E*>(smem) + b * A_ELEMS; };
    float* sInv = reinterpret_cast<float*>(smem + 2 * A_ELEMS * sizeof(E));  // [2][TMR]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hi = lane >> 5;
    const int l31 = lane & 31;
    const int p = blockIdx.y;
    const NnPanel pan = nn_panel<PANEL>(ch, blockIdx.x);   // see nn_search_kernel
    const int chunk = pan.chunk;
    if (p == 1 && nn_chunk_single(ch, chunk)) return;
    const int kf = (p == 0 ? kf0 : kf1) + chunk;
    const E* pv = piv + (int64_t)kf * S * D;
    const float* inv = inv_norm + (int64_t)kf * S;
    const int64_t t_end = pan.t_end;
    const int64_t t_row = pan.t0 + wave * 32 + l31;

    const int n_mt_all = (S + TMR - 1) / TMR;
    const int mt0 = blockIdx.z * tiles_per_split;
    const int n_mt = min(tiles_per_split, n_mt_all - mt0);

    vec8 fb[DK];
    {
        const E* tp = tgt + (t_row < t_end ? t_row : t_end - 1) * D + 8 * hi;
#pragma unroll
        for (int t = 0; t < DK; ++t) fb[t] = __builtin_bit_cast(vec8, ld16(tp + 16 * t));
    }

    u32x4 ra[NP];
    float rinv = 0.f;
    auto stage_load = [&](int mt) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int id = tid + 256 * i;
            if (id < TMR * PPR) {
                const int r = id / PPR, pc = id - r * PPR;
                int row = (mt0 + mt) * TMR + r;
                row = row < S ? row : S - 1;
                ra[i] = ld16(pv + (int64_t)row * D + pc * 8);
            }
        }
        if (tid < TMR) {
            int row = (mt0 + mt) * TMR + tid;
            rinv = inv[row < S ? row : S - 1];
        }
    };
    auto stage_write = [&](int mt) {
        E* a = sA(mt & 1);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int id = tid + 256 * i;
            if (id < TMR * PPR) {
                const int r = id / PPR, pc = id - r * PPR;
                st16(a + r * RS + pc * 8, ra[i]);
            }
        }
        if (tid < TMR) sInv[(mt & 1) * TMR + tid] = rinv;
    };

    float best_v = -INFINITY;
    int best_i = 0;
    stage_load(0);
    stage_write(0);
    __syncthreads();
    for (int mt = 0; mt < n_mt; ++mt) {
        const bool has_next = mt + 1 < n_mt;
        if (has_next) stage_load(mt + 1);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const E* arow = sA(mt & 1) + l31 * RS + 8 * hi;
#pragma unroll
        for (int t = 0; t < DK; ++t) acc = T::mfma32(__builtin_bit_cast(vec8, ld16(arow + 16 * t)), fb[t], acc);
        const float* si = sInv + (mt & 1) * TMR;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = cd_row(r, hi);
            const float sc = acc[r] * si[rl];
            if (sc > best_v) {
                best_v = sc;
                best_i = (mt0 + mt) * TMR + rl;
            }
        }
        if (has_next) stage_write(mt + 1);
        __syncthreads();
    }
    const float ov = __shfl_xor(best_v, 32);
    const int oi = __shfl_xor(best_i, 32);
    if (ov > best_v || (ov == best_v && oi < best_i)) {
        best_v = ov;
        best_i = oi;
    }
    best_i = best_i < S ? best_i : S - 1;
    if (hi == 0 && t_row < t_end) {
        if (part_out)
            part_out[((int64_t)blockIdx.z * gridDim.y + p) * n_tgt + t_row] = NnPartial{best_v, best_i};
        else
            idx_out[(int64_t)p * n_tgt + t_row] = best_i;
    }
}

// ---------------------------------------------------------------------------
// Register-B variant with the pivot tiles staged by LDS-DMA (global_load_lds_dwordx4) instead of through registers:
// no staging VGPRs, no ds_write pass.  The DMA writes lane-linearly, so the image has no row padding; bank conflicts of
// the fragment reads (32 rows, 640-B stride) are avoided by an XOR swizzle of the 16-B piece index with (row >> 1) & 7,
// applied on the SOURCE address of the DMA and on the read (the same involution; it permutes inside aligned groups of
// 8 pieces, D / 8 being a multiple of 8).  Same arithmetic as nn_search_rbg_kernel.
// TT = target tiles (of 32 rows) per wave.  TT = 2 (round 6): a wave keeps 64 targets in registers (160 VGPRs of B fragments),
// every pivot fragment read from LDS feeds TWO MFMAs on two independent accumulator chains, and a barrier interval carries
// twice the matrix work -- half the LDS traffic and half the barriers per MFMA; 2 waves per SIMD instead of 3.  The
// arithmetic of a (target, pivot) pair is unchanged (same contraction order): the kernels are interchangeable bit for bit.
template <typename T, int DK, int TT = 1, typename CHT = NnChunks>
__global__ __launch_bounds__(256, TT == 1 ? 3 : 2) void nn_search_rbg_kernel(const typename T::elem* __restrict__ tgt,
                                                           const typename T::elem* __restrict__ piv,
                                                           const float* __restrict__ inv_norm,
                                                           int32_t* __restrict__ idx_out,
                                                           NnPartial* __restrict__ part_out, int64_t n_tgt, int S,
                                                           int kf0, int kf1, int tiles_per_split, CHT ch) {
    typedef typename T::elem E;
    typedef typename T::vec8 vec8;
    constexpr int D = 16 * DK;
    constexpr int TMR = 32;                  // pivots per tile
    constexpr int PANEL = 128 * TT;          // targets per workgroup
    constexpr int RS = D;                    // LDS row stride (elements): the DMA image is dense
    static_assert((D / 8) % 8 == 0, "the swizzle permutes inside groups of 8 pieces");
    constexpr int NPIECE = TMR * D * 2 / 1024;   // 1 KB DMA pieces per tile (20 at D = 320)
    static_assert(NPIECE % 4 == 0, "pieces split evenly over the 4 waves");
    constexpr int A_ELEMS = TMR * RS;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    auto sA = [&](int b) { return reinterpret_cast<E*>(smem) + b * A_ELEMS; };
    float* sInv = reinterpret_cast<float*>(smem + 2 * A_ELEMS * sizeof(E));  // [2][TMR]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int hi = lane >> 5;
    const int l31 = lane & 31;
    const int p = blockIdx.y;
    const NnPanel pan = nn_panel<PANEL>(ch, blockIdx.x);   // see nn_search_kernel
    const int chunk = pan.chunk;
    if (p == 1 && nn_chunk_single(ch, chunk)) return;
    const int kf = (p == 0 ? kf0 : kf1) + chunk;
    const E* pv = piv + (int64_t)kf * S * D;
    const float* inv = inv_norm + (int64_t)kf * S;
    const int64_t t_end = pan.t_end;
    int64_t t_row[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
        t_row[tt] = pan.t0 + (wave * TT + tt) * 32 + l31;

    const int n_mt_all = (S + TMR - 1) / TMR;
    const int mt0 = blockIdx.z * tiles_per_split;
    const int n_mt = min(tiles_per_split, n_mt_all - mt0);

    vec8 fb[TT][DK];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        const E* tp = tgt + (t_row[tt] < t_end ? t_row[tt] : t_end - 1) * D + 8 * hi;
#pragma unroll
        for (int t = 0; t < DK; ++t) fb[tt][t] = __builtin_bit_cast(vec8, ld16(tp + 16 * t));
    }

    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* glb_ptr;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // this lane's slot of DMA piece j = wave + 4 * i: byte o of the image -> row o / (2 D), position (o % (2 D)) / 16
    // (S % 32 == 0 in this variant: every tile is full, no row clamp)
    int a_off[NPIECE / 4];
#pragma unroll
    for (int i = 0; i < NPIECE / 4; ++i) {
        const int o = (wave_u + 4 * i) * 1024 + lane * 16;
        const int r = o / (2 * D), pos = (o - r * 2 * D) >> 4;
        a_off[i] = r * D + ((pos ^ ((r >> 1) & 7)) << 3);
    }
    float rinv = 0.f;
    auto stage_load = [&](int mt) {
        unsigned char* a = reinterpret_cast<unsigned char*>(sA(mt & 1));
        const E* tile = pv + (int64_t)(mt0 + mt) * TMR * D;
#pragma unroll
        for (int i = 0; i < NPIECE / 4; ++i)
            __builtin_amdgcn_global_load_lds((glb_ptr)(tile + a_off[i]), (lds_ptr)(a + (wave_u + 4 * i) * 1024), 16, 0, 0);
        if (tid < TMR) {
            int row = (mt0 + mt) * TMR + tid;
            rinv = inv[row < S ? row : S - 1];
        }
    };
    auto stage_write = [&](int mt) {
        if (tid < TMR) sInv[(mt & 1) * TMR + tid] = rinv;
    };

    float best_v[TT];
    int best_i[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) best_v[tt] = -INFINITY, best_i[tt] = 0;
    stage_load(0);
    stage_write(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int mt = 0; mt < n_mt; ++mt) {
        const bool has_next = mt + 1 < n_mt;
        if (has_next) stage_load(mt + 1);
        f32x16 acc[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tt][r] = 0.f;
        const E* arow = sA(mt & 1) + l31 * RS;
        const int swz = (l31 >> 1) & 7;
#pragma unroll
        for (int t = 0; t < DK; ++t) {
            const vec8 fa = __builtin_bit_cast(vec8, ld16(arow + (((2 * t + hi) ^ swz) << 3)));
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc[tt] = T::mfma32(fa, fb[tt][t], acc[tt]);
        }
        const float* si = sInv + (mt & 1) * TMR;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = cd_row(r, hi);
            const float w = si[rl];
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) {
                const float sc = acc[tt][r] * w;
                if (sc > best_v[tt]) {
                    best_v[tt] = sc;
                    best_i[tt] = (mt0 + mt) * TMR + rl;
                }
            }
        }
        if (has_next) stage_write(mt + 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        const float ov = __shfl_xor(best_v[tt], 32);
        const int oi = __shfl_xor(best_i[tt], 32);
        float bv = best_v[tt];
        int bi = best_i[tt];
        if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
        bi = bi < S ? bi : S - 1;
        if (hi == 0 && t_row[tt] < t_end) {
            if (part_out)
                part_out[((int64_t)blockIdx.z * gridDim.y + p) * n_tgt + t_row[tt]] = NnPartial{bv, bi};
            else
                idx_out[(int64_t)p * n_tgt + t_row[tt]] = bi;
        }
    }
}

// ---------------------------------------------------------------------------
// The two-target-tile kernel above with SHORT MFMAs (round 6, last session): v_mfma_f32_16x16x32 instead of 32x32x16.  Same
// workgroup (4 waves x 64 targets), same LDS image of a pivot tile (32 x D, dense, DMA-staged, pieces XOR-swizzled with
// (row >> 1) & 7 -- conflict-free for this read pattern too), same bytes through the LDS per flop, same matrix-pipe clocks:
// a wave's 64 targets are four 16-target B-fragment sets (160 VGPRs), a pivot tile two 16-row A fragments per 32-wide k-step,
// each feeding four MFMAs.  Why: on these power-limited boxes the short shape sustains ~16 % more in an MFMA-bound loop
// (tools/ubench/nn_loop_proxy.hip: 1 810 against 1 555 TF/s in the stripped loop of this kernel; the bare MFMAs 2 213 against
// 1 894, profiles/r02_mfma_shapes.txt) -- less accumulator traffic per flop.
// TJ = 16-target sub-tiles per wave: 4 (the two-target-tile form: 256 targets per workgroup) or 2 (the one-tile form: 128).
// Arithmetic: a (target, pivot) dot product is summed 32 features per MFMA in ascending order -- NOT bit-identical to the
// 16-wide steps of the other search kernels (fp32 rounding of the partial sums); exact duplicates still tie exactly (the same
// instruction sequence on the same data) and the first index wins as everywhere (ascending rows, strict '>').
// The tile loop is software-pipelined: fragment addresses as base + immediate, a ring of fragments read ahead
// of their MFMAs with counted waits, and half-tile phases whose argmax fold runs beside the MFMAs of the next half.
template <typename T, int DK, int TJ = 4, typename CHT = NnChunks>
__global__ __launch_bounds__(256, TJ == 4 ? 2 : 3) void nn_search_rbs_kernel(const typename T::elem* __restrict__ tgt,
                                                               const typename T::elem* __restrict__ piv,
                                                               const float* __restrict__ inv_norm,
                                                               int32_t* __restrict__ idx_out,
                                                               NnPartial* __restrict__ part_out, int64_t n_tgt, int S,
                                                               int kf0, int kf1, int tiles_per_split, CHT ch) {
    typedef typename T::elem E;
    typedef typename T::vec8 vec8;
    constexpr int D = 16 * DK;
    constexpr int KS32 = D / 32;             // 32-wide k-steps
    static_assert(D % 32 == 0 && (D / 8) % 8 == 0, "32-wide k-steps; the swizzle permutes inside groups of 8 pieces");
    constexpr int TMR = 32;                  // pivots per tile
    constexpr int PANEL = 64 * TJ;           // targets per workgroup
    constexpr int NPIECE = TMR * D * 2 / 1024;
    static_assert(NPIECE % 4 == 0, "pieces split evenly over the 4 waves");
    constexpr int A_ELEMS = TMR * D;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* sInv = reinterpret_cast<float*>(smem + 2 * A_ELEMS * sizeof(E));  // [2][TMR]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int g = lane >> 4;      // 16-lane row: the k-block of the A / B fragments, the row group of C
    const int n16 = lane & 15;    // A: pivot row of the 16-row sub-tile; B / C: target of the 16-target sub-tile
    const int p = blockIdx.y;
    const NnPanel pan = nn_panel<PANEL>(ch, blockIdx.x);   // see nn_search_kernel
    const int chunk = pan.chunk;
    if (p == 1 && nn_chunk_single(ch, chunk)) return;
    const int kf = (p == 0 ? kf0 : kf1) + chunk;
    const E* pv = piv + (int64_t)kf * S * D;
    const float* inv = inv_norm + (int64_t)kf * S;
    const int64_t t_end = pan.t_end;
    int64_t t_row[TJ];
#pragma unroll
    for (int j = 0; j < TJ; ++j)
        t_row[j] = pan.t0 + wave * (16 * TJ) + 16 * j + n16;

    const int n_mt_all = (S + TMR - 1) / TMR;
    const int mt0 = blockIdx.z * tiles_per_split;
    const int n_mt = min(tiles_per_split, n_mt_all - mt0);

    vec8 fb[TJ][KS32];
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
        const E* tp = tgt + (t_row[j] < t_end ? t_row[j] : t_end - 1) * D + 8 * g;
#pragma unroll
        for (int t = 0; t < KS32; ++t) fb[j][t] = __builtin_bit_cast(vec8, ld16(tp + 32 * t));
    }

    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* glb_ptr;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    int a_off[NPIECE / 4];
#pragma unroll
    for (int i = 0; i < NPIECE / 4; ++i) {
        const int o = (wave_u + 4 * i) * 1024 + lane * 16;
        const int r = o / (2 * D), pos = (o - r * 2 * D) >> 4;
        a_off[i] = r * D + ((pos ^ ((r >> 1) & 7)) << 3);
    }
    float rinv = 0.f;
    // The DMA is issued from an asm statement (M0 = the piece's LDS address, saved and restored), not through
    // __builtin_amdgcn_global_load_lds: the compiler books the builtin as a flat access that may touch LDS, and while one
    // is pending -- here: the whole tile -- it turns every wait for a fragment read into lgkmcnt(0), the ring's read-ahead
    // included.  Nothing changes in what is copied where; the data is ordered as before by the vmcnt(0) and the barrier
    // at the end of the tile.
    const unsigned lds0 = (unsigned)(size_t)(lds_ptr)smem;
    auto stage_load = [&](int mt) {
        const E* tile = pv + (int64_t)(mt0 + mt) * TMR * D;
#pragma unroll
        for (int i = 0; i < NPIECE / 4; ++i) {
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (mt & 1) * (A_ELEMS * (int)sizeof(E)) + (wave_u + 4 * i) * 1024);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"((glb_ptr)(tile + a_off[i])), "s"(dst)
                         : "memory");
        }
        if (tid < TMR) {
            int row = (mt0 + mt) * TMR + tid;
            rinv = inv[row < S ? row : S - 1];
        }
    };
    auto stage_write = [&](int mt) {
        if (tid < TMR) sInv[(mt & 1) * TMR + tid] = rinv;
    };
    // end of a tile: the next tile's DMA has landed, every wave is done with this tile's buffers.  rinv is made opaque so
    // that the compiler settles its own load of it here and not in front of the next stage_load's DMA
    auto tile_done = [&]() {
        asm volatile("" : "+v"(rinv));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };

    // A-fragment addresses (bytes into a tile image) as base + immediate.  Fragment k of a tile is half i = k / KS32 (pivot
    // rows 16 i + n16) at k-step t = k % KS32: the 16-B piece 4 t + g of row r = 16 i + n16, stored at piece
    // (4 t + g) ^ ((r >> 1) & 7).  (r >> 1) & 7 == (n16 >> 1) & 7 for both halves, and 4 t + g = 8 (t >> 1) + (4 (t & 1) + g)
    // whose second term is below 8, so the XOR stays in the low three bits: two per-lane bases (t even / odd) and the
    // immediates (t >> 1) * 128 B, i * HALF_BYTES and, added once per tile, the buffer's A_BYTES.
    constexpr int ROW_BYTES = D * (int)sizeof(E);
    constexpr int HALF_BYTES = 16 * ROW_BYTES;
    constexpr int A_BYTES = A_ELEMS * (int)sizeof(E);
    // fragments in flight: the read of group k + RING - 1 is issued before the MFMAs of group k.  A group is TJ MFMAs of
    // 16 matrix-pipe clocks, so both forms read 128 clocks ahead, about the LDS round trip
    constexpr int RING = TJ == 4 ? 3 : 5;
    static_assert(TMR == 32 && sizeof(E) == 2, "two 16-row halves whose rows 16 i + n16 share (r >> 1) & 7; 8 elements per 16-B piece");
    static_assert(KS32 % 2 == 0, "k-steps pair up into groups of 8 pieces");
    static_assert((KS32 / 2 - 1) * 128 + HALF_BYTES + A_BYTES < 65536, "every fragment offset fits ds_read's 16-bit immediate");
    static_assert(RING - 1 <= KS32, "the ring's prologue stays inside phase A");
    const int fa_base[2] = {n16 * ROW_BYTES + ((g ^ ((n16 >> 1) & 7)) << 4), n16 * ROW_BYTES + (((4 + g) ^ ((n16 >> 1) & 7)) << 4)};
    auto frag = [&](const int (&cur)[2], int k) {
        const int t = k % KS32, i = k / KS32;
        return __builtin_bit_cast(vec8, ld16(smem + cur[t & 1] + (t >> 1) * 128 + i * HALF_BYTES));
    };

    float best_v[TJ];
    int best_i[TJ];
#pragma unroll
    for (int j = 0; j < TJ; ++j) best_v[j] = -INFINITY, best_i[j] = 0;
    stage_load(0);
    stage_write(0);
    // the B fragments are complete here, not at their first use inside the loop: a vmcnt placed there by the compiler would
    // also wait for the DMA of the tile in flight
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int t = 0; t < KS32; ++t) asm volatile("" : "+v"(fb[j][t]));
    // likewise the output pointers: a scalar load pending beside the fragment reads makes the first wait of every tile
    // lgkmcnt(0)
    asm volatile("" ::"s"(idx_out), "s"(part_out));
    tile_done();
    // Half-tile phases.  A tile is 2 KS32 groups of TJ MFMAs on one A fragment each.  Phase A: the KS32 groups of pivot rows
    // 0-15 into acc0, beside them the fold of the PREVIOUS tile's rows 16-31 (acc1, w1 and row1 are carried over the barrier;
    // sInv's buffer of tile mt is overwritten by stage_write(mt + 2), so w1 is in registers before the barrier of tile mt,
    // and row1 names the tile the half belongs to, not the one its fold runs in).  Phase B: rows 16-31 into acc1, beside
    // them the fold of acc0.  Per accumulator the MFMA sequence is t ascending as before: every score keeps its bits.
    // Within a lane the folds stay in ascending pivot order (tile m rows 0-15, tile m rows 16-31, tile m + 1 rows 0-15, ..):
    // with the strict '>' the first index wins.  The fragment reads run as a ring RING - 1 groups ahead of the MFMAs and
    // drain at the end of the tile: the next tile's first reads stand behind the barrier, before which its DMA is not
    // known to have landed.
    constexpr int EPG = TJ / 2;              // scores folded beside one group: 4 TJ per half-tile over the groups 1 .. 8
    static_assert(TJ % 2 == 0 && EPG * (KS32 - 2) >= 4 * TJ, "a half-tile's fold fits beside the inner groups of a phase");
    // element e of a half-tile's fold: row e / TJ of this lane's four, sub-tile e % TJ -- ascending rows per sub-tile
    auto fold1 = [&](const f32x4 (&a)[TJ], const f32x4 w, const int row0, int e) {
        const int r = e / TJ, j = e % TJ;
        // register-only arithmetic is held in its group by making the running best opaque before and after it
        asm volatile("" : "+v"(best_v[j]), "+v"(best_i[j]));
        const float sc = a[j][r] * w[r];
        if (sc > best_v[j]) {
            best_v[j] = sc;
            best_i[j] = row0 + r;
        }
        asm volatile("" : "+v"(best_v[j]), "+v"(best_i[j]));
    };
    f32x4 acc0[TJ], acc1[TJ];
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc1[j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};   // folds to nothing (strict '>')
    f32x4 w0, w1 = f32x4{1.f, 1.f, 1.f, 1.f};
    int row0, row1 = 0;
    vec8 fa[RING];
    int cur[2];
    // group k of a tile: its read-ahead, its TJ MFMAs into acc (C = 0 at the first k-step), EPG scores of accf folded beside
    // them -- {read, TJ x {MFMA, 2 VALU}}, pinned
    auto group = [&](int k, f32x4 (&acc)[TJ], const f32x4 (&accf)[TJ], const f32x4 wf, const int rowf) {
        const int t = k % KS32;
        const bool read = k + RING - 1 < 2 * KS32;
        if (read) fa[(k + RING - 1) % RING] = frag(cur, k + RING - 1);
#pragma unroll
        for (int j = 0; j < TJ; ++j)
            acc[j] = T::mfma16(fa[k % RING], fb[j][t], t == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[j]);
        if (t >= 1 && t <= (4 * TJ) / EPG) {
#pragma unroll
            for (int e = (t - 1) * EPG; e < t * EPG; ++e) fold1(accf, wf, rowf, e);
        }
        if (read) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    for (int mt = 0; mt < n_mt; ++mt) {
        const bool has_next = mt + 1 < n_mt;
        const int buf = (mt & 1) * A_BYTES;
        cur[0] = fa_base[0] + buf, cur[1] = fa_base[1] + buf;
        const float* si = sInv + (mt & 1) * TMR + 4 * g;
#pragma unroll
        for (int k = 0; k < RING - 1; ++k) fa[k] = frag(cur, k);
        w0 = *reinterpret_cast<const f32x4*>(si);
        if (has_next) stage_load(mt + 1);
        row0 = (mt0 + mt) * TMR + 4 * g;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < KS32; ++k) group(k, acc0, acc1, w1, row1);
        w1 = *reinterpret_cast<const f32x4*>(si + 16);
#pragma unroll
        for (int k = KS32; k < 2 * KS32; ++k) group(k, acc1, acc0, w0, row0);
        row1 = row0 + 16;
        if (has_next) stage_write(mt + 1);
        tile_done();
    }
#pragma unroll
    for (int e = 0; e < 4 * TJ; ++e) fold1(acc1, w1, row1, e);   // rows 16-31 of the last tile
    // the four 16-lane rows hold disjoint pivot rows of the same target: merge, lower index on equal scores
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
        float bv = best_v[j];
        int bi = best_i[j];
#pragma unroll
        for (int o_ = 16; o_ <= 32; o_ <<= 1) {
            const float ov = __shfl_xor(bv, o_);
            const int oi = __shfl_xor(bi, o_);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        bi = bi < S ? bi : S - 1;
        if (g == 0 && t_row[j] < t_end) {
            if (part_out)
                part_out[((int64_t)blockIdx.z * gridDim.y + p) * n_tgt + t_row[j]] = NnPartial{bv, bi};
            else
                idx_out[(int64_t)p * n_tgt + t_row[j]] = bi;
        }
    }
}

// merge the per-split candidates: ascending split order == ascending pivot index
__global__ __launch_bounds__(256) void nn_finalize_kernel(const NnPartial* __restrict__ part,
                                                          int32_t* __restrict__ idx_out, int64_t total, int splits) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    NnPartial b = part[g];
    for (int s = 1; s < splits; ++s) {
        const NnPartial c = part[(int64_t)s * total + g];
        if (c.v > b.v || (c.v == b.v && c.i < b.i)) b = c;
    }
    idx_out[g] = b.i;
}

// ---- the kernel forms ---------------------------------------------------------------------------
// One description per form: targets per panel (tn), pivots per tile (tm), threads, dynamic LDS bytes, the name in the
// plan token, whether D is a kernel argument (d_arg; the register-B family has it as a template parameter), whether
// the launcher raises the kernel's dynamic-LDS limit first (lds_attr: the forms that can pass the default 64 KiB) and
// the kernel itself for an element type T and a chunk descriptor CHT (NnChunks / NnRagged).  The plan and the launcher
// read a form's geometry from here and nowhere else.
template <int WN, int BK, int TM>
struct NnGeneric {
    static constexpr int tn = 64 * WN, tm = TM, threads = 256;
    static constexpr size_t lds = 2 * (TM + tn) * BK * 2 + 2 * TM * 4 + 2 * tn * 8;
    static constexpr bool d_arg = true, lds_attr = true;
    template <typename T, typename CHT>
    static constexpr auto kernel() { return nn_search_kernel<T, WN, BK, TM, CHT>; }
};
struct NnWide : NnGeneric<2, 64, 128> { static constexpr const char* name = "wide"; };
struct NnDeep : NnGeneric<1, 256, 64> { static constexpr const char* name = "deep"; };
struct NnBk128 : NnGeneric<1, 128, 128> { static constexpr const char* name = "bk128"; };
struct NnBk64 : NnGeneric<1, 64, 128> { static constexpr const char* name = "bk64"; };
struct NnGlds {
    static constexpr int tn = 256, tm = 256, threads = 512;
    static constexpr size_t lds = 2 * (tm + tn) * 64 * 2 + 2 * tm * 4 + 4 * tn * 8;
    static constexpr bool d_arg = true, lds_attr = true;
    static constexpr const char* name = "glds";
    template <typename T, typename CHT>
    static constexpr auto kernel() {
#ifndef TF_TUNE_NN_NO_GLDS_SH   // A/B switch of tools/build_variants.sh
        return nn_search_glds_kernel<T, true, CHT>;    // short MFMAs (round 6, last session)
#else
        return nn_search_glds_kernel<T, false, CHT>;
#endif
    }
};
// the register-B family (D = 16 * DK = 320): 32-pivot tiles in LDS rows of D + PAD elements
template <int PAD>
struct NnRbFamily {
    static constexpr int DK = 20, tm = 32, threads = 256;
    static constexpr size_t lds = 2 * tm * (16 * DK + PAD) * 2 + 2 * tm * 4;
    static constexpr bool d_arg = false, lds_attr = false;   // 42 KiB of LDS
};
struct NnRb : NnRbFamily<8> {   // pivot tiles staged through registers
    static constexpr int tn = 128;
    static constexpr const char* name = "rb";
    template <typename T, typename CHT>
    static constexpr auto kernel() { return nn_search_rb_kernel<T, DK, CHT>; }
};
template <int TJ>
struct NnRbs : NnRbFamily<0> {   // pivot tiles by LDS-DMA, short MFMAs (16x16x32), TJ target tiles per wave
    static constexpr int tn = 64 * TJ;
    static constexpr const char* name = TJ == 4 ? "rbs<TJ=4>" : "rbs<TJ=2>";
    template <typename T, typename CHT>
    static constexpr auto kernel() { return nn_search_rbs_kernel<T, DK, TJ, CHT>; }
};
template <int TT>
struct NnRbg : NnRbFamily<0> {   // pivot tiles by LDS-DMA, 32x32x16 MFMAs, TT target tiles per wave
    static constexpr int tn = 128 * TT;
    static constexpr const char* name = TT == 2 ? "rbg<TT=2>" : "rbg<TT=1>";
    template <typename T, typename CHT>
    static constexpr auto kernel() { return nn_search_rbg_kernel<T, DK, TT, CHT>; }
};
// The LDS-DMA members of the family, 128- and 256-target panels.  A/B switch of tools/build_variants.sh: rbg in the
// place of rbs.
#ifndef TF_TUNE_NN_NO_RBS
typedef NnRbs<2> NnRbDma;
typedef NnRbs<4> NnRb2Dma;
// (the NnChunks instantiations of rbg have been part of this build all along, launched or not; they stay in it until
// the form is retired)
__attribute__((used)) const void* const nn_rbg_kept[] = {
    (const void*)NnRbg<1>::kernel<BF16, NnChunks>(), (const void*)NnRbg<1>::kernel<F16, NnChunks>(),
    (const void*)NnRbg<2>::kernel<BF16, NnChunks>(), (const void*)NnRbg<2>::kernel<F16, NnChunks>()};
#else
typedef NnRbg<1> NnRbDma;
typedef NnRbg<2> NnRb2Dma;
#endif

// "read an int from the environment, else a default" (unset or not positive: the default).  The callers keep the result
// in a function-local static, so every variable is read once per process.
static int env_int(const char* name, int def) {
    const char* e = getenv(name);
    return e && atoi(e) > 0 ? atoi(e) : def;
}
// TF_NN_RB_GLDS=0: the register-B family never stages its pivot tiles by LDS-DMA
static bool nn_rb_dma() {
    static const bool on = [] { const char* e = getenv("TF_NN_RB_GLDS"); return !e || atoi(e) != 0; }();
    return on;
}

// Launch plan shared by the launchers and tf_nn_search_workspace_bytes.
enum NnKernel {
    NN_RB,      // register-B kernel (D == 320): 128-target panels, 32-pivot tiles
    NN_RB2,     // the same with two target tiles per wave (256-target panels): chip-filling grids, S % 32 == 0
    NN_WIDE,    // generic kernel, 128-target panels, 64-wide D chunks
    NN_BK64,    // generic kernel, 64-target panels, 64-wide D chunks
    NN_BK128,   // few workgroups and a long contraction: 128-wide D chunks
    NN_DEEP,    // fewer still, D >= 1024: 64-pivot tiles and 256-wide D chunks (a quarter of the barrier intervals)
    NN_GLDS     // D % 64 == 0, D >= 512, chip-filling grids: 256 x 256 workgroup tiles staged by LDS-DMA
};
struct NnPlan {
    int kern;
    int tn, tm;   // targets per panel / pivots per tile of the form
    int64_t panels;
    int splits, tiles_per_split;
};

// The form a plan launches, handed to `f` as a value of its description type.  The one place that resolves the
// register-B family: NN_RB2 is the 256-target LDS-DMA member (the plan has checked S % 32 == 0); NN_RB is the
// 128-target one where every pivot tile is full (S % 32 == 0: +1.4 % at cfg2 / cfg4 level 0,
// profiles/r05_nn_glds_ab.txt: 1028 -> 1014 us, 8826 -> 8746 us per block), else the register-staged kernel.
template <typename Fn>
int nn_with_form(const NnPlan& pl, int S, Fn&& f) {
    switch (pl.kern) {
        case NN_RB2: return f(NnRb2Dma{});
        case NN_RB: return nn_rb_dma() && S % 32 == 0 ? f(NnRbDma{}) : f(NnRb{});
        case NN_GLDS: return f(NnGlds{});
        case NN_WIDE: return f(NnWide{});
        case NN_DEEP: return f(NnDeep{});
        case NN_BK128: return f(NnBk128{});
        default: return f(NnBk64{});
    }
}

// Grid target of the pivot-range split: workgroups the launch should have at least.  1024 = 4 per CU for one chunk.
// A multi-chunk launch is C times larger; it keeps splitting up to TF_NN_MIN_WGS (environment; default 4096) so that
// the last round of workgroups is a small fraction of the launch.
static int nn_min_wgs(int C) {
    static const int env = env_int("TF_NN_MIN_WGS", 4096);
    return C > 1 ? env : 1024;
}

// The pivot-range split of a plan whose form (kern, tn, tm) is set: `wgs` = workgroups of the launch before splitting
// (target panels of all chunks x keyframes).  Returns the workgroups of the split launch.
static int64_t nn_split(NnPlan& pl, int64_t wgs, int S, int C) {
    const int n_tiles = (S + pl.tm - 1) / pl.tm;
    int splits = 1;
    if (pl.kern == NN_GLDS) {
        // one workgroup per CU, aim at >= `rounds` rounds of workgroups (tail), never below one tile per split
        static const int rounds = env_int("TF_NN_GLDS_ROUNDS", 3);
        while (wgs * splits < rounds * 256 && splits * 2 <= n_tiles) splits *= 2;
    } else {
        // a multi-chunk launch keeps >= 128 pivots per split: below that the per-workgroup fixed cost (target
        // fragments, partial results, their merge) outweighs the finer tail (cfg1 level 0: 41.8 us at 128 pivots /
        // split, 72 us at 32)
        const int min_tiles = C > 1 ? (128 + pl.tm - 1) / pl.tm : 1;
        while (wgs * splits < nn_min_wgs(C) && splits * 2 <= n_tiles && n_tiles / (splits * 2) >= min_tiles)
            splits *= 2;
    }
    pl.tiles_per_split = (n_tiles + splits - 1) / splits;
    pl.splits = (n_tiles + pl.tiles_per_split - 1) / pl.tiles_per_split;
    return wgs * pl.splits;
}

// splits of the pivot range so that the grid has >= nn_min_wgs workgroups while every split keeps >= 1 tile.
// n_tgt = targets of ONE chunk, C = chunks in the launch (grid.x = C * panels).
static NnPlan nn_plan(int64_t n_tgt, int S, int D, int P, int C = 1) {
    NnPlan pl;
    auto shape = [&](int kern, auto form) {   // the plan with this form; returns the workgroups of the launch
        pl.kern = kern, pl.tn = form.tn, pl.tm = form.tm;
        pl.panels = (n_tgt + pl.tn - 1) / pl.tn;
        return nn_split(pl, pl.panels * C * P, S, C);
    };
#ifndef TF_TUNE_NN_NO_GLDS   // A/B switch of tools/build_variants.sh
    // LDS-DMA kernel (256-target panels, 256-pivot tiles, one 8-wave workgroup per CU): where the launch still has
    // >= TF_NN_GLDS_MIN_WGS workgroups after splitting the pivot range down to one tile per workgroup
    static const int glds_min_d = env_int("TF_NN_GLDS_MIN_D", 512);
    // D = 320 keeps the register-B kernel at the large levels (1.00 vs 1.12 ms at cfg2 level 0); with <= 1024 pivots per
    // keyframe (BASELINE config 1, level 0) its 32-pivot tiles are mostly prologue: 44 -> 33 us (profiles/r05_nn_glds_ab.txt)
    if (D % 64 == 0 && (D >= glds_min_d || (D == 320 && S <= 1024)) && S % 4 == 0) {
        static const int min_wgs = env_int("TF_NN_GLDS_MIN_WGS", 160);
        const int64_t panels = (n_tgt + NnGlds::tn - 1) / NnGlds::tn;
        const int n_tiles = (S + NnGlds::tm - 1) / NnGlds::tm;
        if (panels * C * P * n_tiles >= min_wgs) {
            shape(NN_GLDS, NnGlds{});
            return pl;
        }
    }
#endif
    if (D == 16 * NnRb::DK) {
#ifndef TF_TUNE_NN_NO_RB2
        // two target tiles per wave where the launch still has >= 2 rounds of its 512 resident workgroups (2 per CU) AND a
        // workgroup streams >= 24 pivot tiles: its 160 VGPRs of target fragments are a fixed cost per workgroup (one chunk of
        // cfg5, 32 tiles per workgroup: 196 -> 163 us; one chunk of cfg2, 16 tiles: 123 -> 125 us, profiles/r06_nn_rb2_ab.txt)
        static const int rb2_min = env_int("TF_NN_RB2_MIN_WGS", 1024);
        if (nn_rb_dma() && S % 32 == 0 && shape(NN_RB2, NnRb2Dma{}) >= rb2_min && pl.tiles_per_split >= 24) return pl;
#endif
        shape(NN_RB, NnRb{});
        return pl;
    }
    // 128-target panels halve the pivot re-reads; they pay as soon as the grid still fills the GPU after
    // splitting the pivot range (measured at cfg2 level 1, 5120 targets x 2 keyframes: 34.6 vs 39.8 us)
    if (((n_tgt + NnWide::tn - 1) / NnWide::tn) * P * C >= 64) {
        shape(NN_WIDE, NnWide{});
        return pl;
    }
    // few workgroups and a long contraction: the loop is a chain of load -> LDS -> barrier -> MFMA steps whose
    // latency nothing hides -> wider D chunks (fewer steps)
#ifndef TF_TUNE_NN_NO_DEEP   // A/B switch of tools/build_variants.sh
    if (D >= 1024 && shape(NN_DEEP, NnDeep{}) <= 512) return pl;
#endif
    if (shape(NN_BK128, NnBk128{}) > 512 || D < 512) shape(NN_BK64, NnBk64{});
    return pl;
}

// the targets of a ragged call
static int64_t nn_ragged_rows(const int* frames, int C, int S) {
    int64_t rows = 0;
    for (int j = 0; j < C; ++j) rows += (int64_t)frames[j] * S;
    return rows;
}

// A RAGGED launch: C chunks of frames[j] * S targets, two keyframes (the p = 1 half of a one-keyframe chunk exits at once).
// The rule (host only, a function of the frame counts, S and D):
//   - the kernel FORM is the one the uniform C-chunk launch takes at the MEAN chunk size, ceil(sum_j frames[j] * S / C)
//     targets per chunk: nn_plan(mean, S, D, 2, C).kern;
//   - grid.x = sum_j ceil(frames[j] * S / TN) panels of that form (a chunk's last panel is partial, none straddles two
//     chunks), and the pivot-range split is the form's own rule applied to THAT workgroup count.
// pl.panels = grid.x.  Equal frame counts never come here: the entry points hand them to the uniform launch.
static NnPlan nn_plan_ragged(const int* frames, int C, int S, int D) {
    NnPlan pl = nn_plan((nn_ragged_rows(frames, C, S) + C - 1) / C, S, D, 2, C);
    pl.panels = 0;
    for (int j = 0; j < C; ++j) pl.panels += ((int64_t)frames[j] * S + pl.tn - 1) / pl.tn;
    nn_split(pl, pl.panels * 2, S, C);
    return pl;
}

static int finalize(const NnPartial* part, int32_t* idx, int64_t total, int splits, hipStream_t st) {
    if (tf_plan_note("finalize")) return 0;
    hipLaunchKernelGGL(nn_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, idx, total,
                       splits);
    TF_LAUNCH_CHECK("tf_nn_search(finalize)");
    return 0;
}

// One search launch.  total = targets of all chunks of the call (partial results / indices are laid out over them);
// fin: indices are wanted, so a split launch is followed by the finalize launch (never a ragged one: the gather merges).
struct NnLaunch {
    const void *tgt, *piv;
    const float* inv_norm;
    int32_t* idx;
    NnPartial* ws;
    int64_t total;
    int S, D, P, kf0, kf1;
    hipStream_t st;
    bool fin;
    NnPlan pl;
    unsigned grid_x;       // target panels of all chunks
    const char* suffix;    // of the plan token: "" / ",chunks" / ",ragged"
    const char* label;     // of a failed launch
};

template <typename T, typename CHT>
int nn_launch_as(const NnLaunch& a, const CHT& ch) {
    typedef const typename T::elem* EP;
    const int splits = a.pl.splits;
    const int rc = nn_with_form(a.pl, a.S, [&](auto form) {
        typedef decltype(form) F;
        static_assert(F::lds <= 160 * 1024, "LDS");
        if (tf_plan_note("%s[splits=%d%s]", F::name, splits, a.suffix)) return 0;
        auto kern = F::template kernel<T, CHT>();
        const dim3 grid(a.grid_x, (unsigned)a.P, (unsigned)splits);
        NnPartial* const ws = (splits > 1 || !a.fin) ? a.ws : nullptr;
        if constexpr (F::lds_attr)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)F::lds);
        if constexpr (F::d_arg) {
            hipLaunchKernelGGL(kern, grid, dim3(F::threads), F::lds, a.st, (EP)a.tgt, (EP)a.piv, a.inv_norm, a.idx, ws, a.total,
                               a.S, a.D, a.kf0, a.kf1, a.pl.tiles_per_split, ch);
        } else {
            hipLaunchKernelGGL(kern, grid, dim3(F::threads), F::lds, a.st, (EP)a.tgt, (EP)a.piv, a.inv_norm, a.idx, ws, a.total,
                               a.S, a.kf0, a.kf1, a.pl.tiles_per_split, ch);
        }
        TF_LAUNCH_CHECK(a.label);
        return 0;
    });
    return (rc == 0 && a.fin && splits > 1) ? finalize(a.ws, a.idx, a.total * a.P, splits, a.st) : rc;
}
template <typename CHT>
int nn_launch(int dtype, const NnLaunch& a, const CHT& ch) {
    return dtype == TF_BF16 ? nn_launch_as<BF16>(a, ch) : nn_launch_as<F16>(a, ch);
}

// The uniform call: C chunks of n_tgt targets each (C = 1, single_mask = 0: the plain single-chunk search), `pl` their plan.
int nn_search_chunks(const void* tgt, const void* piv, const float* inv_norm, int32_t* idx, NnPartial* ws, int64_t n_tgt, int S,
                     int D, int P, int kf0, int kf1, int dtype, hipStream_t st, bool fin, int C, uint64_t single_mask,
                     const NnPlan& pl) {
    // the chunk descriptor of a launch carries the targets per chunk in 32 bits (NnChunks)
    TF_ARG(n_tgt <= (int64_t)INT32_MAX, TF_ERR_SHAPE, "tf_nn_search: %lld targets per chunk (< 2^31)", (long long)n_tgt);
    const NnLaunch a{tgt, piv, inv_norm, idx, ws, n_tgt * C, S, D, P, kf0, kf1, st, fin, pl, (unsigned)(pl.panels * C),
                     C > 1 ? ",chunks" : "", "tf_nn_search"};
    return nn_launch(dtype, a, nn_chunks(n_tgt, (int)pl.panels, single_mask));
}

size_t nn_partials_bytes(const NnPlan& pl, int64_t targets, int P) { return (size_t)pl.splits * P * targets * sizeof(NnPartial); }

}  // namespace

// The ragged call (nn_plan_ragged): the NnRagged instantiation of the form's kernel, partial results only, P = 2.  Plan
// tokens are the uniform launch's with ",ragged" in the place of ",chunks".
int tf_nn_search_partials_ragged(const void* tgt, const void* piv, const float* inv_norm, NnPartial* part,
                                 const int* frames, int C, int S, int D, int kf0, int kf1, int dtype, hipStream_t st,
                                 int* splits, uint64_t single_mask) {
    const NnPlan pl = nn_plan_ragged(frames, C, S, D);
    *splits = pl.splits;
    const NnLaunch a{tgt, piv, inv_norm, nullptr, part, nn_ragged_rows(frames, C, S), S, D, 2, kf0, kf1, st, false, pl,
                     (unsigned)pl.panels, ",ragged", "tf_nn_search(ragged)"};
    return nn_launch(dtype, a, nn_ragged(frames, C, S, pl.tn, single_mask));
}

size_t tf_nn_partials_bytes_ragged(const int* frames, int C, int S, int D) {
    return nn_partials_bytes(nn_plan_ragged(frames, C, S, D), nn_ragged_rows(frames, C, S), 2);
}

extern "C" int tf_pivot_inv_norm(const void* piv, float* inv_norm, int64_t rows, int D, int dtype, void* stream) {
    TF_ARG(piv && inv_norm, TF_ERR_NULL, "tf_pivot_inv_norm: null pointer");
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "tf_pivot_inv_norm: dtype %d (bf16/f16 only)", dtype);
    TF_ARG(rows > 0 && D > 0 && D % 8 == 0, TF_ERR_SHAPE, "tf_pivot_inv_norm: rows=%lld D=%d (D %% 8 == 0)",
           (long long)rows, D);
    TF_ARG(tf_aligned16(piv), TF_ERR_ALIGN, "tf_pivot_inv_norm: piv not 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)((rows + 3) / 4 < 4096 ? (rows + 3) / 4 : 4096);
    if (dtype == TF_BF16)
        hipLaunchKernelGGL(pivot_inv_norm_kernel<BF16>, dim3(grid), dim3(256), 0, st,
                           reinterpret_cast<const __bf16*>(piv), inv_norm, rows, D);
    else
        hipLaunchKernelGGL(pivot_inv_norm_kernel<F16>, dim3(grid), dim3(256), 0, st,
                           reinterpret_cast<const _Float16*>(piv), inv_norm, rows, D);
    TF_LAUNCH_CHECK("tf_pivot_inv_norm");
    return 0;
}

// Launch plan of tf_nn_search (C = 1) or of the search launches of tf_nn_gather_blend_chunks (C > 1, P = 2): the real
// launch path under the plan recorder (csrc/tf_common.h).  No device, no allocation.
extern "C" int tf_nn_search_plan(int64_t n_tgt, int S, int D, int P, int C, char* buf, size_t len) {
    TF_ARG(n_tgt > 0 && S > 0 && D > 0 && D % 8 == 0 && (P == 1 || P == 2) && C >= 1 && (C == 1 || P == 2), TF_ERR_SHAPE,
           "tf_nn_search_plan: n_tgt=%lld S=%d D=%d P=%d C=%d", (long long)n_tgt, S, D, P, C);
    return tf_record_plan("tf_nn_search_plan", buf, len, [&] {
        return nn_search_chunks(nullptr, nullptr, nullptr, nullptr, nullptr, n_tgt, S, D, P, 0, 1, TF_BF16, nullptr, C == 1, C, 0,
                                nn_plan(n_tgt, S, D, P, C));
    });
}

// scratch of tf_nn_search under plan `pl`; never 0: the caller always passes a valid pointer
static size_t nn_search_ws_bytes(const NnPlan& pl, int64_t n_tgt, int P) {
    const size_t bytes = pl.splits > 1 ? nn_partials_bytes(pl, n_tgt, P) : 0;
    return bytes < 256 ? 256 : bytes;
}
extern "C" size_t tf_nn_search_workspace_bytes(int64_t n_tgt, int S, int D, int P) {
    if (n_tgt <= 0 || S <= 0 || D <= 0 || P <= 0) return 0;
    return nn_search_ws_bytes(nn_plan(n_tgt, S, D, P), n_tgt, P);
}

extern "C" int tf_nn_search(const void* tgt, const void* piv, const float* inv_norm, int32_t* idx, int64_t n_tgt,
                            int S, int D, int P, int kf0, int kf1, int dtype, void* ws, size_t ws_bytes,
                            void* stream) {
    TF_ARG(tgt && piv && inv_norm && idx && ws, TF_ERR_NULL, "tf_nn_search: null pointer");
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "tf_nn_search: dtype %d (bf16/f16 only)", dtype);
    TF_ARG(n_tgt > 0 && S > 0 && D > 0 && D % 8 == 0 && (P == 1 || P == 2) && kf0 >= 0 && (P == 1 || kf1 >= 0),
           TF_ERR_SHAPE, "tf_nn_search: n_tgt=%lld S=%d D=%d P=%d kf=(%d,%d)", (long long)n_tgt, S, D, P, kf0, kf1);
    TF_ARG(tf_aligned16(tgt) && tf_aligned16(piv) && tf_aligned16(ws) && tf_aligned16(inv_norm), TF_ERR_ALIGN,
           "tf_nn_search: inputs not 16-byte aligned (inv_norm included: the LDS-DMA kernel fetches it in 16-byte pieces)");
    const NnPlan pl = nn_plan(n_tgt, S, D, P);
    TF_ARG(ws_bytes >= nn_search_ws_bytes(pl, n_tgt, P), TF_ERR_WORKSPACE, "tf_nn_search: workspace %zu < %zu bytes", ws_bytes,
           nn_search_ws_bytes(pl, n_tgt, P));
    return nn_search_chunks(tgt, piv, inv_norm, idx, reinterpret_cast<NnPartial*>(ws), n_tgt, S, D, P, kf0, kf1, dtype,
                            reinterpret_cast<hipStream_t>(stream), true, 1, 0, pl);
}

int tf_nn_search_partials(const void* tgt, const void* piv, const float* inv_norm, NnPartial* part, int64_t n_tgt,
                          int S, int D, int P, int kf0, int kf1, int dtype, hipStream_t st, int* splits, int C,
                          uint64_t single_mask) {
    const NnPlan pl = nn_plan(n_tgt, S, D, P, C);
    *splits = pl.splits;
    return nn_search_chunks(tgt, piv, inv_norm, nullptr, part, n_tgt, S, D, P, kf0, kf1, dtype, st, false, C, single_mask, pl);
}

size_t tf_nn_partials_bytes(int64_t n_tgt, int S, int D, int P, int C) {
    return nn_partials_bytes(nn_plan(n_tgt, S, D, P, C), n_tgt * C, P);
}
