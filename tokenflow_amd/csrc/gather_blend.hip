// Token gather + two-keyframe blend + residual add, and the PnP feature-injection copy.
// Replaces tokenflow_utils.py:362-397 and 87-91 of omerbt/TokenFlow.
//
// HBM-bound: each output row (D elements, 640 B .. 2.5 KB) is a contiguous row of one
// keyframe's cached attention output, so a row gather is naturally coalesced.  One
// thread owns one 8-element piece of one token and loops the 3 branches, re-using the
// token's two int32 indices and the frame's weight; 16-byte loads/stores; fp32 math
// with the reference's operation order and NO fma contraction, so fp32 results are
// bit-identical to torch's  w1*a1 + (1-w1)*a2  (+ hidden_states).
#include "ln_row.h"
#include "tf_common.h"

// bit-exactness vs torch needs separately rounded multiplies and adds: no fma contraction here
#pragma clang fp contract(off)

namespace {

template <typename T>
struct Vec8 {  // 8 elements of T as raw 16-byte words
    static constexpr int WORDS = sizeof(T) * 8 / 16;
    u32x4 w[WORDS];
};

template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&f)[8]) {
    if constexpr (sizeof(T) == 4) {
        const u32x4 a = ld16(p), b = ld16(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[i] = __uint_as_float(a[i]);
            f[4 + i] = __uint_as_float(b[i]);
        }
    } else {
        typedef T v8 __attribute__((ext_vector_type(8)));
        const v8 v = __builtin_bit_cast(v8, ld16(p));
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = (float)v[i];
    }
}

template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&f)[8]) {
    if constexpr (sizeof(T) == 4) {
        u32x4 a, b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] = __float_as_uint(f[i]);
            b[i] = __float_as_uint(f[4 + i]);
        }
        st16(p, a);
        st16(p + 4, b);
    } else {
        typedef T v8 __attribute__((ext_vector_type(8)));
        v8 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (T)f[i];  // round-to-nearest-even
        st16(p, __builtin_bit_cast(u32x4, v));
    }
}

// Streaming accesses of the kernel (residual in, result out) are touched exactly once: nontemporal, so that they
// do not push the keyframe rows -- every one of them gathered ~2 n times per block -- out of the L2
// (-2 % at cfg2 levels 0 and 1, profiles/r02_gather_order_ab.txt).
template <typename T>
__device__ __forceinline__ void load8_stream(const T* p, float (&f)[8]) {
    if constexpr (sizeof(T) == 4) {
        const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
        const u32x4 b = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + 4));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[i] = __uint_as_float(a[i]);
            f[4 + i] = __uint_as_float(b[i]);
        }
    } else {
        typedef T v8 __attribute__((ext_vector_type(8)));
        const v8 v = __builtin_bit_cast(v8, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)));
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = (float)v[i];
    }
}

template <typename T>
__device__ __forceinline__ void store8_stream(T* p, const float (&f)[8]) {
    if constexpr (sizeof(T) == 4) {
        u32x4 a, b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] = __float_as_uint(f[i]);
            b[i] = __float_as_uint(f[4 + i]);
        }
        __builtin_nontemporal_store(a, reinterpret_cast<u32x4*>(p));
        __builtin_nontemporal_store(b, reinterpret_cast<u32x4*>(p + 4));
    } else {
        typedef T v8 __attribute__((ext_vector_type(8)));
        v8 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (T)f[i];  // round-to-nearest-even
        __builtin_nontemporal_store(__builtin_bit_cast(u32x4, v), reinterpret_cast<u32x4*>(p));
    }
}

struct NoRes {};

// Multi-chunk call (tf_nn_gather_blend_chunks): `n` frames are C chunks of nc frames; chunk j = frame / nc gathers
// from keyframe slots kf0 + j and kf1 + j.  When the first chunk of the call is chunk 0 of the video it has ONE
// keyframe (tokenflow_utils.py:331-333, 390): its rows are a1 + residual, rounded to the dtype the reference's
// single-keyframe pass would produce (`single_dtype`: torch promotion of the cached output and hidden_states)
// before they are widened to the call's output type -- so the call reproduces C separate calls bit for bit.
struct GbChunks {
    int nc;             // frames per chunk (0: not a multi-chunk call)
    int single_dtype;   // TF_BF16 / TF_F16 / TF_F32
    uint64_t single_mask;   // bit j: chunk j of the call has one keyframe (chunks at or above 64: never)
};
__device__ __forceinline__ bool gb_chunk_single(const GbChunks& ch, int j) { return j < 64 && ((ch.single_mask >> j) & 1); }
// chunk of a token; `frame` (of the whole call) becomes the frame inside the chunk, the index of the chunk's weight
__device__ __forceinline__ int gb_chunk_of(const GbChunks& ch, int64_t, int& frame) {
    const int j = frame / ch.nc;
    frame -= j * ch.nc;
    return j;
}

// Ragged call (tf_nn_gather_blend_chunks_ragged): C <= 64 chunks of unequal frame count.  A token's chunk is found in the
// target prefix table of the launch (tf_common.h, NnRagged) -- a per-thread bisection whose six reads are vector loads from
// the kernel-argument segment: no private array, no device table to copy in.  `w` holds one weight per frame of the CALL
// (the caller concatenates the weights of every chunk size), so the frame index stays global.
struct GbRagged {
    int single_dtype;
    uint64_t single_mask;
    int row0[TF_RAGGED_MAX_CHUNKS + 1];
};
__device__ __forceinline__ bool gb_chunk_single(const GbRagged& ch, int j) { return (ch.single_mask >> j) & 1; }
__device__ __forceinline__ int gb_chunk_of(const GbRagged& ch, int64_t t, int&) { return tf_ragged_find(ch.row0, (int)t); }

// MERGE: the indices come as the search's per-split partial results (tf_nn_gather_blend: no finalize launch
// in between); every thread of a token merges them itself -- `splits` 8-byte reads, broadcast from cache.
// CH: multi-chunk call (P == 2, MERGE).
// DYN: the number of branches is the argument `nb` (multi-edit batches, [source | uncond_1 | cond_1 | ... ]: the *_edits
// entry points) instead of the constant 3; the arithmetic of a branch is the same code, so branch b of a DYN launch is
// bit-identical to branch b of the 3-branch launch on the same tensors.
// CHT: the chunk descriptor of a CH launch, GbChunks (equal chunks) or GbRagged.
template <typename TIn, typename TRes, typename TOut, int P, bool MERGE, bool CH = false, bool DYN = false,
          typename CHT = GbChunks>
__global__ __launch_bounds__(256) void gather_blend_kernel(const TIn* __restrict__ kf_out,
                                                           const int32_t* __restrict__ idx,
                                                           const NnPartial* __restrict__ part, int splits,
                                                           const float* __restrict__ w, const TRes* __restrict__ resid,
                                                           TOut* __restrict__ out, int K, int n, int S, int D, int kf0,
                                                           int kf1, CHT ch, int nb) {
    const int ppr = D >> 3;  // pieces per row
    const int64_t nS = (int64_t)n * S;
    const int64_t total = nS * ppr;
    const int64_t branch_in = (int64_t)K * S * D;
    const int64_t branch_out = nS * D;
    const int64_t frame_in = (int64_t)S * D;
    const TIn* src1 = kf_out + (int64_t)kf0 * frame_in;
    const TIn* src2 = kf_out + (int64_t)kf1 * frame_in;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t t = g / ppr;
        const int c = (int)(g - t * ppr) * 8;
        const int i1 = MERGE ? nn_merge_partials(part + t, P * nS, splits) : idx[t];
        float w1 = 0.f, w2 = 0.f;
        int i2 = 0;
        int frame = (int)(t / S);
        int64_t coff = 0;        // CH: offset of this chunk's keyframe pair from (kf0, kf1)
        bool single = false;     // CH: this token belongs to the one-keyframe chunk
        if constexpr (CH) {
            const int j = gb_chunk_of(ch, t, frame);
            coff = j * frame_in;
            single = gb_chunk_single(ch, j);
        }
        if constexpr (P == 2) {
            if (!single) i2 = MERGE ? nn_merge_partials(part + nS + t, P * nS, splits) : idx[nS + t];
            w1 = w[frame];
            w2 = __fsub_rn(1.0f, w1);
        }
        auto branch = [&](int b) {
            float a1[8], o[8];
            load8(src1 + coff + b * branch_in + (int64_t)i1 * D + c, a1);
            if (P == 2 && !single) {
                float a2[8];
                load8(src2 + coff + b * branch_in + (int64_t)i2 * D + c, a2);
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = __fadd_rn(__fmul_rn(w1, a1[i]), __fmul_rn(w2, a2[i]));
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = a1[i];
            }
            const int64_t off = b * branch_out + t * D + c;
            if constexpr (!__is_same(TRes, NoRes)) {
                float h[8];
                load8_stream(resid + off, h);
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = __fadd_rn(o[i], h[i]);
            }
            if constexpr (CH) {
                if (single && ch.single_dtype != TF_F32) {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        o[i] = ch.single_dtype == TF_BF16 ? (float)(__bf16)o[i] : (float)(_Float16)o[i];
                }
            }
            store8_stream(out + off, o);
        };
        if constexpr (DYN) {
            for (int b = 0; b < nb; ++b) branch(b);
        } else {
#pragma unroll
            for (int b = 0; b < 3; ++b) branch(b);
        }
    }
}

// The same gather + blend + residual with the block's NEXT LayerNorm fused behind it (norm2 / norm3 of
// TokenFlowBlock.forward, tokenflow_utils.py:399-414, whose only consumer is a Linear): the propagation pass leaves
// its residual stream in fp32 (the reference's promotion, 385-397), and a separate norm launch re-reads those 4 bytes
// per element only to emit 2.  Here a row of the result never leaves the registers between the two: LPR lanes own one
// (branch, token) row (the mapping and arithmetic of ln_row.h, LPR from ln_lanes_per_row as in tf_layer_norm, so the
// normalised rows are bit-identical to tf_layer_norm on the stored result at every D), write it once and write its norm
// in the 16-bit type the Linear reads.
// Always the MERGE form (indices from the search's partial results).  T16 = the 16-bit model type (cached attention
// output, residual, norm output); TOut = result type: float (two keyframes) or T16 (the one-keyframe chunk alone).
template <typename T16, typename TOut, int LPR, int NP, int P, bool CH, typename CHT = GbChunks>
__global__ __launch_bounds__(256) void gather_blend_norm_kernel(
    const T16* __restrict__ kf_out, const NnPartial* __restrict__ part, int splits, const float* __restrict__ w,
    const T16* __restrict__ resid, TOut* __restrict__ out, T16* __restrict__ norm_out, const void* __restrict__ gamma,
    const void* __restrict__ beta, int w_dtype, float eps, int K, int n, int S, int D, int kf0, int kf1, CHT ch,
    int nb) {
    constexpr int RPW = 64 / LPR;
    __shared__ __attribute__((aligned(16))) float sw[2][LPR * 8 * NP];
    ln_stage_weights<256>(sw[0], sw[1], gamma, beta, w_dtype, D);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int lr = lane % LPR;
    const int pieces = D >> 3;
    const float inv_d = 1.0f / (float)D;
    const int64_t nS = (int64_t)n * S;
    const int64_t rows = nb * nS;                   // row = b * nS + t  (branch-major, as the output tensor); nb = 3 branches,
                                                    // 1 + 2E in a multi-edit batch
    const int64_t branch_in = (int64_t)K * S * D;
    const int64_t frame_in = (int64_t)S * D;
    const T16* src1 = kf_out + (int64_t)kf0 * frame_in;
    const T16* src2 = kf_out + (int64_t)kf1 * frame_in;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
    for (int64_t r = row0; r < rows; r += (int64_t)gridDim.x * 4 * RPW) {
        const int b = (int)(r / nS);
        const int64_t t = r - b * nS;
        const int i1 = nn_merge_partials(part + t, P * nS, splits);
        float w1 = 0.f, w2 = 0.f;
        int i2 = 0;
        int frame = (int)(t / S);
        int64_t coff = 0;
        bool single = false;
        if constexpr (CH) {
            const int j = gb_chunk_of(ch, t, frame);
            coff = j * frame_in;
            single = gb_chunk_single(ch, j);
        }
        if constexpr (P == 2) {
            if (!single) i2 = nn_merge_partials(part + nS + t, P * nS, splits);
            w1 = w[frame];
            w2 = __fsub_rn(1.0f, w1);
        }
        const T16* r1 = src1 + coff + b * branch_in + (int64_t)i1 * D;
        const T16* r2 = src2 + coff + b * branch_in + (int64_t)i2 * D;
        float v[NP][8];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int p = lr + LPR * j;
            if (p < pieces) {
                float a1[8], h[8];
                load8(r1 + p * 8, a1);
                if (P == 2 && !single) {
                    float a2[8];
                    load8(r2 + p * 8, a2);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[j][i] = __fadd_rn(__fmul_rn(w1, a1[i]), __fmul_rn(w2, a2[i]));
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[j][i] = a1[i];
                }
                load8_stream(resid + r * D + p * 8, h);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[j][i] = __fadd_rn(v[j][i], h[i]);
                if constexpr (CH) {   // the one-keyframe chunk: rounded to the dtype its own pass produces
                    if (single && ch.single_dtype != TF_F32) {
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            v[j][i] = ch.single_dtype == TF_BF16 ? (float)(__bf16)v[j][i] : (float)(_Float16)v[j][i];
                    }
                }
                store8_stream(out + r * D + p * 8, v[j]);
                if constexpr (sizeof(TOut) == 2) {   // the norm sees the STORED (rounded) row
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[j][i] = (float)(TOut)v[j][i];
                }
            }
        }
        (void)ln_row_finish<LPR, NP, T16>(v, lr, pieces, inv_d, eps, sw[0], sw[1], norm_out + r * D);
    }
}

__global__ __launch_bounds__(256) void inject_copy_kernel(u32x4* __restrict__ x, int64_t pieces_per_branch) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < pieces_per_branch;
         g += (int64_t)gridDim.x * 256) {
        const u32x4 v = x[g];
        x[pieces_per_branch + g] = v;
        x[2 * pieces_per_branch + g] = v;
    }
}

// multi-edit batch: x[b] = x[0] for every branch b >= 1 of [source | uncond_1 | cond_1 | ... ]; MASKED: only for the branches
// whose bit is set in `branch_mask` (the edits that inject at this step), the others are neither read nor written
template <bool MASKED>
__global__ __launch_bounds__(256) void inject_copy_edits_kernel(u32x4* __restrict__ x, int64_t pieces_per_branch, int nb,
                                                                unsigned branch_mask) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < pieces_per_branch;
         g += (int64_t)gridDim.x * 256) {
        const u32x4 v = x[g];
        for (int b = 1; b < nb; ++b)
            if (!MASKED || ((branch_mask >> b) & 1u)) x[b * pieces_per_branch + g] = v;
    }
}

struct GbArgs {
    const void* kf_out;
    const int32_t* idx;
    const NnPartial* part;   // alternative to idx: partial results of `splits` pivot-range splits
    int splits;
    const float* w;
    const void* resid;
    void* out;
    int K, n, S, D, P, kf0, kf1;
    hipStream_t st;
    GbChunks ch;
    // fused norm (gather_blend_norm_kernel): norm_out != nullptr
    void* norm_out = nullptr;
    const void* gamma = nullptr;
    const void* beta = nullptr;
    int w_dtype = 0;
    float eps = 0.f;
    int nb = 3;         // branches; dyn: the *_edits entry points (branch count as a kernel argument)
    bool dyn = false;
    const GbRagged* rg = nullptr;   // ragged call: the descriptor in the place of `ch`
};
static const GbChunks& gb_desc(const GbArgs& a, const GbChunks*) { return a.ch; }
static const GbRagged& gb_desc(const GbArgs& a, const GbRagged*) { return *a.rg; }

// fused-norm form: T16 in / residual / norm out, result float (P = 2) or T16 (P = 1)
template <typename T16, typename TOut, int P, bool CH, typename CHT = GbChunks>
void launch_gbn(const GbArgs& a) {
    const int64_t rows = (int64_t)a.nb * a.n * a.S;
    auto go = [&](auto kern, int lpr) {
        const int rows_per_wg = 4 * (64 / lpr);
        int64_t blocks = (rows + rows_per_wg - 1) / rows_per_wg;
        if (blocks > 256 * 16) blocks = 256 * 16;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, a.st, (const T16*)a.kf_out, a.part, a.splits, a.w,
                           (const T16*)a.resid, (TOut*)a.out, (T16*)a.norm_out, a.gamma, a.beta, a.w_dtype, a.eps, a.K,
                           a.n, a.S, a.D, a.kf0, P == 2 ? a.kf1 : a.kf0, gb_desc(a, (const CHT*)nullptr), a.nb);
    };
    if (tf_plan_note(a.rg ? "gather_norm[branches=%d,ragged]" : "gather_norm[branches=%d]", a.nb)) return;
    // lanes per row as tf_layer_norm has them (ln_row.h): the norm's bits depend on it.  3 pieces per lane cover the
    // model's widths (D = 320 / 640 / 1280) and everything up to D = 384 / 768 / 1536 at 16 / 32 / 64 lanes; the widths
    // between (D <= 512 at 16 lanes, <= 1024 at 32) take the 4-piece instantiation
    const int pieces = a.D >> 3, lpr = ln_lanes_per_row(a.D);
    if (lpr == 16) {
        if (pieces <= 48) go(gather_blend_norm_kernel<T16, TOut, 16, 3, P, CH, CHT>, 16);
        else go(gather_blend_norm_kernel<T16, TOut, 16, LN_MAXP, P, CH, CHT>, 16);
    } else if (lpr == 32) {
        if (pieces <= 96) go(gather_blend_norm_kernel<T16, TOut, 32, 3, P, CH, CHT>, 32);
        else go(gather_blend_norm_kernel<T16, TOut, 32, LN_MAXP, P, CH, CHT>, 32);
    } else {
        go(gather_blend_norm_kernel<T16, TOut, 64, 3, P, CH, CHT>, 64);
    }
}

// which calls the fused-norm form covers (the hook path's: 16-bit model, residual of the model type)
static bool gbn_supported(int D, int P, int in_dtype, int res_dtype, int out_dtype, int norm_dtype, bool has_res) {
    return has_res && (in_dtype == TF_BF16 || in_dtype == TF_F16) && res_dtype == in_dtype && norm_dtype == in_dtype &&
           out_dtype == (P == 2 ? TF_F32 : in_dtype) && D % 8 == 0 && D <= 1536;
}

template <typename T16>
void dispatch_gbn(const GbArgs& a) {
    if (a.rg) launch_gbn<T16, float, 2, true, GbRagged>(a);
    else if (a.ch.nc > 0) launch_gbn<T16, float, 2, true>(a);
    else if (a.P == 2) launch_gbn<T16, float, 2, false>(a);
    else launch_gbn<T16, T16, 1, false>(a);
}

template <typename TIn, typename TRes, typename TOut>
void launch_gb(const GbArgs& a) {
    const int64_t total = (int64_t)a.n * a.S * (a.D >> 3);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    auto go = [&](auto kern, int kf1, auto* desc) {   // desc: the descriptor type of `kern` (gb_desc)
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, a.st, (const TIn*)a.kf_out, a.idx, a.part,
                           a.splits, a.w, (const TRes*)a.resid, (TOut*)a.out, a.K, a.n, a.S, a.D, a.kf0, kf1, gb_desc(a, desc),
                           a.nb);
    };
    const GbChunks* const chunks = nullptr;
    const GbRagged* const ragged = nullptr;
    if (tf_plan_note(a.rg ? "gather[branches=%d,ragged]" : "gather[branches=%d]", a.nb)) return;
    if (a.rg) {   // ragged call: the chunk forms over the prefix table
        if (a.dyn) go(gather_blend_kernel<TIn, TRes, TOut, 2, true, true, true, GbRagged>, a.kf1, ragged);
        else go(gather_blend_kernel<TIn, TRes, TOut, 2, true, true, false, GbRagged>, a.kf1, ragged);
    } else if (a.dyn) {   // multi-edit batch: the chunk form, or the one-keyframe chunk alone
        if (a.ch.nc > 0) go(gather_blend_kernel<TIn, TRes, TOut, 2, true, true, true>, a.kf1, chunks);
        else go(gather_blend_kernel<TIn, TRes, TOut, 1, true, false, true>, a.kf0, chunks);
    } else if (a.ch.nc > 0) {
        go(gather_blend_kernel<TIn, TRes, TOut, 2, true, true>, a.kf1, chunks);
    } else if (a.part) {
        if (a.P == 2) go(gather_blend_kernel<TIn, TRes, TOut, 2, true>, a.kf1, chunks);
        else go(gather_blend_kernel<TIn, TRes, TOut, 1, true>, a.kf0, chunks);
    } else {
        if (a.P == 2) go(gather_blend_kernel<TIn, TRes, TOut, 2, false>, a.kf1, chunks);
        else go(gather_blend_kernel<TIn, TRes, TOut, 1, false>, a.kf0, chunks);
    }
}

template <typename TIn, typename TRes>
void dispatch_out(const GbArgs& a, int out_dtype) {
    switch (out_dtype) {
        case TF_BF16: launch_gb<TIn, TRes, __bf16>(a); break;
        case TF_F16: launch_gb<TIn, TRes, _Float16>(a); break;
        default: launch_gb<TIn, TRes, float>(a); break;
    }
}

template <typename TIn>
void dispatch_res(const GbArgs& a, int res_dtype, int out_dtype) {
    if (!a.resid) return dispatch_out<TIn, NoRes>(a, out_dtype);
    switch (res_dtype) {
        case TF_BF16: dispatch_out<TIn, __bf16>(a, out_dtype); break;
        case TF_F16: dispatch_out<TIn, _Float16>(a, out_dtype); break;
        default: dispatch_out<TIn, float>(a, out_dtype); break;
    }
}

void dispatch_in(const GbArgs& a, int in_dtype, int res_dtype, int out_dtype) {
    switch (in_dtype) {
        case TF_BF16: dispatch_res<__bf16>(a, res_dtype, out_dtype); break;
        case TF_F16: dispatch_res<_Float16>(a, res_dtype, out_dtype); break;
        default: dispatch_res<float>(a, res_dtype, out_dtype); break;
    }
}

bool gb_okdt(int d) { return d == TF_BF16 || d == TF_F16 || d == TF_F32; }

}  // namespace

extern "C" int tf_gather_blend(const void* kf_out, const int32_t* idx, const float* w, const void* resid, void* out,
                               int K, int n, int S, int D, int P, int kf0, int kf1, int in_dtype, int res_dtype,
                               int out_dtype, void* stream) {
    TF_ARG(kf_out && idx && out && (P == 1 || w), TF_ERR_NULL, "tf_gather_blend: null pointer");
    TF_ARG(gb_okdt(in_dtype) && gb_okdt(out_dtype) && (!resid || gb_okdt(res_dtype)), TF_ERR_DTYPE,
           "tf_gather_blend: dtypes in=%d res=%d out=%d", in_dtype, res_dtype, out_dtype);
    TF_ARG(K > 0 && n > 0 && S > 0 && D > 0 && D % 8 == 0 && (P == 1 || P == 2) && kf0 >= 0 && kf0 < K &&
               (P == 1 || (kf1 >= 0 && kf1 < K)),
           TF_ERR_SHAPE, "tf_gather_blend: K=%d n=%d S=%d D=%d P=%d kf=(%d,%d)", K, n, S, D, P, kf0, kf1);
    TF_ARG(tf_aligned16(kf_out) && tf_aligned16(out) && tf_aligned16(resid), TF_ERR_ALIGN,
           "tf_gather_blend: tensors not 16-byte aligned");
    GbArgs a{kf_out, idx, nullptr, 0, w, resid, out, K, n, S, D, P, kf0, kf1, reinterpret_cast<hipStream_t>(stream),
             GbChunks{0, 0, 0}};
    dispatch_in(a, in_dtype, res_dtype, out_dtype);
    TF_LAUNCH_CHECK("tf_gather_blend");
    return 0;
}

extern "C" size_t tf_nn_gather_blend_workspace_bytes(int64_t n_tgt, int S, int D, int P) {
    if (n_tgt <= 0 || S <= 0 || D <= 0 || P <= 0) return 0;
    const size_t b = tf_nn_partials_bytes(n_tgt, S, D, P);
    return b < 256 ? 256 : b;
}

struct NormArgs {   // the block's next LayerNorm, fused behind the gather (all null / 0: no norm)
    void* out = nullptr;
    const void* gamma = nullptr;
    const void* beta = nullptr;
    float eps = 0.f;
    int w_dtype = 0, dtype = 0;
};
// of a *_norm* entry point, in the order these have the arguments
static NormArgs norm_args(const void* gamma, const void* beta, float eps, int w_dtype, void* norm_out, int norm_dtype) {
    NormArgs nm;
    nm.out = norm_out, nm.gamma = gamma, nm.beta = beta, nm.eps = eps, nm.w_dtype = w_dtype, nm.dtype = norm_dtype;
    return nm;
}

// What every tf_nn_gather_blend* entry point is called with; `name` is the entry point's own, for its refusals.
struct GbCall {
    const char* name;
    const void *tgt, *piv;
    const float* inv_norm;
    const void* kf_out;
    const float* w;
    const void* resid;
    void* out;
    int search_dtype, in_dtype, res_dtype, out_dtype;
    void* ws;
    size_t ws_bytes;
    void* stream;
    NormArgs nm;
};

// The refusals the three impls below share, in two halves: each impl has its shape refusals where it always had them,
// between the halves or in front of both.  First half: null pointers (w_ok: the blend weights, which a one-keyframe call
// goes without), the search dtype, the tensor dtypes (single_dtype: null for a call that has none).
static int gb_check_types(const GbCall& c, bool w_ok, const int* single_dtype) {
    TF_ARG(c.tgt && c.piv && c.inv_norm && c.kf_out && c.out && c.ws && w_ok, TF_ERR_NULL, "%s: null pointer", c.name);
    TF_ARG(c.search_dtype == TF_BF16 || c.search_dtype == TF_F16, TF_ERR_DTYPE, "%s: search dtype %d (bf16/f16 only)", c.name,
           c.search_dtype);
    const bool ok = gb_okdt(c.in_dtype) && gb_okdt(c.out_dtype) && (!c.resid || gb_okdt(c.res_dtype));
    if (single_dtype)
        TF_ARG(ok && gb_okdt(*single_dtype), TF_ERR_DTYPE, "%s: dtypes in=%d res=%d out=%d single=%d", c.name, c.in_dtype,
               c.res_dtype, c.out_dtype, *single_dtype);
    else
        TF_ARG(ok, TF_ERR_DTYPE, "%s: dtypes in=%d res=%d out=%d", c.name, c.in_dtype, c.res_dtype, c.out_dtype);
    return 0;
}
// Second half: 16-byte alignment, the fused norm of a P-keyframe gather (norm_result: how the impl words the result type
// it needs) and the workspace of `need` bytes.
static int gb_check_rest(const GbCall& c, int D, int P, const char* norm_result, size_t need) {
    TF_ARG(tf_aligned16(c.tgt) && tf_aligned16(c.piv) && tf_aligned16(c.kf_out) && tf_aligned16(c.out) &&
               tf_aligned16(c.resid) && tf_aligned16(c.ws) && tf_aligned16(c.inv_norm),
           TF_ERR_ALIGN, "%s: tensors not 16-byte aligned (inv_norm included)", c.name);
    const NormArgs& nm = c.nm;
    if (nm.out) {
        TF_ARG((!nm.gamma && !nm.beta) || gb_okdt(nm.w_dtype), TF_ERR_DTYPE, "%s: norm weight dtype %d", c.name, nm.w_dtype);
        TF_ARG(gbn_supported(D, P, c.in_dtype, c.res_dtype, c.out_dtype, nm.dtype, c.resid != nullptr), TF_ERR_DTYPE,
               "%s: the fused norm needs a 16-bit cached output, a residual and a norm output of that same type%s; D <= 1536",
               c.name, norm_result);
        TF_ARG(tf_aligned16(nm.out) && tf_aligned16(nm.gamma) && tf_aligned16(nm.beta), TF_ERR_ALIGN,
               "%s: norm tensors not 16-byte aligned", c.name);
    }
    TF_ARG(c.ws_bytes >= need, TF_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", c.name, c.ws_bytes, need);
    return 0;
}

// The gather behind the search of all three impls: plain or with the fused norm.  (While a plan is recorded nothing was
// launched: no launch check.)
static int run_gather(const GbCall& c, GbArgs& a) {
    const NormArgs& nm = c.nm;
    if (nm.out) {
        a.norm_out = nm.out, a.gamma = nm.gamma, a.beta = nm.beta, a.w_dtype = nm.w_dtype, a.eps = nm.eps;
        if (c.in_dtype == TF_BF16) dispatch_gbn<__bf16>(a);
        else dispatch_gbn<_Float16>(a);
    } else {
        dispatch_in(a, c.in_dtype, c.res_dtype, c.out_dtype);
    }
    if (tf_plan_rec) return 0;
    TF_LAUNCH_CHECK(c.name);
    return 0;
}

static int nn_gather_blend_impl(const GbCall& c, int K, int n, int S, int D, int P, int kf0, int kf1,
                                int n_edits = 0) {   // n_edits >= 1: a multi-edit batch of 1 + 2*n_edits branches
    if (const int rc = gb_check_types(c, P == 1 || c.w, nullptr)) return rc;
    TF_ARG(K > 0 && n > 0 && S > 0 && D > 0 && D % 8 == 0 && (P == 1 || P == 2) && kf0 >= 0 && kf0 < K &&
               (P == 1 || (kf1 >= 0 && kf1 < K)),
           TF_ERR_SHAPE, "%s: K=%d n=%d S=%d D=%d P=%d kf=(%d,%d)", c.name, K, n, S, D, P, kf0, kf1);
    const int64_t n_tgt = (int64_t)n * S;
    if (const int rc = gb_check_rest(c, D, P, ", and the result in fp32 (two keyframes) or that type (one)",
                                     tf_nn_gather_blend_workspace_bytes(n_tgt, S, D, P)))
        return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
    NnPartial* part = reinterpret_cast<NnPartial*>(c.ws);
    int splits = 1;
    if (const int rc = tf_nn_search_partials(c.tgt, c.piv, c.inv_norm, part, n_tgt, S, D, P, kf0, kf1, c.search_dtype, st, &splits))
        return rc;
    GbArgs a{c.kf_out, nullptr, part, splits, c.w, c.resid, c.out, K, n, S, D, P, kf0, kf1, st, GbChunks{0, 0, 0}};
    if (n_edits > 0) a.nb = 1 + 2 * n_edits, a.dyn = true;
    return run_gather(c, a);
}

extern "C" int tf_nn_gather_blend(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                                  const float* w, const void* resid, void* out, int K, int n, int S, int D, int P,
                                  int kf0, int kf1, int search_dtype, int in_dtype, int res_dtype, int out_dtype,
                                  void* ws, size_t ws_bytes, void* stream) {
    return nn_gather_blend_impl({"tf_nn_gather_blend", tgt, piv, inv_norm, kf_out, w, resid, out, search_dtype, in_dtype,
                                 res_dtype, out_dtype, ws, ws_bytes, stream, NormArgs{}},
                                K, n, S, D, P, kf0, kf1);
}

extern "C" int tf_nn_gather_blend_norm(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                                       const float* w, const void* resid, void* out, int K, int n, int S, int D, int P,
                                       int kf0, int kf1, int search_dtype, int in_dtype, int res_dtype, int out_dtype,
                                       const void* gamma, const void* beta, float eps, int w_dtype, void* norm_out,
                                       int norm_dtype, void* ws, size_t ws_bytes, void* stream) {
    TF_ARG(norm_out, TF_ERR_NULL, "tf_nn_gather_blend_norm: null norm_out");
    return nn_gather_blend_impl({"tf_nn_gather_blend_norm", tgt, piv, inv_norm, kf_out, w, resid, out, search_dtype, in_dtype,
                                 res_dtype, out_dtype, ws, ws_bytes, stream,
                                 norm_args(gamma, beta, eps, w_dtype, norm_out, norm_dtype)},
                                K, n, S, D, P, kf0, kf1);
}

extern "C" size_t tf_nn_gather_blend_chunks_workspace_bytes(int64_t n_tgt_chunk, int S, int D, int C) {
    if (n_tgt_chunk <= 0 || S <= 0 || D <= 0 || C <= 0) return 0;
    const size_t b = tf_nn_partials_bytes(n_tgt_chunk, S, D, 2, C);
    return b < 256 ? 256 : b;
}

static int nn_gather_blend_chunks_impl(const GbCall& c, int K, int n, int C, int S, int D, int slot0, uint64_t single_mask,
                                       int single_dtype, int n_edits = 0,
                                       bool segments = false) {   // segments: the mask of the *_segments entry points
    if (const int rc = gb_check_types(c, c.w != nullptr, &single_dtype)) return rc;
    // chunk j reads keyframe slots slot0 + j and slot0 + j - 1 (the one-keyframe chunk only slot0)
    const bool first_single = single_mask & 1;
    TF_ARG(K > 0 && n > 0 && C > 0 && S > 0 && D > 0 && D % 8 == 0 && slot0 + C <= K &&
               slot0 >= (first_single ? 0 : 1) && (segments || C > 1 || !first_single),
           TF_ERR_SHAPE, "%s: K=%d n=%d C=%d S=%d D=%d slot0=%d first_single=%d", c.name, K, n, C, S, D, slot0,
           (int)first_single);
    // a chunk that starts a keyframe segment matches slot0 + j alone: one bit per chunk of the call
    TF_ARG(!segments || (C <= 64 && (C == 64 || !(single_mask >> C))), TF_ERR_SHAPE,
           "%s: C=%d single_mask=0x%llx (C <= 64, no bit at or above C)", c.name, C, (unsigned long long)single_mask);
    const int64_t n_tgt = (int64_t)n * S;   // per chunk
    if (const int rc = gb_check_rest(c, D, 2, " and the result in fp32", tf_nn_gather_blend_chunks_workspace_bytes(n_tgt, S, D, C)))
        return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
    NnPartial* part = reinterpret_cast<NnPartial*>(c.ws);
    int splits = 1;
    if (const int rc = tf_nn_search_partials(c.tgt, c.piv, c.inv_norm, part, n_tgt, S, D, 2, slot0, slot0 - 1, c.search_dtype, st,
                                             &splits, C, single_mask))
        return rc;
    GbArgs a{c.kf_out, nullptr, part, splits, c.w, c.resid, c.out, K, n * C, S, D, 2, slot0, slot0 - 1, st,
             GbChunks{n, single_dtype, single_mask}};
    if (n_edits > 0) a.nb = 1 + 2 * n_edits, a.dyn = true;
    return run_gather(c, a);
}

extern "C" int tf_nn_gather_blend_chunks(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                                         const float* w, const void* resid, void* out, int K, int n, int C, int S,
                                         int D, int slot0, int first_single, int search_dtype, int in_dtype,
                                         int res_dtype, int out_dtype, int single_dtype, void* ws, size_t ws_bytes,
                                         void* stream) {
    return nn_gather_blend_chunks_impl({"tf_nn_gather_blend_chunks", tgt, piv, inv_norm, kf_out, w, resid, out, search_dtype,
                                        in_dtype, res_dtype, out_dtype, ws, ws_bytes, stream, NormArgs{}},
                                       K, n, C, S, D, slot0, first_single ? 1 : 0, single_dtype);
}

extern "C" int tf_nn_gather_blend_chunks_norm(const void* tgt, const void* piv, const float* inv_norm,
                                              const void* kf_out, const float* w, const void* resid, void* out, int K,
                                              int n, int C, int S, int D, int slot0, int first_single, int search_dtype,
                                              int in_dtype, int res_dtype, int out_dtype, int single_dtype,
                                              const void* gamma, const void* beta, float eps, int w_dtype,
                                              void* norm_out, int norm_dtype, void* ws, size_t ws_bytes, void* stream) {
    TF_ARG(norm_out, TF_ERR_NULL, "tf_nn_gather_blend_chunks_norm: null norm_out");
    return nn_gather_blend_chunks_impl({"tf_nn_gather_blend_chunks_norm", tgt, piv, inv_norm, kf_out, w, resid, out,
                                        search_dtype, in_dtype, res_dtype, out_dtype, ws, ws_bytes, stream,
                                        norm_args(gamma, beta, eps, w_dtype, norm_out, norm_dtype)},
                                       K, n, C, S, D, slot0, first_single ? 1 : 0, single_dtype);
}

// Keyframe segments (include/tokenflow_hip.h): the chunk forms with one bit per chunk in the place of first_single -- every
// chunk that starts a segment is a one-keyframe chunk.  Same search launch, same gather launch; mask 0 / 1 are the chunk forms.
extern "C" int tf_nn_gather_blend_chunks_segments(const void* tgt, const void* piv, const float* inv_norm,
                                                  const void* kf_out, const float* w, const void* resid, void* out, int K,
                                                  int n, int C, int S, int D, int slot0, uint64_t single_mask,
                                                  int search_dtype, int in_dtype, int res_dtype, int out_dtype,
                                                  int single_dtype, void* ws, size_t ws_bytes, void* stream) {
    return nn_gather_blend_chunks_impl({"tf_nn_gather_blend_chunks_segments", tgt, piv, inv_norm, kf_out, w, resid, out,
                                        search_dtype, in_dtype, res_dtype, out_dtype, ws, ws_bytes, stream, NormArgs{}},
                                       K, n, C, S, D, slot0, single_mask, single_dtype, 0, true);
}

extern "C" int tf_nn_gather_blend_chunks_norm_segments(const void* tgt, const void* piv, const float* inv_norm,
                                                       const void* kf_out, const float* w, const void* resid, void* out,
                                                       int K, int n, int C, int S, int D, int slot0, uint64_t single_mask,
                                                       int search_dtype, int in_dtype, int res_dtype, int out_dtype,
                                                       int single_dtype, const void* gamma, const void* beta, float eps,
                                                       int w_dtype, void* norm_out, int norm_dtype, void* ws,
                                                       size_t ws_bytes, void* stream) {
    TF_ARG(norm_out, TF_ERR_NULL, "tf_nn_gather_blend_chunks_norm_segments: null norm_out");
    return nn_gather_blend_chunks_impl({"tf_nn_gather_blend_chunks_norm_segments", tgt, piv, inv_norm, kf_out, w, resid, out,
                                        search_dtype, in_dtype, res_dtype, out_dtype, ws, ws_bytes, stream,
                                        norm_args(gamma, beta, eps, w_dtype, norm_out, norm_dtype)},
                                       K, n, C, S, D, slot0, single_mask, single_dtype, 0, true);
}

// placeholder tensors of the *_plan queries: aligned, never dereferenced
static void* const gb_ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
static const float* const gb_phf = reinterpret_cast<const float*>(gb_ph);

// Launch plan of tf_nn_gather_blend_chunks_segments (host only): the entry point itself under the plan recorder.
extern "C" int tf_nn_gather_blend_segments_plan(int n, int C, int S, int D, uint64_t single_mask, char* buf, size_t len) {
    TF_ARG(n > 0 && C > 0 && S > 0 && D > 0 && D % 8 == 0, TF_ERR_SHAPE,
           "tf_nn_gather_blend_segments_plan: n=%d C=%d S=%d D=%d", n, C, S, D);
    return tf_record_plan("tf_nn_gather_blend_segments_plan", buf, len, [&] {
        return tf_nn_gather_blend_chunks_segments(gb_ph, gb_ph, gb_phf, gb_ph, gb_phf, gb_ph, gb_ph, C + 1, n, C, S, D,
                                                  (single_mask & 1) ? 0 : 1, single_mask, TF_BF16, TF_BF16, TF_BF16, TF_F32,
                                                  TF_BF16, gb_ph, (size_t)-1, nullptr);
    });
}

// Multi-edit batches (include/tokenflow_hip.h): the chunk forms over B = 1 + 2*n_edits branches.  ONE search (the launches of the
// 3-branch call: the search reads the source branch only), then the gather loops the B branches on the same candidates.
// C == 1 is served by the one-chunk forms (the one-keyframe chunk 0 of the video: P = 1; any other chunk: P = 2).
static int nn_gather_blend_edits(const GbCall& c, int K, int n, int C, int S, int D, int slot0, int first_single,
                                 int single_dtype, int n_edits) {
    TF_ARG(n_edits >= 1 && n_edits <= TF_MAX_EDITS, TF_ERR_SHAPE, "%s: n_edits=%d (1 .. %d)", c.name, n_edits, TF_MAX_EDITS);
    if (C == 1 && first_single) {
        TF_ARG(slot0 >= 0 && slot0 < K, TF_ERR_SHAPE, "%s: slot0=%d outside the %d keyframes", c.name, slot0, K);
        TF_ARG(c.out_dtype == single_dtype, TF_ERR_DTYPE,
               "%s: the one-keyframe chunk alone is stored in the dtype its own pass produces (out=%d single=%d)", c.name,
               c.out_dtype, single_dtype);
        GbCall one = c;
        one.w = nullptr;
        return nn_gather_blend_impl(one, K, n, S, D, 1, slot0, 0, n_edits);
    }
    return nn_gather_blend_chunks_impl(c, K, n, C, S, D, slot0, first_single ? 1 : 0, single_dtype, n_edits);
}

extern "C" int tf_nn_gather_blend_chunks_edits(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                                               const float* w, const void* resid, void* out, int K, int n, int C, int S,
                                               int D, int slot0, int first_single, int search_dtype, int in_dtype,
                                               int res_dtype, int out_dtype, int single_dtype, int n_edits, void* ws,
                                               size_t ws_bytes, void* stream) {
    return nn_gather_blend_edits({"tf_nn_gather_blend_chunks_edits", tgt, piv, inv_norm, kf_out, w, resid, out, search_dtype,
                                  in_dtype, res_dtype, out_dtype, ws, ws_bytes, stream, NormArgs{}},
                                 K, n, C, S, D, slot0, first_single, single_dtype, n_edits);
}

extern "C" int tf_nn_gather_blend_chunks_norm_edits(const void* tgt, const void* piv, const float* inv_norm,
                                                    const void* kf_out, const float* w, const void* resid, void* out,
                                                    int K, int n, int C, int S, int D, int slot0, int first_single,
                                                    int search_dtype, int in_dtype, int res_dtype, int out_dtype,
                                                    int single_dtype, int n_edits, const void* gamma, const void* beta,
                                                    float eps, int w_dtype, void* norm_out, int norm_dtype, void* ws,
                                                    size_t ws_bytes, void* stream) {
    TF_ARG(norm_out, TF_ERR_NULL, "tf_nn_gather_blend_chunks_norm_edits: null norm_out");
    return nn_gather_blend_edits({"tf_nn_gather_blend_chunks_norm_edits", tgt, piv, inv_norm, kf_out, w, resid, out,
                                  search_dtype, in_dtype, res_dtype, out_dtype, ws, ws_bytes, stream,
                                  norm_args(gamma, beta, eps, w_dtype, norm_out, norm_dtype)},
                                 K, n, C, S, D, slot0, first_single, single_dtype, n_edits);
}

// Launch plan of tf_nn_gather_blend_chunks_edits (host only): the entry point itself under the plan recorder.
extern "C" int tf_nn_gather_blend_edits_plan(int n, int C, int S, int D, int first_single, int n_edits, char* buf,
                                             size_t len) {
    TF_ARG(n > 0 && C > 0 && S > 0 && D > 0 && D % 8 == 0, TF_ERR_SHAPE, "tf_nn_gather_blend_edits_plan: n=%d C=%d S=%d D=%d",
           n, C, S, D);
    return tf_record_plan("tf_nn_gather_blend_edits_plan", buf, len, [&] {
        return tf_nn_gather_blend_chunks_edits(gb_ph, gb_ph, gb_phf, gb_ph, gb_phf, gb_ph, gb_ph, C + 1, n, C, S, D,
                                               first_single ? 0 : 1, first_single, TF_BF16, TF_BF16, TF_BF16,
                                               (C == 1 && first_single) ? TF_BF16 : TF_F32, TF_BF16, n_edits, gb_ph, (size_t)-1,
                                               nullptr);
    });
}

// Ragged chunk runs (include/tokenflow_hip.h): chunk j of the call has its own frame count.  Equal counts ARE today's calls
// (the segments form for n_edits = 1, the edits form above it); everything else is one ragged search and one ragged gather.
static bool ragged_uniform(const int* frames, int C) {
    for (int j = 1; j < C; ++j)
        if (frames[j] != frames[0]) return false;
    return true;
}
// the shape refusals every ragged entry point shares; *rows = targets of the call
static int ragged_check(const char* name, const int* frames, int C, int S, int D, uint64_t single_mask, int64_t* rows) {
    TF_ARG(frames, TF_ERR_NULL, "%s: null chunk_frames", name);
    TF_ARG(C >= 1 && C <= TF_RAGGED_MAX_CHUNKS && S > 0 && D > 0 && D % 8 == 0, TF_ERR_SHAPE,
           "%s: C=%d S=%d D=%d (1 <= C <= %d)", name, C, S, D, TF_RAGGED_MAX_CHUNKS);
    TF_ARG(C == 64 || !(single_mask >> C), TF_ERR_SHAPE, "%s: C=%d single_mask=0x%llx (no bit at or above C)", name, C,
           (unsigned long long)single_mask);
    int64_t r = 0;
    for (int j = 0; j < C; ++j) {
        TF_ARG(frames[j] >= 1, TF_ERR_SHAPE, "%s: chunk %d has %d frames (>= 1)", name, j, frames[j]);
        r += (int64_t)frames[j] * S;
        TF_ARG(r <= (int64_t)INT32_MAX, TF_ERR_SHAPE, "%s: the call's targets (sum of frames * S) must stay below 2^31", name);
    }
    *rows = r;
    return 0;
}

extern "C" size_t tf_nn_gather_blend_ragged_workspace_bytes(const int* chunk_frames, int C, int S, int D) {
    int64_t rows = 0;
    if (ragged_check("tf_nn_gather_blend_ragged_workspace_bytes", chunk_frames, C, S, D, 0, &rows)) return 0;
    size_t b;
    if (ragged_uniform(chunk_frames, C)) {
        const int64_t nS = (int64_t)chunk_frames[0] * S;
        b = tf_nn_gather_blend_chunks_workspace_bytes(nS, S, D, C);
        if (C == 1) {   // the one-keyframe chunk alone of a multi-edit batch searches one keyframe
            const size_t b1 = tf_nn_gather_blend_workspace_bytes(nS, S, D, 1);
            b = b1 > b ? b1 : b;
        }
    } else {
        b = tf_nn_partials_bytes_ragged(chunk_frames, C, S, D);
    }
    return b < 256 ? 256 : b;
}

static int nn_gather_blend_ragged_impl(const GbCall& c, int K, const int* frames, int C, int S, int D, int slot0,
                                       uint64_t single_mask, int single_dtype, int n_edits) {
    int64_t rows = 0;
    if (const int rc = ragged_check(c.name, frames, C, S, D, single_mask, &rows)) return rc;
    TF_ARG(n_edits >= 1 && n_edits <= TF_MAX_EDITS, TF_ERR_SHAPE, "%s: n_edits=%d (1 .. %d)", c.name, n_edits, TF_MAX_EDITS);
    TF_ARG(n_edits == 1 || single_mask <= 1, TF_ERR_SHAPE,
           "%s: single_mask=0x%llx with %d edits (segments and multi-edit batches do not combine: bit 0 only)", c.name,
           (unsigned long long)single_mask, n_edits);
    const bool first_single = single_mask & 1;
    TF_ARG(K > 0 && slot0 + C <= K && slot0 >= (first_single ? 0 : 1), TF_ERR_SHAPE, "%s: K=%d C=%d slot0=%d first_single=%d",
           c.name, K, C, slot0, (int)first_single);
    if (ragged_uniform(frames, C)) {   // today's call: same launches, same plan tokens, same bits
        if (n_edits == 1) return nn_gather_blend_chunks_impl(c, K, frames[0], C, S, D, slot0, single_mask, single_dtype, 0, true);
        return nn_gather_blend_edits(c, K, frames[0], C, S, D, slot0, first_single, single_dtype, n_edits);
    }
    if (const int rc = gb_check_types(c, c.w != nullptr, &single_dtype)) return rc;
    if (const int rc = gb_check_rest(c, D, 2, " and the result in fp32", tf_nn_gather_blend_ragged_workspace_bytes(frames, C, S, D)))
        return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
    NnPartial* part = reinterpret_cast<NnPartial*>(c.ws);
    int splits = 1;
    if (const int rc = tf_nn_search_partials_ragged(c.tgt, c.piv, c.inv_norm, part, frames, C, S, D, slot0, slot0 - 1,
                                                    c.search_dtype, st, &splits, single_mask))
        return rc;
    GbRagged rg;
    rg.single_dtype = single_dtype, rg.single_mask = single_mask;
    int64_t row = 0;
    for (int j = 0; j <= TF_RAGGED_MAX_CHUNKS; ++j) {
        rg.row0[j] = j <= C ? (int)row : INT32_MAX;
        if (j < C) row += (int64_t)frames[j] * S;
    }
    GbArgs a{c.kf_out, nullptr, part, splits, c.w, c.resid, c.out, K, (int)(rows / S), S, D, 2, slot0, slot0 - 1, st,
             GbChunks{0, 0, 0}};
    a.rg = &rg;
    a.nb = 1 + 2 * n_edits, a.dyn = n_edits > 1;
    return run_gather(c, a);
}

extern "C" int tf_nn_gather_blend_chunks_ragged(const void* tgt, const void* piv, const float* inv_norm, const void* kf_out,
                                                const float* w, const void* resid, void* out, int K, const int* chunk_frames,
                                                int C, int S, int D, int slot0, uint64_t single_mask, int search_dtype,
                                                int in_dtype, int res_dtype, int out_dtype, int single_dtype, int n_edits,
                                                void* ws, size_t ws_bytes, void* stream) {
    return nn_gather_blend_ragged_impl({"tf_nn_gather_blend_chunks_ragged", tgt, piv, inv_norm, kf_out, w, resid, out,
                                        search_dtype, in_dtype, res_dtype, out_dtype, ws, ws_bytes, stream, NormArgs{}},
                                       K, chunk_frames, C, S, D, slot0, single_mask, single_dtype, n_edits);
}

extern "C" int tf_nn_gather_blend_chunks_norm_ragged(const void* tgt, const void* piv, const float* inv_norm,
                                                     const void* kf_out, const float* w, const void* resid, void* out, int K,
                                                     const int* chunk_frames, int C, int S, int D, int slot0,
                                                     uint64_t single_mask, int search_dtype, int in_dtype, int res_dtype,
                                                     int out_dtype, int single_dtype, int n_edits, const void* gamma,
                                                     const void* beta, float eps, int w_dtype, void* norm_out, int norm_dtype,
                                                     void* ws, size_t ws_bytes, void* stream) {
    TF_ARG(norm_out, TF_ERR_NULL, "tf_nn_gather_blend_chunks_norm_ragged: null norm_out");
    return nn_gather_blend_ragged_impl({"tf_nn_gather_blend_chunks_norm_ragged", tgt, piv, inv_norm, kf_out, w, resid, out,
                                        search_dtype, in_dtype, res_dtype, out_dtype, ws, ws_bytes, stream,
                                        norm_args(gamma, beta, eps, w_dtype, norm_out, norm_dtype)},
                                       K, chunk_frames, C, S, D, slot0, single_mask, single_dtype, n_edits);
}

// Launch plan of tf_nn_gather_blend_chunks_ragged (host only): the entry point itself under the plan recorder.
extern "C" int tf_nn_gather_blend_ragged_plan(const int* chunk_frames, int C, int S, int D, uint64_t single_mask, int n_edits,
                                              char* buf, size_t len) {
    // the one-keyframe chunk alone of a multi-edit batch is stored in the dtype its own pass produces
    const bool one_single = C == 1 && (single_mask & 1) && n_edits > 1;
    return tf_record_plan("tf_nn_gather_blend_ragged_plan", buf, len, [&] {
        return tf_nn_gather_blend_chunks_ragged(gb_ph, gb_ph, gb_phf, gb_ph, gb_phf, gb_ph, gb_ph, C + 1, chunk_frames, C, S, D,
                                                (single_mask & 1) ? 0 : 1, single_mask, TF_BF16, TF_BF16, TF_BF16,
                                                one_single ? TF_BF16 : TF_F32, TF_BF16, n_edits, gb_ph, (size_t)-1, nullptr);
    });
}

extern "C" int tf_inject_copy(void* x, int64_t elems_per_branch, int elem_bytes, void* stream) {
    TF_ARG(x, TF_ERR_NULL, "tf_inject_copy: null pointer");
    TF_ARG(elems_per_branch > 0 && elem_bytes > 0 && (elems_per_branch * elem_bytes) % 16 == 0, TF_ERR_SHAPE,
           "tf_inject_copy: elems_per_branch=%lld elem_bytes=%d (bytes per branch %% 16 == 0)",
           (long long)elems_per_branch, elem_bytes);
    TF_ARG(tf_aligned16(x), TF_ERR_ALIGN, "tf_inject_copy: x not 16-byte aligned");
    const int64_t pieces = elems_per_branch * elem_bytes / 16;
    int64_t blocks = (pieces + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(inject_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<u32x4*>(x), pieces);
    TF_LAUNCH_CHECK("tf_inject_copy");
    return 0;
}

// edit_mask: bit e = edit e's uncond and cond branches take the source; `masked` = false is the unmasked launch
static int inject_copy_edits_impl(const char* name, void* x, int64_t elems_per_branch, int n_branches, bool masked,
                                  unsigned edit_mask, int elem_bytes, void* stream) {
    TF_ARG(x, TF_ERR_NULL, "%s: null pointer", name);
    TF_ARG(elems_per_branch > 0 && elem_bytes > 0 && (elems_per_branch * elem_bytes) % 16 == 0 && n_branches >= 3 &&
               n_branches <= 1 + 2 * TF_MAX_EDITS && (n_branches & 1),
           TF_ERR_SHAPE, "%s: elems_per_branch=%lld elem_bytes=%d n_branches=%d (bytes per branch %% 16 == 0; "
           "1 + 2E branches, E <= %d)", name, (long long)elems_per_branch, elem_bytes, n_branches, TF_MAX_EDITS);
    TF_ARG(tf_aligned16(x), TF_ERR_ALIGN, "%s: x not 16-byte aligned", name);
    const int n_edits = (n_branches - 1) / 2;
    TF_ARG(!masked || !(edit_mask >> n_edits), TF_ERR_SHAPE, "%s: edit_mask=0x%x has bits at or above the %d edits", name,
           edit_mask, n_edits);
    if (masked && edit_mask == 0) return 0;   // nobody injects: nothing to launch
    unsigned branch_mask = 0;
    for (int e = 0; e < n_edits; ++e)
        if ((edit_mask >> e) & 1u) branch_mask |= 3u << (1 + 2 * e);
    const int64_t pieces = elems_per_branch * elem_bytes / 16;
    int64_t blocks = (pieces + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(masked ? inject_copy_edits_kernel<true> : inject_copy_edits_kernel<false>, dim3((unsigned)blocks),
                       dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<u32x4*>(x), pieces, n_branches,
                       branch_mask);
    TF_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int tf_inject_copy_edits(void* x, int64_t elems_per_branch, int n_branches, int elem_bytes, void* stream) {
    return inject_copy_edits_impl("tf_inject_copy_edits", x, elems_per_branch, n_branches, false, 0u, elem_bytes, stream);
}

extern "C" int tf_inject_copy_edits_masked(void* x, int64_t elems_per_branch, int n_branches, unsigned edit_mask,
                                           int elem_bytes, void* stream) {
    return inject_copy_edits_impl("tf_inject_copy_edits_masked", x, elems_per_branch, n_branches, true, edit_mask, elem_bytes,
                                  stream);
}
