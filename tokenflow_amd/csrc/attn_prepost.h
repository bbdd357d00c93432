// Extended attention: the V^T / key-norm pre-pass and the merge kernels of the split and runs forms.
// Included by ext_attn.hip only.
#pragma once

#include "attn_common.h"

namespace {

__device__ __forceinline__ int swap23(int x) { return (x & ~12) | ((x & 4) << 1) | ((x & 8) >> 1); }

// V [3,K,S,H*DH] (token stride ld) -> Vt [3][H][DH][K*Spad + 64], position = f*Spad + swap23(key in frame),
// zero for keys >= S.  grid = (Spad/64, H, branches * frames), 256 threads; one workgroup = 64 keys x DH of one head.
// 16-byte global accesses on both sides (rows of V in, 8 consecutive positions of one V^T row out); the
// transpose itself is 2-byte LDS reads of a [64][DH+2] tile (odd dword stride: conflict-free columns).
// With k != nullptr (Dh = 40 kernels) the same workgroup also writes max |k|^2 over its 64 keys of this head to
// knorm2[(b*H + h) * K*Spad/64 + f*Spad/64 + tt]: the score bound q.k <= |q| max|k| of ext_attn_kernel.
template <typename T>
__global__ __launch_bounds__(256) void vt_pack_kernel(const typename T::elem* __restrict__ v,
                                                      typename T::elem* __restrict__ vt,
                                                      const typename T::elem* __restrict__ k,
                                                      float* __restrict__ knorm2, unsigned own, unsigned kc_mask, int b_src,
                                                      int b0, int nf,
                                                      int K,
                                                      int S, int H, int DH, int Spad, int64_t ld, int64_t v_bs,
                                                      int64_t v_fs, int64_t k_bs, int64_t k_fs, int* __restrict__ run_hdr,
                                                      int run_slots) {
    typedef typename T::elem E;
    typedef typename T::vec8 vec8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    E* tile = reinterpret_cast<E*>(smem);  // [64][DH + 2]
    const int row = DH + 2;
    const int ppr = DH >> 3;               // 16-B pieces per V row
    // blockIdx.z = (branch - b0) * nf + frame: nf frames of every branch from b0 on.  K = frames of the IMAGE (row stride of
    // vt, of knorm2): a run launch packs its nf < K frames with v / vt / k / knorm2 pointing at the run's first frame
    const int tt = blockIdx.x, h = blockIdx.y;
    const int b = b0 + (int)blockIdx.z / nf, f = (int)blockIdx.z % nf;
    // run launches: the number of partial-result slots the run fills, for tf_ext_attn_runs_merge
    if (run_hdr != nullptr && (blockIdx.x | blockIdx.y | blockIdx.z | threadIdx.x) == 0) *run_hdr = run_slots;
    const E* src = v + b * v_bs + f * v_fs + h * DH;
    // keys of branch b where the branch's own keys are read (bit b of `own`: no injection; in a multi-edit batch the source
    // and the edits that do not inject); under injection a branch reads the SOURCE keys, whose norms the workgroups of
    // branch b_src compute (the first packed branch; -1: the source is among the `own` branches)
    const bool own_k = (own >> b) & 1u;
    if (k != nullptr && (own_k || b == b_src) && threadIdx.x < 64) {   // wave 0: one key per lane
        const int kb = own_k ? b : 0;
        // compact q / k of a multi-edit part call (kc_mask = its injection mask, else 0): the keys of branch kb lie two slots
        // further in for every injecting edit in front of its edit; the norms keep the dense index
        const int ks = kb - 2 * __popc(kc_mask & ((1u << ((kb > 0 ? kb - 1 : 0) >> 1)) - 1u));
        const int kk = tt * 64 + (int)threadIdx.x;
        float acc = 0.f;
        if (kk < S) {
            const E* kp = k + ks * k_bs + f * k_fs + (int64_t)kk * ld + h * DH;
            for (int c8 = 0; c8 < DH; c8 += 8) {
                const vec8 x = __builtin_bit_cast(vec8, ld16(kp + c8));
#pragma unroll
                for (int j = 0; j < 8; ++j) acc = fmaf((float)x[j], (float)x[j], acc);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc = fmaxf(acc, __shfl_xor(acc, o));
        if (threadIdx.x == 0) knorm2[((int64_t)(kb * H + h) * K + f) * (Spad / 64) + tt] = acc;
    }
    for (int id = threadIdx.x; id < 64 * ppr; id += 256) {
        const int key = id / ppr, pc = id - key * ppr;
        const int kk = tt * 64 + key;
        const vec8 val = kk < S ? __builtin_bit_cast(vec8, ld16(src + (int64_t)kk * ld + pc * 8))
                                : __builtin_bit_cast(vec8, u32x4{0, 0, 0, 0});
        E* dstp = tile + key * row + pc * 8;   // (DH+2)*2 bytes per row: only 4-byte aligned -> element stores
#pragma unroll
        for (int j = 0; j < 8; ++j) dstp[j] = val[j];
    }
    __syncthreads();
    const int64_t vt_row = vt_row_stride(K, Spad);
    E* dst = vt + ((int64_t)(b * H + h) * DH) * vt_row + (int64_t)f * Spad + tt * 64;
    for (int id = threadIdx.x; id < DH * 8; id += 256) {
        const int d = id >> 3, pg = id & 7;   // 8 consecutive positions pg*8 .. +7 of V^T row d
        vec8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = tile[swap23(pg * 8 + j) * row + d];
        st16(dst + (int64_t)d * vt_row + pg * 8, __builtin_bit_cast(u32x4, o));
    }
}

// Split form, second step: out = sum_seg O_seg 2^(sh_seg - M) / sum_seg l_seg 2^(sh_seg - M), M = max_seg sh_seg.
// One thread per (bank, frame, head, query, 4 consecutive d).
template <typename T>
__global__ __launch_bounds__(256) void attn_merge_kernel(const float* __restrict__ partials, void* __restrict__ out,
                                                         int Kq, int S, int H, int DH, int nseg, int out_f32,
                                                         int64_t o_bs, int64_t o_fs) {
    typedef typename T::elem E;
    typedef typename T::vec4 vec4;
    const int PS = DH + 8, dq = DH >> 2;
    const int64_t total = (int64_t)2 * Kq * H * S * dq;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t R = g / dq;                 // ((vbank*Kq + f)*H + h)*S + q
        const int d0 = (int)(g - R * dq) * 4;
        const float* pr = partials + R * nseg * PS;
        float M = -INFINITY;
        for (int sg = 0; sg < nseg; ++sg) M = fmaxf(M, pr[sg * PS + DH + 1]);
        f32x4 num = {0.f, 0.f, 0.f, 0.f};
        float den = 0.f;
        for (int sg = 0; sg < nseg; ++sg) {
            const float w = __builtin_amdgcn_exp2f(pr[sg * PS + DH + 1] - M);
            const f32x4 o4 = *reinterpret_cast<const f32x4*>(pr + sg * PS + d0);
            num += o4 * w;
            den = fmaf(pr[sg * PS + DH], w, den);
        }
        const float inv = 1.0f / den;
        const int q = (int)(R % S);
        int64_t t = R / S;
        const int h = (int)(t % H);
        t /= H;
        const int f = (int)(t % Kq), vbank = (int)(t / Kq);
        store_out4<E, vec4>(out, (1 + vbank) * o_bs + f * o_fs + (int64_t)q * (H * DH) + h * DH + d0, num * inv, out_f32);
    }
}

// Runs form (tf_ext_attn_run / tf_ext_attn_runs_merge), merge: the same sum over the slots of EVERY run of the bank.  Run r owns
// slots [r * spr, (r + 1) * spr) of a row and filled the first hdr[r] of them (left by the run's pre-pass: a run splits itself
// by split_plan's rule on its own frame count).  The slots are reduced in ascending order, whatever the order or the streams
// in which the runs executed: the result is a function of the runs alone.
template <typename T>
__global__ __launch_bounds__(256) void attn_runs_merge_kernel(const float* __restrict__ partials, const int* __restrict__ hdr,
                                                              void* __restrict__ out, int Kq, int S, int H, int DH, int n_runs,
                                                              int spr, int out_f32, int64_t o_bs, int64_t o_fs) {
    typedef typename T::elem E;
    typedef typename T::vec4 vec4;
    const int PS = DH + 8, dq = DH >> 2;
    const int64_t total = (int64_t)2 * Kq * H * S * dq;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t R = g / dq;                 // ((vbank*Kq + f)*H + h)*S + q
        const int d0 = (int)(g - R * dq) * 4;
        const float* pr = partials + R * ((int64_t)n_runs * spr) * PS;
        float M = -INFINITY;
        for (int r = 0; r < n_runs; ++r) {
            const int ns = min(hdr[r], spr);
            for (int sg = 0; sg < ns; ++sg) M = fmaxf(M, pr[(r * spr + sg) * PS + DH + 1]);
        }
        f32x4 num = {0.f, 0.f, 0.f, 0.f};
        float den = 0.f;
        for (int r = 0; r < n_runs; ++r) {
            const int ns = min(hdr[r], spr);
            for (int sg = 0; sg < ns; ++sg) {
                const float* ps = pr + (r * spr + sg) * PS;
                const float w = __builtin_amdgcn_exp2f(ps[DH + 1] - M);
                num += *reinterpret_cast<const f32x4*>(ps + d0) * w;
                den = fmaf(ps[DH], w, den);
            }
        }
        const float inv = 1.0f / den;
        const int q = (int)(R % S);
        int64_t t = R / S;
        const int h = (int)(t % H);
        t /= H;
        const int f = (int)(t % Kq), vbank = (int)(t / Kq);
        store_out4<E, vec4>(out, (1 + vbank) * o_bs + f * o_fs + (int64_t)q * (H * DH) + h * DH + d0, num * inv, out_f32);
    }
}

// Runs form of a multi-edit batch (tf_ext_attn_run_edits / tf_ext_attn_runs_merge_edits), merge: the 2E bank branches of ALL
// edits in one launch.  partials [2E][Kq][H][S][n_runs * spr][DH + 8]: edit e's two banks are exactly the region a single-edit
// run set has.  How many slots a run filled depends on the edit's injection state (split_plan's `dual`), so hdr[r] carries
// BOTH counts -- bits 0-15 for an edit that does not inject, bits 16-31 for one that does -- and bit e of inject_mask picks
// edit e's.  The same sums in the same slot order as attn_runs_merge_kernel.
template <typename T>
__global__ __launch_bounds__(256) void attn_runs_merge_edits_kernel(const float* __restrict__ partials,
                                                                    const int* __restrict__ hdr, void* __restrict__ out, int Kq,
                                                                    int S, int H, int DH, int n_runs, int spr, int n_banks,
                                                                    unsigned inject_mask, int out_f32, int64_t o_bs,
                                                                    int64_t o_fs) {
    typedef typename T::elem E;
    typedef typename T::vec4 vec4;
    const int PS = DH + 8, dq = DH >> 2;
    const int64_t total = (int64_t)n_banks * Kq * H * S * dq;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t R = g / dq;                 // ((vbank*Kq + f)*H + h)*S + q, vbank = 2 * edit + (0 uncond, 1 cond)
        const int d0 = (int)(g - R * dq) * 4;
        const int q = (int)(R % S);
        int64_t t = R / S;
        const int h = (int)(t % H);
        t /= H;
        const int f = (int)(t % Kq), vbank = (int)(t / Kq);
        const int hsh = ((inject_mask >> (vbank >> 1)) & 1u) ? 16 : 0;
        const float* pr = partials + R * ((int64_t)n_runs * spr) * PS;
        float M = -INFINITY;
        for (int r = 0; r < n_runs; ++r) {
            const int ns = min((hdr[r] >> hsh) & 0xffff, spr);
            for (int sg = 0; sg < ns; ++sg) M = fmaxf(M, pr[(r * spr + sg) * PS + DH + 1]);
        }
        f32x4 num = {0.f, 0.f, 0.f, 0.f};
        float den = 0.f;
        for (int r = 0; r < n_runs; ++r) {
            const int ns = min((hdr[r] >> hsh) & 0xffff, spr);
            for (int sg = 0; sg < ns; ++sg) {
                const float* ps = pr + (r * spr + sg) * PS;
                const float w = __builtin_amdgcn_exp2f(ps[DH + 1] - M);
                num += *reinterpret_cast<const f32x4*>(ps + d0) * w;
                den = fmaf(ps[DH], w, den);
            }
        }
        const float inv = 1.0f / den;
        store_out4<E, vec4>(out, (1 + vbank) * o_bs + f * o_fs + (int64_t)q * (H * DH) + h * DH + d0, num * inv, out_f32);
    }
}

// The V^T pre-pass over branches [b_lo, b_hi) of v (a multi-edit batch: once for all 1 + 2E branches)
template <typename T>
int launch_vt_pack(const AttnParams& p, const void* v, int DH, int b_lo, int b_hi, unsigned own, int b_src, hipStream_t st,
                   unsigned kc_mask = 0) {
    typedef typename T::elem E;
    dim3 grid((unsigned)(p.Spad / 64), (unsigned)p.H, (unsigned)((b_hi - b_lo) * p.K));
    const size_t lds = (size_t)64 * (DH + 2) * sizeof(E);
    // the Dh = 40 kernels also need the key norm bounds (score bound, see BOUND)
    const bool bound = attn_has_bound(DH);
    if (!tf_plan_note("vt_pack")) {
        hipLaunchKernelGGL(vt_pack_kernel<T>, grid, dim3(256), lds, st, reinterpret_cast<const E*>(v),
                           reinterpret_cast<E*>(const_cast<void*>(p.vt)),
                           bound ? reinterpret_cast<const E*>(p.k) : nullptr, const_cast<float*>(p.knorm2),
                           own, kc_mask, b_src, b_lo, p.K, p.Kb, p.S, p.H, DH, p.Spad, p.ld, p.v_bs, p.v_fs, p.k_bs, p.k_fs,
                           p.run_hdr, p.nseg);
        TF_LAUNCH_CHECK("tf_ext_attn_fwd(vt_pack)");
    }
    return 0;
}

}  // namespace
