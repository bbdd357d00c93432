// Proxy of the level-0 NN-search inner loop (nn_search_rbg_kernel<.., 2>: a wave keeps 64 targets x 320 features as MFMA B
// fragments in registers, 32-pivot tiles stream through LDS as A fragments), stripped of staging, barriers and the argmax
// epilogue, run for hundreds of ms on toggling data (the boxes are power-limited).  Question (round 6, after the mixed
// MFMA shapes of the attention kernel): the bare v_mfma_f32_16x16x32_bf16 sustains 17 % more than v_mfma_f32_32x32x16_bf16
// on random data (profiles/r02_mfma_shapes.txt) -- does the search loop get any of that at equal matrix-pipe clocks?
//   SHAPE 0: per 32-pivot tile and 16-wide k-step: 1 ds_read_b128 (32 pivots x 16 k) -> 2 MFMAs 32x32x16 (two 32-target tiles)
//   SHAPE 1: per 32-pivot tile and 32-wide k-step: 2 ds_read_b128 (16 pivots x 32 k each) -> 8 MFMAs 16x16x32 (four 16-target tiles)
// Same LDS bytes, same matrix-pipe clocks (1280 per tile), same accumulator and B-fragment register counts.
// Shapes 2 and 3 carry the REAL epilogue of nn_search_rbs_kernel (every score times a per-row weight read from LDS, strict
// compare against the running best, two selects: value and index) instead of the fmax:
//   SHAPE 3: the loop of SHAPE 1 (k-step outer, half inner), the epilogue behind the last MFMA of the tile
//   SHAPE 2: half-tile phases -- 40 MFMAs on pivot rows 0-15, then 40 on rows 16-31, the fragment reads a ring two groups
//            of four MFMAs ahead, the epilogue of one half interleaved with the MFMAs of the next (two VALU per MFMA;
//            that of rows 16-31 runs beside the NEXT tile's first phase)
//   hipcc --offload-arch=gfx950 -O3 -o nn_loop_proxy nn_loop_proxy.hip && ./nn_loop_proxy
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int SHAPE>
__global__ __launch_bounds__(256, 2) void k(const u32x4* __restrict__ src, float* out, int iters) {
    __shared__ u32x4 lds[2 * 20 * 64];   // two tile images of 20 fragments x 64 lanes x 16 B (32 pivots x 320 features)
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < 2 * 20 * 64; i += 256) lds[i] = src[i & 2047];
    __syncthreads();
    bf16x8 fb[2][20];                     // 64 targets x 320 features: 160 VGPRs
    for (int t = 0; t < 20; ++t)
        for (int j = 0; j < 2; ++j) fb[j][t] = __builtin_bit_cast(bf16x8, src[(t * 128 + j * 64 + lane + tid) & 2047]);
    float best = -1e30f;
    float bv[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
    int bi[4] = {0, 0, 0, 0};
    const int g = lane >> 4;
    const float* wl = reinterpret_cast<const float*>(lds) + 4 * g;   // 32 "inverse norms" per tile image, any finite data
    f32x4 c0[4], c1[4];
    for (int j = 0; j < 4; ++j) c1[j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    f32x4 w0, w1 = f32x4{1.f, 1.f, 1.f, 1.f};
    int row0, row1 = 0;
    bf16x8 ring[3];
    auto fold1 = [&](const f32x4 (&a)[4], const f32x4 w, const int rowb, int e) {
        const int r = e / 4, j = e % 4;
        asm volatile("" : "+v"(bv[j]), "+v"(bi[j]));
        const float sc = a[j][r] * w[r];
        if (sc > bv[j]) {
            bv[j] = sc;
            bi[j] = rowb + r;
        }
        asm volatile("" : "+v"(bv[j]), "+v"(bi[j]));
    };
    for (int it = 0; it < iters; ++it) {
        int off = (it & 1) * 1280 + lane;
        asm volatile("" : "+v"(off));
        const u32x4* f = lds + off;
        if (SHAPE == 0) {
            f32x16 a0, a1;
            for (int r = 0; r < 16; ++r) a0[r] = a1[r] = 0.f;
#pragma unroll
            for (int t = 0; t < 20; ++t) {
                const bf16x8 fa = __builtin_bit_cast(bf16x8, f[t * 64]);
                a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb[0][t], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb[1][t], a1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) best = fmaxf(best, fmaxf(a0[r], a1[r]));
        } else if (SHAPE == 2) {
            // fragment k of the tile: half i = k / 10, k-step t = k % 10 (the image keeps SHAPE 1's order (2 t + i))
            auto frag = [&](int k) { return __builtin_bit_cast(bf16x8, f[(2 * (k % 10) + k / 10) * 64]); };
            auto group = [&](int k, f32x4 (&acc)[4], const f32x4 (&accf)[4], const f32x4 wf, const int rowf) {
                const int t = k % 10;
                if (k + 2 < 20) ring[(k + 2) % 3] = frag(k + 2);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring[k % 3], fb[j & 1][2 * t + (j >> 1)],
                                                                     t == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[j], 0, 0, 0);
                if (t >= 1 && t <= 8) {
                    fold1(accf, wf, rowf, 2 * (t - 1));
                    fold1(accf, wf, rowf, 2 * (t - 1) + 1);
                }
                if (k + 2 < 20) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            const float* wt = wl + (it & 1) * 5120;
            ring[0] = frag(0);
            ring[1] = frag(1);
            w0 = *reinterpret_cast<const f32x4*>(wt);
            row0 = it * 32 + 4 * g;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 10; ++k) group(k, c0, c1, w1, row1);
            w1 = *reinterpret_cast<const f32x4*>(wt + 16);
#pragma unroll
            for (int k = 10; k < 20; ++k) group(k, c1, c0, w0, row0);
            row1 = row0 + 16;
        } else if (SHAPE == 3) {
            f32x4 a[2][4];
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 4; ++j) a[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 10; ++t) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const bf16x8 fa = __builtin_bit_cast(bf16x8, f[(2 * t + i) * 64]);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        a[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[j & 1][2 * t + (j >> 1)], a[i][j], 0, 0, 0);
                }
            }
            const float* wt = wl + (it & 1) * 5120;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(wt + 16 * i);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float sc = a[i][j][r] * w[r];
                        if (sc > bv[j]) {
                            bv[j] = sc;
                            bi[j] = it * 32 + 16 * i + 4 * g + r;
                        }
                    }
            }
        } else {
            f32x4 a[2][4];
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 4; ++j) a[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 10; ++t) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const bf16x8 fa = __builtin_bit_cast(bf16x8, f[(2 * t + i) * 64]);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        a[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[j & 1][2 * t + (j >> 1)], a[i][j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) best = fmaxf(best, a[i][j][r]);
        }
    }
    if (SHAPE == 2)
        for (int e = 0; e < 16; ++e) fold1(c1, w1, row1, e);
    for (int j = 0; j < 4; ++j) best = fmaxf(best, bv[j] + (float)bi[j]);
    out[blockIdx.x * 256 + tid] = best;
}

template <int SHAPE>
float run(const u32x4* src, float* out, int iters) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    hipLaunchKernelGGL((k<SHAPE>), dim3(512), dim3(256), 0, 0, src, out, 100);
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL((k<SHAPE>), dim3(512), dim3(256), 0, 0, src, out, iters);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    return ms;
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 60000;
    unsigned short* h = (unsigned short*)malloc(2048 * 16);
    unsigned x = 12345u;
    for (int i = 0; i < 2048 * 8; ++i) {
        x = x * 1664525u + 1013904223u;
        h[i] = (unsigned short)(((x >> 16) & 0x80ff) | 0x3f00);
    }
    u32x4* src;
    float* out;
    (void)hipMalloc(&src, 2048 * 16);
    (void)hipMemcpy(src, h, 2048 * 16, hipMemcpyHostToDevice);
    (void)hipMalloc(&out, 512 * 256 * 4);
    for (int rep = 0; rep < 2; ++rep) {
        const float t0 = run<0>(src, out, iters), t1 = run<1>(src, out, iters);
        const float t3 = run<3>(src, out, iters), t2 = run<2>(src, out, iters);
        const double fl = (double)iters * 512 * 4 * 2.0 * 32 * 64 * 320;   // per wave and tile: 32 pivots x 64 targets x 320
        printf("2 waves/SIMD, %d tiles per wave: 32x32x16 %.1f ms = %.0f TF/s | 16x16x32 %.1f ms = %.0f TF/s\n", iters, t0,
               fl / t0 / 1e9, t1, fl / t1 / 1e9);
        printf("  with the argmax epilogue: SHAPE 3 (behind the tile) %.1f ms = %.0f TF/s | SHAPE 2 (half-tile phases, ring) "
               "%.1f ms = %.0f TF/s\n", t3, fl / t3 / 1e9, t2, fl / t2 / 1e9);
    }
    return 0;
}
