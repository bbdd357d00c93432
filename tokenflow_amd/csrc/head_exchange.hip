// Pack / unpack kernels of the frames <-> heads re-sharding of the multi-GPU pivotal pass (tokenflow_amd/sharded.py).
// The reference is single-process; these have no counterpart there.  They exist so that a rank's q / k / v slabs go
// into the all-to-all send buffer, and the returned attention outputs into the [3,Kl,S,D] result, in ONE launch each
// (the torch formulation was ~10 strided copy kernels per block -- at 8 ranks more host time than the rank's GPU work).
// Pure data movement, HBM-bound: one thread = one 16-byte piece, grid-stride.
#include "tf_common.h"

namespace {

// One edit: q, k, v of its three branches less what injection leaves at home -- at most 6 slabs.  A multi-edit batch packs up
// to 6 per edit (no edit injects) and unpacks 2 per edit.  Two parameter-block sizes, so that a single edit's launches keep
// their 96-byte block and their code.
constexpr int MAX_SLABS_1 = 6;
constexpr int MAX_SLABS = 6 * TF_MAX_EDITS;

template <int N>
struct SlabPtrs {
    const unsigned char* src[N];   // pack: slab i = a [Kl, S, ld] tensor (frame stride fs[i]); unpack: dst[i]
    int64_t fs[N];                 // frame strides in BYTES
};

// send[w][f][i][s][hd] = slab_i[f][s][w*hd ...]
template <int N>
__global__ __launch_bounds__(256) void head_pack_kernel(SlabPtrs<N> sl, unsigned char* __restrict__ send, int ns, int W,
                                                        int Kl, int S, int hd_pieces, int64_t ld_bytes) {
    const int64_t total = (int64_t)W * Kl * ns * S * hd_pieces;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        int64_t t = g;
        const int pc = (int)(t % hd_pieces);
        t /= hd_pieces;
        const int s = (int)(t % S);
        t /= S;
        const int i = (int)(t % ns);
        t /= ns;
        const int f = (int)(t % Kl);
        const int w = (int)(t / Kl);
        const unsigned char* src = sl.src[i] + f * sl.fs[i] + (int64_t)s * ld_bytes + ((int64_t)w * hd_pieces + pc) * 16;
        st16(send + g * 16, ld16(src));
    }
}

// The same launch with extra workgroups behind the packing ones that compute inv_norm[r] = 1 / ||piv[r]|| of the rank's
// pivot rows (tf_pivot_inv_norm's arithmetic, one wave per row): at the coarse levels of a sharded rank a launch costs
// more than either piece of work.
template <typename T, int N>
__global__ __launch_bounds__(256) void head_pack_norm_kernel(SlabPtrs<N> sl, unsigned char* __restrict__ send, int ns, int W,
                                                             int Kl, int S, int hd_pieces, int64_t ld_bytes, int nb_pack,
                                                             const typename T::elem* __restrict__ piv,
                                                             float* __restrict__ inv_norm, int64_t rows, int D) {
    if ((int)blockIdx.x < nb_pack) {
        const int64_t total = (int64_t)W * Kl * ns * S * hd_pieces;
        for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)nb_pack * 256) {
            int64_t t = g;
            const int pc = (int)(t % hd_pieces);
            t /= hd_pieces;
            const int s = (int)(t % S);
            t /= S;
            const int i = (int)(t % ns);
            t /= ns;
            const int f = (int)(t % Kl);
            const int w = (int)(t / Kl);
            const unsigned char* src = sl.src[i] + f * sl.fs[i] + (int64_t)s * ld_bytes + ((int64_t)w * hd_pieces + pc) * 16;
            st16(send + g * 16, ld16(src));
        }
    } else {
        const int lane = threadIdx.x & 63;
        const int64_t nwaves = (int64_t)(gridDim.x - nb_pack) * 4;
        for (int64_t r = (int64_t)(blockIdx.x - nb_pack) * 4 + (threadIdx.x >> 6); r < rows; r += nwaves) {
            const float inv = tf_row_inv_norm<T>(piv + r * D, D, lane);
            if (lane == 0) inv_norm[r] = inv;
        }
    }
}

// dst_b[f][s][w*hd ...] = recv[w][f][b][s][hd]
template <int N>
__global__ __launch_bounds__(256) void head_unpack_kernel(const unsigned char* __restrict__ recv, SlabPtrs<N> sl, int nb,
                                                          int W, int Kl, int S, int hd_pieces, int64_t ld_bytes) {
    const int64_t total = (int64_t)W * Kl * nb * S * hd_pieces;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        int64_t t = g;
        const int pc = (int)(t % hd_pieces);
        t /= hd_pieces;
        const int s = (int)(t % S);
        t /= S;
        const int b = (int)(t % nb);
        t /= nb;
        const int f = (int)(t % Kl);
        const int w = (int)(t / Kl);
        unsigned char* dst = const_cast<unsigned char*>(sl.src[b]) + f * sl.fs[b] + (int64_t)s * ld_bytes +
                             ((int64_t)w * hd_pieces + pc) * 16;
        st16(dst, ld16(recv + g * 16));
    }
}

// Halo pack of a windowed frame shard (tf_window_halo_pack): the send rows of ONE tf_all_to_all_rows.  Send row r belongs to
// the segment s with row0[s] <= r < row0[s + 1] (peer order) and holds the slabs of local frame f0[s] + r - row0[s]; a frame
// several peers read lies in several segments.  The table rides in the kernel arguments: no device table, no sync, capturable.
struct HaloSegs {
    int n;                         // segments = ranks
    int row0[TF_MAX_WORLD + 1];    // first send row per segment; row0[n] = rows in all
    int f0[TF_MAX_WORLD];          // first local frame per segment
};

// send[r][i][s][0..D) = slab_i[frame(r)][s][0..D): one thread = one 16-byte piece, grid-stride over the bytes of the send buffer
template <int N>
__global__ __launch_bounds__(256) void window_halo_pack_kernel(SlabPtrs<N> sl, unsigned char* __restrict__ send, HaloSegs sg,
                                                               int ns, int S, int d_pieces, int64_t ld_bytes) {
    const int64_t per_row = (int64_t)ns * S * d_pieces;
    const int64_t total = (int64_t)sg.row0[sg.n] * per_row;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int r = (int)(g / per_row);
        int64_t t = g - (int64_t)r * per_row;
        const int pc = (int)(t % d_pieces);
        t /= d_pieces;
        const int s = (int)(t % S);
        const int i = (int)(t / S);
        int seg = 0;
        while (seg + 1 < sg.n && r >= sg.row0[seg + 1]) ++seg;
        const int f = sg.f0[seg] + (r - sg.row0[seg]);
        const unsigned char* src = sl.src[i] + f * sl.fs[i] + (int64_t)s * ld_bytes + (int64_t)pc * 16;
        st16(send + g * 16, ld16(src));
    }
}

// Halo pack of an ANCHORED windowed frame shard (tf_frame_set_halo_pack): as above, but what peer p reads of this rank is a SET
// of local frames (its window reach plus the anchors this rank owns): a 64-bit mask per peer instead of one range.  Send row r
// of segment s holds the (r - row0[s])-th member of mask[s] in ascending order.  Masks and prefix ride in the kernel arguments.
struct HaloSets {
    int n;                             // peers = ranks
    int row0[TF_MAX_WORLD + 1];        // first send row per peer; row0[n] = rows in all
    uint64_t mask[TF_MAX_WORLD];       // local frames per peer
};

// One workgroup column (blockIdx.x) = ONE send row: the peer scan and the n-th set bit are a function of blockIdx.x alone
// (wave-uniform, scalar registers, done once); the workgroups blockIdx.y .. of the row stride over its 16-byte pieces.
template <int N>
__global__ __launch_bounds__(256) void frame_set_halo_pack_kernel(SlabPtrs<N> sl, unsigned char* __restrict__ send, HaloSets sg,
                                                                  int ns, int S, int d_pieces, int64_t ld_bytes) {
    const int r = (int)blockIdx.x;
    int seg = 0;
    while (seg + 1 < sg.n && r >= sg.row0[seg + 1]) ++seg;
    uint64_t m = sg.mask[seg];
    for (int j = r - sg.row0[seg]; j > 0; --j) m &= m - 1;   // drop the j lowest members
    const int f = __builtin_ctzll(m);
    const int per_slab = S * d_pieces;
    const int64_t per_row = (int64_t)ns * per_slab;
    unsigned char* dst = send + (int64_t)r * per_row * 16;
    for (int64_t g = (int64_t)blockIdx.y * 256 + threadIdx.x; g < per_row; g += (int64_t)gridDim.y * 256) {
        const int i = (int)(g / per_slab);
        const int t = (int)(g - (int64_t)i * per_slab);
        const int s = t / d_pieces, pc = t - s * d_pieces;
        const unsigned char* src = sl.src[i] + f * sl.fs[i] + (int64_t)s * ld_bytes + (int64_t)pc * 16;
        st16(dst + g * 16, ld16(src));
    }
}

int check(const char* name, const void* const* slabs, const int64_t* fs, int n, const void* buf, int W, int Kl, int S,
          int hd, int64_t ld, int elem_bytes) {
    TF_ARG(slabs && fs && buf, TF_ERR_NULL, "%s: null pointer", name);
    TF_ARG(n >= 1 && n <= MAX_SLABS && W >= 1 && Kl >= 1 && S >= 1 && hd >= 1 && (elem_bytes == 2 || elem_bytes == 4) &&
               ((int64_t)hd * elem_bytes) % 16 == 0 && ld >= (int64_t)W * hd && ((int64_t)ld * elem_bytes) % 16 == 0,
           TF_ERR_SHAPE, "%s: n=%d W=%d Kl=%d S=%d hd=%d ld=%lld elem_bytes=%d (hd*elem_bytes and ld*elem_bytes multiples of 16)",
           name, n, W, Kl, S, hd, (long long)ld, elem_bytes);
    TF_ARG(tf_aligned16(buf), TF_ERR_ALIGN, "%s: buffer not 16-byte aligned", name);
    for (int i = 0; i < n; ++i) {
        TF_ARG(slabs[i], TF_ERR_NULL, "%s: slab %d is null", name, i);
        TF_ARG(tf_aligned16(slabs[i]) && (fs[i] * elem_bytes) % 16 == 0, TF_ERR_ALIGN, "%s: slab %d not 16-byte aligned", name, i);
    }
    return 0;
}

template <int N>
SlabPtrs<N> slab_ptrs(const void* const* slabs, const int64_t* frame_strides, int n, int elem_bytes) {
    SlabPtrs<N> sl{};
    for (int i = 0; i < n; ++i) {
        sl.src[i] = static_cast<const unsigned char*>(slabs[i]);
        sl.fs[i] = frame_strides[i] * elem_bytes;
    }
    return sl;
}

template <typename T, int N>
void launch_pack_norm(const void* const* slabs, const int64_t* frame_strides, int ns, void* send, int W, int Kl, int S,
                      int hd_pieces, int64_t ld, int elem_bytes, int64_t blocks, int64_t nblocks, const void* piv,
                      float* inv_norm, int64_t rows, int D, hipStream_t st) {
    hipLaunchKernelGGL((head_pack_norm_kernel<T, N>), dim3((unsigned)(blocks + nblocks)), dim3(256), 0, st,
                       slab_ptrs<N>(slabs, frame_strides, ns, elem_bytes), static_cast<unsigned char*>(send), ns, W, Kl, S,
                       hd_pieces, ld * elem_bytes, (int)blocks, static_cast<const typename T::elem*>(piv), inv_norm, rows, D);
}

}  // namespace

int tf_head_pack_norm(const void* const* slabs, const int64_t* frame_strides, int ns, void* send, int W, int Kl, int S,
                      int hd, int64_t ld, int elem_bytes, const void* piv, float* inv_norm, int64_t rows, int D, int dtype,
                      void* stream) {
    if (!piv) return tf_head_pack(slabs, frame_strides, ns, send, W, Kl, S, hd, ld, elem_bytes, stream);
    if (const int rc = check("tf_head_pack", slabs, frame_strides, ns, send, W, Kl, S, hd, ld, elem_bytes)) return rc;
    TF_ARG(inv_norm && rows > 0 && D > 0 && D % 8 == 0 && (dtype == TF_BF16 || dtype == TF_F16) && tf_aligned16(piv),
           TF_ERR_SHAPE, "tf_head_pack(+inverse norms): rows=%lld D=%d dtype=%d", (long long)rows, D, dtype);
    const int hd_pieces = hd * elem_bytes / 16;
    const int64_t total = (int64_t)W * Kl * ns * S * hd_pieces;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    int64_t nblocks = (rows + 3) / 4;
    if (nblocks > 4096) nblocks = 4096;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    auto go = ns <= MAX_SLABS_1 ? (dtype == TF_BF16 ? launch_pack_norm<BF16, MAX_SLABS_1> : launch_pack_norm<F16, MAX_SLABS_1>)
                                : (dtype == TF_BF16 ? launch_pack_norm<BF16, MAX_SLABS> : launch_pack_norm<F16, MAX_SLABS>);
    go(slabs, frame_strides, ns, send, W, Kl, S, hd_pieces, ld, elem_bytes, blocks, nblocks, piv, inv_norm, rows, D, st);
    TF_LAUNCH_CHECK("tf_head_pack");
    return 0;
}

extern "C" int tf_head_pack(const void* const* slabs, const int64_t* frame_strides, int ns, void* send, int W, int Kl,
                            int S, int hd, int64_t ld, int elem_bytes, void* stream) {
    if (const int rc = check("tf_head_pack", slabs, frame_strides, ns, send, W, Kl, S, hd, ld, elem_bytes)) return rc;
    const int hd_pieces = hd * elem_bytes / 16;
    const int64_t total = (int64_t)W * Kl * ns * S * hd_pieces;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (ns <= MAX_SLABS_1)
        hipLaunchKernelGGL(head_pack_kernel<MAX_SLABS_1>, dim3((unsigned)blocks), dim3(256), 0, st,
                           slab_ptrs<MAX_SLABS_1>(slabs, frame_strides, ns, elem_bytes), static_cast<unsigned char*>(send), ns,
                           W, Kl, S, hd_pieces, ld * elem_bytes);
    else
        hipLaunchKernelGGL(head_pack_kernel<MAX_SLABS>, dim3((unsigned)blocks), dim3(256), 0, st,
                           slab_ptrs<MAX_SLABS>(slabs, frame_strides, ns, elem_bytes), static_cast<unsigned char*>(send), ns, W,
                           Kl, S, hd_pieces, ld * elem_bytes);
    TF_LAUNCH_CHECK("tf_head_pack");
    return 0;
}

extern "C" int tf_head_unpack(const void* recv, void* const* dsts, const int64_t* frame_strides, int nb, int W, int Kl,
                              int S, int hd, int64_t ld, int elem_bytes, void* stream) {
    if (const int rc = check("tf_head_unpack", const_cast<const void* const*>(dsts), frame_strides, nb, recv, W, Kl, S, hd,
                             ld, elem_bytes))
        return rc;
    const int hd_pieces = hd * elem_bytes / 16;
    const int64_t total = (int64_t)W * Kl * nb * S * hd_pieces;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const void* const* dptrs = const_cast<const void* const*>(dsts);
    if (nb <= MAX_SLABS_1)
        hipLaunchKernelGGL(head_unpack_kernel<MAX_SLABS_1>, dim3((unsigned)blocks), dim3(256), 0, st,
                           static_cast<const unsigned char*>(recv), slab_ptrs<MAX_SLABS_1>(dptrs, frame_strides, nb, elem_bytes),
                           nb, W, Kl, S, hd_pieces, ld * elem_bytes);
    else
        hipLaunchKernelGGL(head_unpack_kernel<MAX_SLABS>, dim3((unsigned)blocks), dim3(256), 0, st,
                           static_cast<const unsigned char*>(recv), slab_ptrs<MAX_SLABS>(dptrs, frame_strides, nb, elem_bytes),
                           nb, W, Kl, S, hd_pieces, ld * elem_bytes);
    TF_LAUNCH_CHECK("tf_head_unpack");
    return 0;
}

// One launch packs the bank slabs of the local keyframes that peers read into the send buffer of one tf_all_to_all_rows
// (include/tokenflow_hip.h).  Pure data movement; every argument is checked before anything touches the device.
extern "C" int tf_window_halo_pack(const void* const* slabs, const int64_t* frame_strides, int ns, void* send, int n_seg,
                                   const int* seg_f0, const int* seg_n, int Kl, int S, int D, int64_t ld, int dtype,
                                   void* stream) {
    const char* const name = "tf_window_halo_pack";
    TF_ARG(slabs && frame_strides && send && seg_f0 && seg_n, TF_ERR_NULL, "%s: null pointer", name);
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "%s: dtype %d (bf16/f16 only)", name, dtype);
    TF_ARG(ns >= 1 && ns <= MAX_SLABS_1 && n_seg >= 1 && n_seg <= TF_MAX_WORLD && Kl >= 1 && S >= 1 && D >= 8 && D % 8 == 0 &&
               ld >= D && ld % 8 == 0,
           TF_ERR_SHAPE, "%s: ns=%d segments=%d Kl=%d S=%d D=%d ld=%lld (D and ld multiples of 8 elements, ld >= D, at most %d "
           "slabs and %d segments)", name, ns, n_seg, Kl, S, D, (long long)ld, MAX_SLABS_1, TF_MAX_WORLD);
    HaloSegs sg{};
    sg.n = n_seg;
    int64_t rows = 0;
    for (int p = 0; p < n_seg; ++p) {
        TF_ARG(seg_n[p] >= 0 && seg_f0[p] >= 0 && (int64_t)seg_f0[p] + seg_n[p] <= Kl, TF_ERR_SHAPE,
               "%s: segment %d = local frames [%d, %d) outside the %d local keyframes", name, p, seg_f0[p], seg_f0[p] + seg_n[p], Kl);
        sg.row0[p] = (int)rows, sg.f0[p] = seg_f0[p];
        rows += seg_n[p];
    }
    TF_ARG(rows < (1 << 16), TF_ERR_SHAPE, "%s: %lld send rows (below 65536)", name, (long long)rows);
    sg.row0[n_seg] = (int)rows;
    TF_ARG(tf_aligned16(send), TF_ERR_ALIGN, "%s: send buffer not 16-byte aligned", name);
    for (int i = 0; i < ns; ++i) {
        TF_ARG(slabs[i], TF_ERR_NULL, "%s: slab %d is null", name, i);
        TF_ARG(tf_aligned16(slabs[i]) && (frame_strides[i] * 2) % 16 == 0, TF_ERR_ALIGN, "%s: slab %d not 16-byte aligned", name, i);
        // (a frame holds S token rows: the last byte read is inside the slab's Kl frames)
        TF_ARG(frame_strides[i] >= (int64_t)(S - 1) * ld + D || Kl == 1, TF_ERR_SHAPE, "%s: slab %d: frame stride %lld below a frame",
               name, i, (long long)frame_strides[i]);
    }
    if (rows == 0) return 0;   // nobody reads this rank's frames and it sends none to itself: nothing to launch
    const int d_pieces = D * 2 / 16;
    const int64_t total = rows * ns * S * d_pieces;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;   // 256 CUs x 8 resident workgroups; the rest by the grid stride
    hipLaunchKernelGGL(window_halo_pack_kernel<MAX_SLABS_1>, dim3((unsigned)blocks), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), slab_ptrs<MAX_SLABS_1>(slabs, frame_strides, ns, 2),
                       static_cast<unsigned char*>(send), sg, ns, S, d_pieces, ld * 2);
    TF_LAUNCH_CHECK("tf_window_halo_pack");
    return 0;
}

// The same packing where what a peer reads is a SET of local frames (include/tokenflow_hip.h): an anchored windowed frame shard.
extern "C" int tf_frame_set_halo_pack(const void* const* slabs, const int64_t* frame_strides, int ns, void* send, int n_peer,
                                      const uint64_t* masks, int Kl, int S, int D, int64_t ld, int dtype, void* stream) {
    const char* const name = "tf_frame_set_halo_pack";
    TF_ARG(slabs && frame_strides && send && masks, TF_ERR_NULL, "%s: null pointer", name);
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "%s: dtype %d (bf16/f16 only)", name, dtype);
    TF_ARG(ns >= 1 && ns <= MAX_SLABS_1 && n_peer >= 1 && n_peer <= TF_MAX_WORLD && Kl >= 1 && Kl <= 64 && S >= 1 && D >= 8 &&
               D % 8 == 0 && ld >= D && ld % 8 == 0 && (int64_t)S * (D / 8) < ((int64_t)1 << 30),
           TF_ERR_SHAPE, "%s: ns=%d peers=%d Kl=%d S=%d D=%d ld=%lld (D and ld multiples of 8 elements, ld >= D, at most %d "
           "slabs, %d peers and 64 local frames)", name, ns, n_peer, Kl, S, D, (long long)ld, MAX_SLABS_1, TF_MAX_WORLD);
    HaloSets sg{};
    sg.n = n_peer;
    int rows = 0;
    for (int p = 0; p < n_peer; ++p) {
        TF_ARG(Kl == 64 || !(masks[p] >> Kl), TF_ERR_SHAPE, "%s: mask %d = 0x%llx has bits at or above the %d local keyframes", name,
               p, (unsigned long long)masks[p], Kl);
        sg.row0[p] = rows, sg.mask[p] = masks[p];
        rows += __builtin_popcountll(masks[p]);
    }
    sg.row0[n_peer] = rows;
    TF_ARG(tf_aligned16(send), TF_ERR_ALIGN, "%s: send buffer not 16-byte aligned", name);
    for (int i = 0; i < ns; ++i) {
        TF_ARG(slabs[i], TF_ERR_NULL, "%s: slab %d is null", name, i);
        TF_ARG(tf_aligned16(slabs[i]) && (frame_strides[i] * 2) % 16 == 0, TF_ERR_ALIGN, "%s: slab %d not 16-byte aligned", name, i);
        // (a frame holds S token rows: the last byte read is inside the slab's Kl frames)
        TF_ARG(frame_strides[i] >= (int64_t)(S - 1) * ld + D || Kl == 1, TF_ERR_SHAPE, "%s: slab %d: frame stride %lld below a frame",
               name, i, (long long)frame_strides[i]);
    }
    if (rows == 0) return 0;   // nobody reads this rank's frames and it sends none to itself: nothing to launch
    const int d_pieces = D * 2 / 16;
    const int64_t per_row = (int64_t)ns * S * d_pieces;
    // about 2048 workgroups in all (256 CUs x 8 resident), at least one and at most a row's worth per send row (rows <= 4096)
    int64_t ny = (2048 + rows - 1) / rows;
    if (ny > (per_row + 255) / 256) ny = (per_row + 255) / 256;
    hipLaunchKernelGGL(frame_set_halo_pack_kernel<MAX_SLABS_1>, dim3((unsigned)rows, (unsigned)ny), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), slab_ptrs<MAX_SLABS_1>(slabs, frame_strides, ns, 2),
                       static_cast<unsigned char*>(send), sg, ns, S, d_pieces, ld * 2);
    TF_LAUNCH_CHECK("tf_frame_set_halo_pack");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Halo pack of a windowed / anchored frame shard that carries a MULTI-EDIT batch (tf_edit_halo_pack): the work of
// tf_frame_set_halo_pack -- per peer a 64-bit mask over the local frames, send rows in ascending member order -- for up to
// 4 * TF_MAX_EDITS slabs (the compact k slots and two value slabs per edit), and, in extra workgroup columns behind the packing
// ones (as head_pack_norm_kernel appends its norm workgroups), the copy of nq compact q slabs into a dense staging region
// [nq][Kl][S][D]: a mixed injection mask reads the source's q beside the non-injecting edits' and the part call addresses them
// with ONE branch stride.  A plain window's ranges are contiguous masks, so this one entry serves both passes.
namespace {

constexpr int MAX_SLABS_E = 4 * TF_MAX_EDITS;
constexpr int MAX_Q_SLABS = 1 + 2 * TF_MAX_EDITS;

// Column blockIdx.x < rows: ONE send row, as frame_set_halo_pack_kernel.  Column rows + c: frame c % Kl of q slab c / Kl.
__global__ __launch_bounds__(256) void edit_halo_pack_kernel(SlabPtrs<MAX_SLABS_E> sl, unsigned char* __restrict__ send, HaloSets sg,
                                                             int ns, int S, int d_pieces, int64_t ld_bytes,
                                                             SlabPtrs<MAX_Q_SLABS> ql, unsigned char* __restrict__ q_stage, int Kl,
                                                             int64_t ld_q_bytes) {
    const int rows = sg.row0[sg.n];
    const int per_slab = S * d_pieces;
    if ((int)blockIdx.x >= rows) {
        const int c = (int)blockIdx.x - rows;
        const int i = c / Kl, f = c - i * Kl;
        const unsigned char* src = ql.src[i] + f * ql.fs[i];
        unsigned char* dst = q_stage + (int64_t)c * per_slab * 16;
        for (int t = (int)blockIdx.y * 256 + threadIdx.x; t < per_slab; t += (int)gridDim.y * 256) {
            const int s = t / d_pieces, pc = t - s * d_pieces;
            st16(dst + (int64_t)t * 16, ld16(src + (int64_t)s * ld_q_bytes + (int64_t)pc * 16));
        }
        return;
    }
    const int r = (int)blockIdx.x;
    int seg = 0;
    while (seg + 1 < sg.n && r >= sg.row0[seg + 1]) ++seg;
    uint64_t m = sg.mask[seg];
    for (int j = r - sg.row0[seg]; j > 0; --j) m &= m - 1;   // drop the j lowest members
    const int f = __builtin_ctzll(m);
    const int64_t per_row = (int64_t)ns * per_slab;
    unsigned char* dst = send + (int64_t)r * per_row * 16;
    for (int64_t g = (int64_t)blockIdx.y * 256 + threadIdx.x; g < per_row; g += (int64_t)gridDim.y * 256) {
        const int i = (int)(g / per_slab);
        const int t = (int)(g - (int64_t)i * per_slab);
        const int s = t / d_pieces, pc = t - s * d_pieces;
        const unsigned char* src = sl.src[i] + f * sl.fs[i] + (int64_t)s * ld_bytes + (int64_t)pc * 16;
        st16(dst + g * 16, ld16(src));
    }
}

}  // namespace

extern "C" int tf_edit_halo_pack(const void* const* slabs, const int64_t* frame_strides, int ns, void* send, int n_peer,
                                 const uint64_t* masks, const void* const* q_slabs, const int64_t* q_frame_strides, int nq,
                                 void* q_stage, int Kl, int S, int D, int64_t ld, int64_t ld_q, int dtype, void* stream) {
    const char* const name = "tf_edit_halo_pack";
    TF_ARG(slabs && frame_strides && send && masks, TF_ERR_NULL, "%s: null pointer", name);
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "%s: dtype %d (bf16/f16 only)", name, dtype);
    TF_ARG(ns >= 1 && ns <= MAX_SLABS_E && n_peer >= 1 && n_peer <= TF_MAX_WORLD && Kl >= 1 && Kl <= 64 && S >= 1 && D >= 8 &&
               D % 8 == 0 && ld >= D && ld % 8 == 0 && (int64_t)S * (D / 8) < ((int64_t)1 << 30),
           TF_ERR_SHAPE, "%s: ns=%d peers=%d Kl=%d S=%d D=%d ld=%lld (D and ld multiples of 8 elements, ld >= D, at most %d "
           "slabs, %d peers and 64 local frames)", name, ns, n_peer, Kl, S, D, (long long)ld, MAX_SLABS_E, TF_MAX_WORLD);
    TF_ARG(nq >= 0 && nq <= MAX_Q_SLABS, TF_ERR_SHAPE, "%s: nq=%d (0 .. %d compact q slabs)", name, nq, MAX_Q_SLABS);
    HaloSets sg{};
    sg.n = n_peer;
    int rows = 0;
    for (int p = 0; p < n_peer; ++p) {
        TF_ARG(Kl == 64 || !(masks[p] >> Kl), TF_ERR_SHAPE, "%s: mask %d = 0x%llx has bits at or above the %d local keyframes", name,
               p, (unsigned long long)masks[p], Kl);
        sg.row0[p] = rows, sg.mask[p] = masks[p];
        rows += __builtin_popcountll(masks[p]);
    }
    sg.row0[n_peer] = rows;
    TF_ARG(tf_aligned16(send), TF_ERR_ALIGN, "%s: send buffer not 16-byte aligned", name);
    for (int i = 0; i < ns; ++i) {
        TF_ARG(slabs[i], TF_ERR_NULL, "%s: slab %d is null", name, i);
        TF_ARG(tf_aligned16(slabs[i]) && (frame_strides[i] * 2) % 16 == 0, TF_ERR_ALIGN, "%s: slab %d not 16-byte aligned", name, i);
        // (a frame holds S token rows: the last byte read is inside the slab's Kl frames)
        TF_ARG(frame_strides[i] >= (int64_t)(S - 1) * ld + D || Kl == 1, TF_ERR_SHAPE, "%s: slab %d: frame stride %lld below a frame",
               name, i, (long long)frame_strides[i]);
    }
    if (nq) {
        TF_ARG(q_slabs && q_frame_strides && q_stage, TF_ERR_NULL, "%s: null q pointer", name);
        TF_ARG(ld_q >= D && ld_q % 8 == 0, TF_ERR_SHAPE, "%s: ld_q=%lld (a multiple of 8 elements, >= D)", name, (long long)ld_q);
        TF_ARG(tf_aligned16(q_stage), TF_ERR_ALIGN, "%s: q staging region not 16-byte aligned", name);
        for (int i = 0; i < nq; ++i) {
            TF_ARG(q_slabs[i], TF_ERR_NULL, "%s: q slab %d is null", name, i);
            TF_ARG(tf_aligned16(q_slabs[i]) && (q_frame_strides[i] * 2) % 16 == 0, TF_ERR_ALIGN, "%s: q slab %d not 16-byte aligned",
                   name, i);
            TF_ARG(q_frame_strides[i] >= (int64_t)(S - 1) * ld_q + D || Kl == 1, TF_ERR_SHAPE,
                   "%s: q slab %d: frame stride %lld below a frame", name, i, (long long)q_frame_strides[i]);
        }
    }
    const int cols = rows + nq * Kl;
    if (cols == 0) return 0;   // nobody reads this rank's frames, it sends none to itself and stages no q: nothing to launch
    const int d_pieces = D * 2 / 16;
    const int64_t per_row = (int64_t)ns * S * d_pieces;
    // about 2048 workgroups in all (256 CUs x 8 resident), at least one and at most a row's worth per column
    int64_t ny = (2048 + cols - 1) / cols;
    if (ny > (per_row + 255) / 256) ny = (per_row + 255) / 256;
    SlabPtrs<MAX_Q_SLABS> ql{};
    if (nq) ql = slab_ptrs<MAX_Q_SLABS>(q_slabs, q_frame_strides, nq, 2);
    hipLaunchKernelGGL(edit_halo_pack_kernel, dim3((unsigned)cols, (unsigned)ny), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), slab_ptrs<MAX_SLABS_E>(slabs, frame_strides, ns, 2),
                       static_cast<unsigned char*>(send), sg, ns, S, d_pieces, ld * 2, ql, static_cast<unsigned char*>(q_stage), Kl,
                       ld_q * 2);
    TF_LAUNCH_CHECK("tf_edit_halo_pack");
    return 0;
}
