// One rank's pivotal pass of a transformer block in a frame-sharded multi-GPU run, issued by ONE host call.
//
// The reference is single-process; tokenflow_amd/sharded.py describes the partitioning
// (tokenflow_utils.py:133-138: every keyframe's queries read the keys / values of ALL K keyframes; 331-333: chunk c
// reads keyframes c and c-1) and is the Python form of the same sequence.  This file is that sequence as native
// code: the per-block work of a rank at 8 GPUs is a dozen launches of 5..500 us with three exchanges between them,
// and a Python host spends 200-300 us per block issuing them (profiles/r03_rank_step_v2.txt) -- more than the GPU
// needs for the block at three of the four UNet levels.  Here the host cost is one foreign call.
//
// Streams: the caller's stream carries the compute AND every collective of the pivotal pass's communicator (one
// communicator, one stream: no reliance on cross-stream ordering inside RCCL; a hand-over between two streams on the
// critical path also costs ~10 us of idle device each way, profiles/r04_rank_timeline_v1.txt).  Two side streams:
// an auxiliary COMPUTE stream runs the source branch of the local frames beside the first exchange and the bank
// attention where those are separate launches (level 0; forked behind the pack -- in FRONT of the exchange -- and joined
// in front of the second exchange by events, nothing waits on it before the join), and the neighbour halo has a stream of its own (with its own communicator when the host gives one:
// collectives of ONE RCCL communicator execute in issue order, and a 10 MB halo message in front of the next block's
// all-to-all would sit on the critical path); it has the rest of the pass to arrive.  All ordering is by events; no
// host synchronisation anywhere.
// TF_RANK_BANK_RUNS uses the same auxiliary compute stream for the LOCAL run of the bank (the rank's own keyframes: source
// branch + bank branches, forked behind the pack and in front of the gather, joined in front of the merge).
#include <stdio.h>
#include <stdlib.h>

#include <new>

#include "attn_fused.h"
#include "tf_common.h"

struct tf_comm;   // csrc/comm.hip

namespace {

constexpr int RING = 64;

int hip_fail(const char* what, hipError_t e) {
    tf_set_error("%s: %s", what, hipGetErrorString(e));
    return (int)e;
}
#define TF_HIP(call, what)                                   \
    do {                                                     \
        const hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) return hip_fail(what, e_);     \
    } while (0)

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

struct tf_rank {
    tf_comm* comm;
    tf_comm* halo_comm;
    int K, world, rank, Kl, kf0;
    int counts[TF_MAX_WORLD];
    hipStream_t hs = nullptr;   // neighbour halo
    hipStream_t as = nullptr;   // auxiliary COMPUTE stream: the source branch beside the exchange and the bank launch
    hipEvent_t ring[RING];
    int ring_i = 0;
    hipEvent_t halo_done[TF_RANK_SLOTS];
    bool halo_set[TF_RANK_SLOTS];

    hipEvent_t next() {
        hipEvent_t e = ring[ring_i];
        ring_i = (ring_i + 1) % RING;
        return e;
    }
};

namespace {

// `to` continues after everything enqueued on `from` so far.  Events are reused: a wait captures the record that is
// current when it is issued (HIP semantics), and 64 events outlast any hand-over of a block.
int order(tf_rank* rk, hipStream_t from, hipStream_t to, const char* what) {
    if (tf_plan_rec) return 0;   // plan recording: no streams to order
    hipEvent_t e = rk->next();
    TF_HIP(hipEventRecord(e, from), what);
    TF_HIP(hipStreamWaitEvent(to, e, 0), what);
    return 0;
}

struct Layout {   // exchange buffers of one call inside the caller's workspace
    size_t send, recv, send2, recv2, ws_bank, ws_src, total;
    size_t ws_bank_bytes, ws_src_bytes;
};

// TF_RANK_BANK_RUNS: the runs of the bank a rank computes, in SLOT order -- its own keyframes, the frames to their left, the
// frames to their right (the empty ones dropped).  The order fixes the arithmetic of the merge, whatever the schedule.
struct Runs {
    int n, f0[3], len[3];
};
Runs rank_runs(const tf_rank* rk) {
    Runs r{};
    r.f0[r.n] = rk->kf0, r.len[r.n] = rk->Kl, ++r.n;
    if (rk->kf0 > 0) r.f0[r.n] = 0, r.len[r.n] = rk->kf0, ++r.n;
    if (rk->kf0 + rk->Kl < rk->K) r.f0[r.n] = rk->kf0 + rk->Kl, r.len[r.n] = rk->K - rk->kf0 - rk->Kl, ++r.n;
    return r;
}

Layout layout(const tf_rank* rk, int S, int H, int Dh, int dtype, int mode) {
    const size_t eb = 2;
    const int W = rk->world, Kl = rk->Kl, K = rk->K;
    const size_t D = (size_t)H * Dh;
    Layout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += up256(bytes);
        return at;
    };
    if (mode == TF_RANK_HEADS) {
        const size_t hd = D / W;
        L.send = take((size_t)W * Kl * 6 * S * hd * eb);
        L.recv = take((size_t)K * 6 * S * hd * eb);
        L.send2 = take((size_t)K * 2 * S * hd * eb);
        L.recv2 = take((size_t)W * Kl * 2 * S * hd * eb);
        L.ws_bank_bytes = tf_ext_attn_workspace_bytes(K, S, H / W, Dh, dtype);
        L.ws_src_bytes = tf_ext_attn_workspace_bytes(Kl, S, H, Dh, dtype);
        L.ws_bank = take(L.ws_bank_bytes);
        L.ws_src = take(L.ws_src_bytes);
    } else if (mode == TF_RANK_BANK_RUNS) {
        // only what peers read travels: [k1, k2, v1, v2], under injection [k0, v1, v2] (sized for the former)
        L.send = take((size_t)Kl * 4 * S * D * eb);
        L.recv = take((size_t)K * 4 * S * D * eb);
        L.ws_bank_bytes = tf_ext_attn_runs_workspace_bytes(K, Kl, S, H, Dh, rank_runs(rk).n, dtype);
        L.ws_bank = take(L.ws_bank_bytes);
    } else {
        L.send = take((size_t)Kl * 6 * S * D * eb);
        L.recv = take((size_t)K * 6 * S * D * eb);
        L.ws_bank_bytes = tf_ext_attn_workspace_bytes(K, S, H, Dh, dtype);
        L.ws_bank = take(L.ws_bank_bytes);
    }
    L.total = off;
    return L;
}

// ---- the steps of a pass behind the record switch of the plan query (tf_rank_pivotal_edits_plan): while a recorder is set
//      on the calling thread every step appends its token and touches no device, stream or communicator -- the attention entry
//      points do the same for their launches -- so the plan is recorded by the code that runs, not by a copy of it.
int do_pack(const void* const* slabs, const int64_t* fss, int ns, void* send, int W, int Kl, int S, int hd, int64_t ld,
            const void* piv, float* inv, int64_t rows, int D, int dtype, void* stream) {
    if (piv ? tf_plan_note("pack+inv[ns=%d]", ns) : tf_plan_note("pack[ns=%d]", ns)) return 0;
    return tf_head_pack_norm(slabs, fss, ns, send, W, Kl, S, hd, ld, 2, piv, inv, rows, D, dtype, stream);
}
int do_unpack(const void* recv, void* const* dsts, const int64_t* dfs, int nb, int W, int Kl, int S, int hd, int64_t ld,
              void* stream) {
    if (tf_plan_note("unpack[nb=%d]", nb)) return 0;
    return tf_head_unpack(recv, dsts, dfs, nb, W, Kl, S, hd, ld, 2, stream);
}
int do_a2a(tf_comm* comm, const void* send, void* recv, const int64_t* send_rows, const int64_t* recv_rows, int slabs,
           int64_t slab_elems, int dtype, void* stream) {
    if (tf_plan_note("a2a[slabs=%d]", slabs)) return 0;
    return tf_all_to_all_rows(comm, send, recv, send_rows, recv_rows, slabs * slab_elems, dtype, stream);
}
int do_gather(tf_comm* comm, const void* send, void* recv, const int64_t* rows, int slabs, int64_t slab_elems, int dtype,
              void* stream) {
    if (tf_plan_note("gather[slabs=%d]", slabs)) return 0;
    return tf_allgather_rows(comm, send, recv, rows, slabs * slab_elems, dtype, stream);
}
int do_inv_norm(const void* piv, float* inv, int64_t rows, int D, int dtype, void* stream) {
    if (tf_plan_note("inv_norm")) return 0;
    return tf_pivot_inv_norm(piv, inv, rows, D, dtype, stream);
}

// TOKENFLOW_RANK_SRC_AUX=0: the source part in line on the caller's stream instead of the auxiliary compute stream
bool src_aux_enabled() {
    static const bool on = [] { const char* e = getenv("TOKENFLOW_RANK_SRC_AUX"); return !e || atoi(e) != 0; }();
    return on;
}

// ---- neighbour halo: the last local keyframe's pivots, inverse norms and the `nbr` branches of the attention output -> slot 0
//      of rank r+1, ONE grouped exchange of 2 + nbr messages on the halo stream (the entry point moves bytes: the 16-bit rows
//      are counted as SD/2 four-byte elements next to the fp32 inverse norms; S*D is even, D being a multiple of 8)
int halo_exchange(tf_rank* rk, unsigned short* piv, float* inv_ext, unsigned short* kfo, int nbr, int64_t o_bs, int64_t SD,
                  int S, int slot, hipStream_t st, const char* fn) {
    const int W = rk->world, Kl = rk->Kl;
    const int to = rk->rank + 1 < W ? rk->rank + 1 : -1, from = rk->rank > 0 ? rk->rank - 1 : -1;
    if (to < 0 && from < 0) return 0;
    constexpr int MAXM = 3 + 2 * TF_MAX_EDITS;
    const int n = 2 + nbr;
    if (tf_plan_note("halo[n=%d]", n)) return 0;
    if (const int rc = order(rk, st, rk->hs, fn)) return rc;
    const void* snd[MAXM];
    void* rcv[MAXM];
    int64_t n32[MAXM];
    snd[0] = piv + (int64_t)Kl * SD, rcv[0] = piv, n32[0] = SD / 2;
    for (int b = 0; b < nbr; ++b)
        snd[1 + b] = kfo + b * o_bs + (int64_t)Kl * SD, rcv[1 + b] = kfo + b * o_bs, n32[1 + b] = SD / 2;
    snd[n - 1] = inv_ext + (int64_t)Kl * S, rcv[n - 1] = inv_ext, n32[n - 1] = S;
    if (const int rc = tf_sendrecv_pivot(rk->halo_comm, snd, n32, n, to, rcv, n32, n, from, TF_F32, rk->hs)) return rc;
    TF_HIP(hipEventRecord(rk->halo_done[slot], rk->hs), fn);
    rk->halo_set[slot] = true;
    return 0;
}

// contiguous runs of the K keyframes, the first K % W ranks hold one more (sharded.py)
void partition(tf_rank* rk, int K, int world, int rank) {
    rk->K = K, rk->world = world, rk->rank = rank;
    int off = 0;
    for (int r = 0; r < world; ++r) {
        rk->counts[r] = K / world + (r < K % world ? 1 : 0);
        if (r == rank) rk->kf0 = off;
        off += rk->counts[r];
    }
    rk->Kl = rk->counts[rank];
}

// ---- sliding-window bank on a frame shard (tf_rank_pivotal_window): what `sharded.window_halo_plan` computes in Python.
//      With radius R rank r reads the global frames [lo, hi) = [max(0, kf0 - R), min(K, kf0 + Kl + R)): hl = kf0 - lo halo
//      frames on the left, hr on the right, F in all.  Peer p sends it own(p) & [lo, hi) -- several ranks' worth for R > Kl --
//      and it sends peer p own(r) & [lo_p, hi_p); its own frames travel as its self rows, so that the receive buffer IS the
//      extended bank in ascending global frame order.  Local query i (global g = kf0 + i) gets the window of g shifted by -lo.
struct WinGeom {
    int lo, hi, hl, hr, F;
    int seg_f0[TF_MAX_WORLD], seg_n[TF_MAX_WORLD];   // per peer: the local frames it reads (first, count)
    int64_t send_rows[TF_MAX_WORLD], recv_rows[TF_MAX_WORLD];
    int64_t send_total;
    int win_lo[TF_MAX_WINDOW_FRAMES], win_n[TF_MAX_WINDOW_FRAMES];
};

inline int imax(int a, int b) { return a > b ? a : b; }
inline int imin(int a, int b) { return a < b ? a : b; }

// (Kl <= TF_MAX_WINDOW_FRAMES is the caller's check: the window table holds one entry per local keyframe)
WinGeom window_geometry(const tf_rank* rk, int R) {
    WinGeom g{};
    const int K = rk->K, Kl = rk->Kl, kf0 = rk->kf0;
    const int64_t Rl = R;   // (a radius near INT_MAX must not overflow the sums)
    g.lo = (int)(kf0 - Rl > 0 ? kf0 - Rl : 0);
    g.hi = (int)(kf0 + Kl + Rl < K ? kf0 + Kl + Rl : K);
    g.hl = kf0 - g.lo, g.hr = g.hi - kf0 - Kl, g.F = g.hi - g.lo;
    int off = 0;
    for (int p = 0; p < rk->world; ++p) {
        const int p0 = off, p1 = off + rk->counts[p];
        off = p1;
        // what arrives from p: own(p) & [lo, hi)
        const int a = imax(p0, g.lo), b = imin(p1, g.hi);
        g.recv_rows[p] = b > a ? b - a : 0;
        // what goes to p: own(r) & [lo_p, hi_p)
        const int lo_p = (int)(p0 - Rl > 0 ? p0 - Rl : 0), hi_p = (int)(p1 + Rl < K ? p1 + Rl : K);
        const int c = imax(kf0, lo_p), d = imin(kf0 + Kl, hi_p);
        g.seg_n[p] = d > c ? d - c : 0;
        g.seg_f0[p] = d > c ? c - kf0 : 0;
        g.send_rows[p] = g.seg_n[p];
        g.send_total += g.seg_n[p];
    }
    for (int i = 0; i < Kl && i < TF_MAX_WINDOW_FRAMES; ++i) {
        const int64_t gi = kf0 + i;
        const int w0 = (int)(gi - Rl > 0 ? gi - Rl : 0), w1 = (int)(gi + Rl < K - 1 ? gi + Rl : K - 1);
        g.win_lo[i] = w0 - g.lo, g.win_n[i] = w1 - w0 + 1;
    }
    return g;
}

struct WinLayout {   // exchange buffers of one windowed call inside the caller's workspace
    size_t send, recv, ws_bank, ws_src, total;
    size_t ws_bank_bytes, ws_src_bytes;
};

WinLayout window_layout(const tf_rank* rk, const WinGeom& g, int S, int H, int Dh, int dtype) {
    const size_t eb = 2, D = (size_t)H * Dh;
    WinLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += up256(bytes);
        return at;
    };
    // only what peers read travels: [k1, k2, v1, v2], under injection [k0, v1, v2] (sized for the former)
    L.send = take((size_t)g.send_total * 4 * S * D * eb);
    L.recv = take((size_t)g.F * 4 * S * D * eb);
    // the bank part and the source part may run concurrently: a workspace each
    L.ws_bank_bytes = tf_ext_attn_workspace_bytes(g.F, S, H, Dh, dtype);
    L.ws_src_bytes = tf_ext_attn_workspace_bytes(rk->Kl, S, H, Dh, dtype);
    L.ws_bank = take(L.ws_bank_bytes);
    L.ws_src = take(L.ws_src_bytes);
    L.total = off;
    return L;
}

int do_halo_pack(const void* const* slabs, const int64_t* fss, int ns, void* send, const tf_rank* rk, const WinGeom& g, int S,
                 int D, int64_t ld, int dtype, void* stream) {
    if (tf_plan_note("halo_pack[ns=%d]", ns)) return 0;
    return tf_window_halo_pack(slabs, fss, ns, send, rk->world, g.seg_f0, g.seg_n, rk->Kl, S, D, ld, dtype, stream);
}

// the sparse exchange: its plan token lists the rows per peer, out and in ("/"-separated, rank order)
int do_a2a_rows(const tf_rank* rk, const void* send, void* recv, const WinGeom& g, int slabs, int64_t slab_elems, int dtype,
                void* stream) {
    if (tf_plan_rec) {
        char out[4 * TF_MAX_WORLD + 8], in[4 * TF_MAX_WORLD + 8];
        size_t no = 0, ni = 0;
        for (int p = 0; p < rk->world; ++p) {
            no += (size_t)snprintf(out + no, sizeof(out) - no, p ? "/%d" : "%d", (int)g.send_rows[p]);
            ni += (size_t)snprintf(in + ni, sizeof(in) - ni, p ? "/%d" : "%d", (int)g.recv_rows[p]);
        }
        tf_plan_note("a2a[slabs=%d,send=%s,recv=%s]", slabs, out, in);
        return 0;
    }
    return tf_all_to_all_rows(rk->comm, send, recv, g.send_rows, g.recv_rows, slabs * slab_elems, dtype, stream);
}

}  // namespace

extern "C" int tf_rank_create(tf_comm* comm, tf_comm* halo_comm, int K, tf_rank** out) {
    TF_ARG(out, TF_ERR_NULL, "tf_rank_create: null pointer");
    const int world = comm ? tf_comm_world(comm) : 1, rank = comm ? tf_comm_rank(comm) : 0;
    TF_ARG(world >= 1 && world <= TF_MAX_WORLD && K >= world, TF_ERR_SHAPE,
           "tf_rank_create: %d keyframes over %d ranks (every rank owns at least one; at most %d ranks)", K, world,
           TF_MAX_WORLD);
    TF_ARG(!halo_comm || (tf_comm_world(halo_comm) == world && tf_comm_rank(halo_comm) == rank), TF_ERR_SHAPE,
           "tf_rank_create: the halo communicator must have the same rank and world");
    tf_rank* rk = new (std::nothrow) tf_rank();
    TF_ARG(rk, TF_ERR_NULL, "tf_rank_create: out of memory");
    rk->comm = comm;
    rk->halo_comm = halo_comm ? halo_comm : comm;
    partition(rk, K, world, rank);
    for (int i = 0; i < TF_RANK_SLOTS; ++i) rk->halo_set[i] = false, rk->halo_done[i] = nullptr;
    for (int i = 0; i < RING; ++i) rk->ring[i] = nullptr;
    hipError_t e = hipSuccess;
    for (int i = 0; i < RING && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&rk->ring[i], hipEventDisableTiming);
    for (int i = 0; i < TF_RANK_SLOTS && e == hipSuccess; ++i)
        e = hipEventCreateWithFlags(&rk->halo_done[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&rk->hs, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&rk->as, hipStreamNonBlocking);
    if (e != hipSuccess) {
        tf_rank_destroy(rk);
        return hip_fail("tf_rank_create", e);
    }
    *out = rk;
    return 0;
}

extern "C" int tf_rank_destroy(tf_rank* rk) {
    if (!rk) return 0;
    for (hipStream_t s : {rk->hs, rk->as})
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    for (int i = 0; i < RING; ++i)
        if (rk->ring[i]) (void)hipEventDestroy(rk->ring[i]);
    for (int i = 0; i < TF_RANK_SLOTS; ++i)
        if (rk->halo_done[i]) (void)hipEventDestroy(rk->halo_done[i]);
    delete rk;
    return 0;
}

extern "C" int tf_rank_local_keyframes(const tf_rank* rk) { return rk ? rk->Kl : 0; }
extern "C" int tf_rank_first_keyframe(const tf_rank* rk) { return rk ? rk->kf0 : 0; }

extern "C" size_t tf_rank_pivotal_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int dtype) {
    if (!rk || S <= 0 || H <= 0 || Dh <= 0 || dtype == TF_F32) return 0;
    if (rk->world == 1) return up256(tf_ext_attn_workspace_bytes(rk->K, S, H, Dh, dtype));
    const size_t bank = layout(rk, S, H, Dh, dtype, TF_RANK_BANK).total;
    const size_t heads = H % rk->world == 0 ? layout(rk, S, H, Dh, dtype, TF_RANK_HEADS).total : 0;
    const size_t runs = layout(rk, S, H, Dh, dtype, TF_RANK_BANK_RUNS).total;   // hosts size ONE workspace for every mode
    const size_t two = bank > heads ? bank : heads;
    return two > runs ? two : runs;
}

extern "C" int tf_rank_pivotal(tf_rank* rk, const void* q, const void* k, const void* v, const int64_t* st_in,
                               void* piv_ext, float* inv_ext, void* kfo_ext, int S, int H, int Dh, float scale,
                               int flags, int dtype, int mode, int slot, void* ws, size_t ws_bytes, void* stream) {
    const bool no_halo = (mode & TF_RANK_NO_HALO) != 0;   // attention only: kfo_ext is a plain [3, Kl, S, H*Dh] output
    const bool want_inv = (mode & TF_RANK_INV_NORM) != 0; // the call computes the local pivots' inverse norms (in its pack launch)
    mode &= ~(TF_RANK_NO_HALO | TF_RANK_INV_NORM);
    TF_ARG(rk && q && k && v && st_in && kfo_ext && ws && (no_halo || (piv_ext && inv_ext)), TF_ERR_NULL,
           "tf_rank_pivotal: null pointer");
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "tf_rank_pivotal: dtype %d (bf16/f16 only)", dtype);
    TF_ARG(mode == TF_RANK_HEADS || mode == TF_RANK_BANK || mode == TF_RANK_BANK_RUNS, TF_ERR_SHAPE,
           "tf_rank_pivotal: mode %d", mode);
    TF_ARG(slot >= 0 && slot < TF_RANK_SLOTS, TF_ERR_SHAPE, "tf_rank_pivotal: slot %d outside [0, %d)", slot, TF_RANK_SLOTS);
    TF_ARG(!(want_inv && no_halo), TF_ERR_SHAPE, "tf_rank_pivotal: TF_RANK_INV_NORM needs the propagation state (no TF_RANK_NO_HALO)");
    TF_ARG(!(flags & (TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY)), TF_ERR_SHAPE,
           "tf_rank_pivotal: the part flags are the executor's own");
    TF_ARG(ws_bytes >= tf_rank_pivotal_workspace_bytes(rk, S, H, Dh, dtype), TF_ERR_WORKSPACE,
           "tf_rank_pivotal: workspace %zu < %zu bytes", ws_bytes, tf_rank_pivotal_workspace_bytes(rk, S, H, Dh, dtype));
    const int W = rk->world, Kl = rk->Kl, K = rk->K, o = (W > 1 && !no_halo) ? 1 : 0;
    const int64_t D = (int64_t)H * Dh, SD = (int64_t)S * D;
    const int64_t q_bs = st_in[0], q_fs = st_in[1], k_bs = st_in[2], k_fs = st_in[3], v_bs = st_in[4], v_fs = st_in[5],
                  ld_q = st_in[6], ld = st_in[7];
    typedef unsigned short E;   // any 16-bit element: only pointer arithmetic happens here
    const E* qe = static_cast<const E*>(q);
    const E* ke = static_cast<const E*>(k);
    const E* ve = static_cast<const E*>(v);
    E* kfo = static_cast<E*>(kfo_ext);
    E* piv = static_cast<E*>(piv_ext);
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t o_bs = (int64_t)(Kl + o) * SD;   // branch stride of the halo-extended attention output
    E* out_loc = kfo + (int64_t)o * SD;            // its local slots
    const int inject = flags & TF_ATTN_INJECT;
    if (!no_halo) rk->halo_set[slot] = false;

    // the local keyframes' pivots and inverse norms (slots o.. of the halo-extended state)
    const E* piv_loc = want_inv ? piv + (int64_t)o * SD : nullptr;
    float* inv_loc = want_inv ? inv_ext + (int64_t)o * S : nullptr;
    if (W == 1) {
        if (want_inv)
            if (const int rc = do_inv_norm(piv_loc, inv_loc, (int64_t)Kl * S, (int)D, dtype, stream)) return rc;
        const int64_t strides[9] = {q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, SD, ld_q};
        return tf_ext_attn_fwd_strided(q, k, v, out_loc, K, K, 0, S, H, Dh, ld, strides, scale, flags, dtype, ws, ws_bytes,
                                       stream);
    }
    int64_t cnt[TF_MAX_WORLD], own[TF_MAX_WORLD];
    for (int p = 0; p < W; ++p) cnt[p] = rk->counts[p], own[p] = Kl;

    if (mode == TF_RANK_HEADS) {
        TF_ARG(H % W == 0, TF_ERR_SHAPE, "tf_rank_pivotal: %d heads do not divide over %d ranks (use TF_RANK_BANK)", H, W);
        TF_ARG(ld_q == ld, TF_ERR_SHAPE, "tf_rank_pivotal: the head re-sharding packs q, k, v with one token stride");
        const Layout L = layout(rk, S, H, Dh, dtype, TF_RANK_HEADS);
        const int Hl = H / W;
        const int64_t hd = D / W, Shd = (int64_t)S * hd;
        E* send = reinterpret_cast<E*>(wsb + L.send);
        E* recv = reinterpret_cast<E*>(wsb + L.recv);
        E* send2 = reinterpret_cast<E*>(wsb + L.send2);
        E* recv2 = reinterpret_cast<E*>(wsb + L.recv2);
        // ---- pack: head group w of every slab the bank branches read, frame-major (slab order [q.., k.., v..])
        const void* slabs[6];
        int64_t fss[6];
        int ns;
        if (inject) {   // source q, k (what uncond and cond use, tokenflow_utils.py:124-130) and the two value banks
            ns = 4;
            slabs[0] = qe, slabs[1] = ke, slabs[2] = ve + v_bs, slabs[3] = ve + 2 * v_bs;
            fss[0] = q_fs, fss[1] = k_fs, fss[2] = v_fs, fss[3] = v_fs;
        } else {
            ns = 6;
            slabs[0] = qe + q_bs, slabs[1] = qe + 2 * q_bs, slabs[2] = ke + k_bs, slabs[3] = ke + 2 * k_bs;
            slabs[4] = ve + v_bs, slabs[5] = ve + 2 * v_bs;
            fss[0] = fss[1] = q_fs, fss[2] = fss[3] = k_fs, fss[4] = fss[5] = v_fs;
        }
        if (const int rc = do_pack(slabs, fss, ns, send, W, Kl, S, (int)hd, ld, piv_loc, inv_loc, (int64_t)Kl * S, (int)D,
                                   dtype, stream))
            return rc;
        // ---- the two tensor sets of the attention: the bank branches on this rank's head group over all K frames, read
        //      from `recv` and written to `send2` in place (both laid out for the collectives), and the source branch of
        //      the local frames on the local projections.
        const int64_t fs_r = ns * Shd;          // frame stride of recv [K][ns][S][hd]
        // base such that branch b sits at base + b * Shd (the strided entry point's convention): a bank-only call
        // never touches branch 0, so the base may lie one slab in front of the buffer -- formed as an integer
        auto slab = [&](const E* buf, int64_t first_slab, int first_branch) {
            return reinterpret_cast<const E*>(reinterpret_cast<uintptr_t>(buf) +
                                              (uintptr_t)((first_slab - first_branch) * Shd * (int64_t)sizeof(E)));
        };
        const E *qb, *kb, *vb;
        if (inject)    // slabs [q0, k0, v1, v2]
            qb = slab(recv, 0, 0), kb = slab(recv, 1, 0), vb = slab(recv, 2, 1);
        else           // slabs [q1, q2, k1, k2, v1, v2]
            qb = slab(recv, 0, 1), kb = slab(recv, 2, 1), vb = slab(recv, 4, 1);
        E* ob = const_cast<E*>(slab(send2, 0, 1));                           // send2 [K][uncond|cond][S][hd]
        TfAttnSet sets[2] = {};
        sets[0].q = qb, sets[0].k = kb, sets[0].v = vb, sets[0].out = ob;
        sets[0].q_bs = Shd, sets[0].q_fs = fs_r, sets[0].ld_q = hd, sets[0].k_bs = Shd, sets[0].k_fs = fs_r;
        sets[0].v_bs = Shd, sets[0].v_fs = fs_r, sets[0].ld = hd, sets[0].o_bs = Shd, sets[0].o_fs = 2 * Shd;
        sets[0].H = Hl, sets[0].Kq = K, sets[0].q_frame0 = 0, sets[0].Kb = K, sets[0].b0 = 1, sets[0].nb = 2;
        sets[1].q = q, sets[1].k = k, sets[1].v = v, sets[1].out = out_loc;
        sets[1].q_bs = q_bs, sets[1].q_fs = q_fs, sets[1].ld_q = ld_q, sets[1].k_bs = k_bs, sets[1].k_fs = k_fs;
        sets[1].v_bs = v_bs, sets[1].v_fs = v_fs, sets[1].ld = ld, sets[1].o_bs = o_bs, sets[1].o_fs = SD;
        sets[1].H = H, sets[1].Kq = Kl, sets[1].q_frame0 = 0, sets[1].Kb = Kl, sets[1].b0 = 0, sets[1].nb = 1;
        // small problems (the coarse levels, a rank's share of the middle ones): ONE launch for both sets behind the
        // exchange -- no V^T pre-passes, no split + merge pair, no separate source launch (csrc/ext_attn_fused.hip)
        // The plan (which kernel, which key split: it decides the arithmetic) must be the SAME on every rank of the
        // block: derived from rank-independent quantities -- the largest local run ceil(K / W) stands for Kl (with an
        // uneven K the ranks' own Kl differ by one).
        TfAttnSet plan_sets[2] = {sets[0], sets[1]};
        plan_sets[1].Kq = plan_sets[1].Kb = (K + W - 1) / W;
        const TfFusedPlan plan = tf_attn_fused_plan(plan_sets, 2, S, Dh, dtype, flags);
        // Everything on the caller's stream, collectives included: every collective of the communicator is issued on
        // ONE stream (no reliance on RCCL's ordering of one communicator across streams), and a hand-over between two
        // streams costs ~10 us of idle device each way (profiles/r04_rank_timeline_v1.txt: four of them per block were
        // 45 us of a 120 us block at the coarse levels).
        // Where the source branch of the local frames is a launch of its own (level 0: the fused plan does not apply), it
        // runs on the auxiliary COMPUTE stream, forked HERE -- behind the pack, in front of the first exchange: it reads
        // only the caller's q / k / v, so it runs under the exchange's wire time and then beside the bank launch, which
        // absorbs what is left of it (a rank's own frames are too few workgroups to fill the chip: cfg2 level 0 at W = 8,
        // 128 workgroups, 61 us alone; 471 -> 440 us per level-0 block with the wire taken out,
        // profiles/r05_rank_step_srcaux_ab.txt).  Joined in front of the second exchange.  The collectives stay on the
        // caller's stream.  TOKENFLOW_RANK_SRC_AUX=0: in line on the caller's stream, behind the exchange.
        const int64_t src_strides[9] = {q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, SD, ld_q};
        auto source_branch = [&](hipStream_t on) {
            return tf_ext_attn_fwd_strided(q, k, v, out_loc, Kl, Kl, 0, S, H, Dh, ld, src_strides, scale,
                                           flags | TF_ATTN_SOURCE_ONLY, dtype, wsb + L.ws_src, L.ws_src_bytes, on);
        };
        const bool fork = !plan.use && src_aux_enabled() && !tf_plan_rec;   // (a recorded plan lists the in-line order)
        if (fork) {
            if (const int rc = order(rk, st, rk->as, "tf_rank_pivotal")) return rc;
            if (const int rc = source_branch(rk->as)) return rc;
        }
        if (const int rc = do_a2a(rk->comm, send, recv, own, cnt, ns, Shd, dtype, st)) return rc;
        if (plan.use) {
            // small problems (the coarse levels, a rank's share of the middle ones): ONE launch for both sets behind
            // the exchange -- no V^T pre-passes, no split + merge pair, no separate source launch
            if (const int rc = tf_attn_fused_launch(sets, 2, S, Dh, scale, flags, dtype, plan, st)) return rc;
        } else {
            if (!fork)
                if (const int rc = source_branch(st)) return rc;
            const int64_t strides[9] = {Shd, fs_r, Shd, fs_r, Shd, fs_r, Shd, 2 * Shd, hd};
            if (const int rc = tf_ext_attn_fwd_strided(qb, kb, vb, ob, K, K, 0, S, Hl, Dh, hd, strides, scale,
                                                       flags | TF_ATTN_BANK_ONLY, dtype,
                                                       wsb + L.ws_bank, L.ws_bank_bytes, stream))
                return rc;
            if (fork)
                if (const int rc = order(rk, rk->as, st, "tf_rank_pivotal")) return rc;
        }
        // ---- outputs back to the frame owners: on the caller's stream (nothing can run beside this exchange: the
        //      unpack and the next block need its result)
        if (const int rc = do_a2a(rk->comm, send2, recv2, cnt, own, 2, Shd, dtype, st)) return rc;
        void* dsts[2] = {out_loc + o_bs, out_loc + 2 * o_bs};
        const int64_t dfs[2] = {SD, SD};
        if (const int rc = do_unpack(recv2, dsts, dfs, 2, W, Kl, S, (int)hd, D, stream)) return rc;
    } else if (mode == TF_RANK_BANK_RUNS) {
        // ---- the bank in runs: the local run starts before the gather lands (tf_ext_attn_run / tf_ext_attn_runs_merge)
        const Layout L = layout(rk, S, H, Dh, dtype, TF_RANK_BANK_RUNS);
        E* send = reinterpret_cast<E*>(wsb + L.send);
        E* recv = reinterpret_cast<E*>(wsb + L.recv);
        void* wsr = wsb + L.ws_bank;
        const Runs R = rank_runs(rk);
        // 1. pack only what PEERS read: the source branch's k and v stay at home (2 of 6 slabs; 1 of 4 under injection, where
        //    the source k IS the bank's k)
        const void* slabs[4];
        int64_t fss[4];
        int ns;
        if (inject) {
            ns = 3;
            slabs[0] = ke, slabs[1] = ve + v_bs, slabs[2] = ve + 2 * v_bs;
            fss[0] = k_fs, fss[1] = fss[2] = v_fs;
        } else {
            ns = 4;
            slabs[0] = ke + k_bs, slabs[1] = ke + 2 * k_bs, slabs[2] = ve + v_bs, slabs[3] = ve + 2 * v_bs;
            fss[0] = fss[1] = k_fs, fss[2] = fss[3] = v_fs;
        }
        if (const int rc = do_pack(slabs, fss, ns, send, 1, Kl, S, (int)D, ld, piv_loc, inv_loc, (int64_t)Kl * S, (int)D,
                                   dtype, stream))
            return rc;
        // 2. the LOCAL run on the auxiliary compute stream, forked behind the pack and in FRONT of the gather: the source
        //    branch of the rank's frames and their bank branches against the rank's OWN keyframes, read from the caller's
        //    q / k / v in place.  Bank frame f of the caller's k / v lives at base + (f - kf0) * frame stride: the shifted
        //    base is formed as an integer (it may lie in front of the tensor; only the run's frames are dereferenced).
        auto shifted = [](const E* base, int64_t elems) {
            return reinterpret_cast<const E*>(reinterpret_cast<uintptr_t>(base) + (uintptr_t)(elems * (int64_t)sizeof(E)));
        };
        const int run_flags = flags & (TF_ATTN_INJECT | TF_ATTN_FOLD_SCALE | TF_ATTN_HINT_MIX | TF_ATTN_NO_SPLIT);
        {
            if (const int rc = order(rk, st, rk->as, "tf_rank_pivotal")) return rc;
            const int64_t strides[9] = {q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, SD, ld_q};
            if (const int rc = tf_ext_attn_run(q, shifted(ke, -(int64_t)rk->kf0 * k_fs), shifted(ve, -(int64_t)rk->kf0 * v_fs),
                                               out_loc, K, Kl, rk->kf0, R.f0[0], R.len[0], 0, R.n, S, H, Dh, ld, strides,
                                               scale, run_flags, dtype, wsr, L.ws_bank_bytes, rk->as))
                return rc;
        }
        // 3. the gather stays on the caller's stream: every collective of a communicator on ONE stream (see the heads form)
        if (const int rc = do_gather(rk->comm, send, recv, cnt, ns, SD, dtype, st)) return rc;
        // 4. behind it the remote runs, read from the receive buffer [K][slabs][S][D] in place (bank branches only: the
        //    base of a tensor whose branch 0 does not exist lies one slab in front of its first slab)
        const int64_t fs_r = ns * SD;
        const E* kb = inject ? recv : shifted(recv, -SD);            // [k0 | ...] or [k1, k2 | ...]
        const E* vb = inject ? recv : shifted(recv, SD);             // [k0, v1, v2] or [k1, k2, v1, v2]
        const int64_t rstrides[9] = {q_bs, q_fs, SD, fs_r, SD, fs_r, o_bs, SD, ld_q};
        for (int r = 1; r < R.n; ++r)
            if (const int rc = tf_ext_attn_run(q, kb, vb, out_loc, K, Kl, rk->kf0, R.f0[r], R.len[r], r, R.n, S, H, Dh, D,
                                               rstrides, scale, run_flags | TF_ATTN_BANK_ONLY, dtype, wsr, L.ws_bank_bytes,
                                               stream))
                return rc;
        //    join the local run, merge into the local slots of kfo_ext
        if (const int rc = order(rk, rk->as, st, "tf_rank_pivotal")) return rc;
        if (const int rc = tf_ext_attn_runs_merge(out_loc, K, Kl, S, H, Dh, R.n, o_bs, SD, run_flags, dtype, wsr,
                                                  L.ws_bank_bytes, stream))
            return rc;
    } else {
        // ---- ONE collective: the slabs the attention reads across frames, gathered into [K][slabs][S][D]
        const Layout L = layout(rk, S, H, Dh, dtype, TF_RANK_BANK);
        E* send = reinterpret_cast<E*>(wsb + L.send);
        E* recv = reinterpret_cast<E*>(wsb + L.recv);
        const void* slabs[6];
        int64_t fss[6];
        int ns;
        if (inject) {
            ns = 4;
            slabs[0] = ke, slabs[1] = ve, slabs[2] = ve + v_bs, slabs[3] = ve + 2 * v_bs;
            fss[0] = k_fs, fss[1] = fss[2] = fss[3] = v_fs;
        } else {
            ns = 6;
            slabs[0] = ke, slabs[1] = ke + k_bs, slabs[2] = ke + 2 * k_bs;
            slabs[3] = ve, slabs[4] = ve + v_bs, slabs[5] = ve + 2 * v_bs;
            fss[0] = fss[1] = fss[2] = k_fs, fss[3] = fss[4] = fss[5] = v_fs;
        }
        if (const int rc = do_pack(slabs, fss, ns, send, 1, Kl, S, (int)D, ld, piv_loc, inv_loc, (int64_t)Kl * S, (int)D,
                                   dtype, stream))
            return rc;
        // the gather on the caller's stream: the attention needs it at once (no stream hand-over, see above)
        if (const int rc = do_gather(rk->comm, send, recv, cnt, ns, SD, dtype, st)) return rc;
        const int64_t fs_r = ns * SD;
        const E* kb = recv;
        const E* vb = recv + (inject ? 1 : 3) * SD;
        const int64_t strides[9] = {q_bs, q_fs, SD, fs_r, SD, fs_r, o_bs, SD, ld_q};
        if (const int rc = tf_ext_attn_fwd_strided(q, kb, vb, out_loc, K, Kl, rk->kf0, S, H, Dh, D, strides, scale, flags,
                                                   dtype, wsb + L.ws_bank, L.ws_bank_bytes, stream))
            return rc;
    }

    // ---- neighbour halo: the last local keyframe's pivots, inverse norms and attention output -> slot 0 of rank r+1
    if (!no_halo)
        if (const int rc = halo_exchange(rk, piv, inv_ext, kfo, 3, o_bs, SD, S, slot, st, "tf_rank_pivotal")) return rc;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// One rank's pivotal pass over a SLIDING-WINDOW bank (include/tokenflow_hip.h): tf_rank_pivotal with a radius.  The rank needs
// the keyframes within `radius` of its own run only: ONE halo pack, ONE sparse tf_all_to_all_rows (mostly neighbour ranks)
// whose receive buffer is the halo-extended bank, the windowed bank part over it in place, the source part of the local frames
// on the auxiliary compute stream beside the exchange.
extern "C" size_t tf_rank_pivotal_window_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int dtype, int radius) {
    if (!rk || S <= 0 || H <= 0 || Dh <= 0 || dtype == TF_F32 || radius < 0) return 0;
    const size_t full = tf_rank_pivotal_workspace_bytes(rk, S, H, Dh, dtype);   // a covering radius IS tf_rank_pivotal
    if (rk->world == 1 || radius >= rk->K - 1 || rk->Kl > TF_MAX_WINDOW_FRAMES) return full;
    const size_t win = window_layout(rk, window_geometry(rk, radius), S, H, Dh, dtype).total;
    return win > full ? win : full;   // ONE workspace whatever the radius
}

extern "C" int tf_rank_pivotal_window(tf_rank* rk, const void* q, const void* k, const void* v, const int64_t* st_in,
                                      void* piv_ext, float* inv_ext, void* kfo_ext, int S, int H, int Dh, float scale,
                                      int flags, int dtype, int mode, int slot, int radius, void* ws, size_t ws_bytes,
                                      void* stream) {
    const char* const fn = "tf_rank_pivotal_window";
    const bool no_halo = (mode & TF_RANK_NO_HALO) != 0, want_inv = (mode & TF_RANK_INV_NORM) != 0;
    const int mods = mode & (TF_RANK_NO_HALO | TF_RANK_INV_NORM), base = mode & ~(TF_RANK_NO_HALO | TF_RANK_INV_NORM);
    // ---- arguments first: nothing below this block's end has touched the device
    TF_ARG(rk && q && k && v && st_in && kfo_ext && ws && (no_halo || (piv_ext && inv_ext)), TF_ERR_NULL, "%s: null pointer", fn);
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "%s: dtype %d (bf16/f16 only)", fn, dtype);
    TF_ARG(radius >= 0, TF_ERR_SHAPE, "%s: radius %d (>= 0)", fn, radius);
    TF_ARG(base == 0 || base == TF_RANK_BANK, TF_ERR_SHAPE,
           "%s: mode %d (the windowed pass has the bank form only: TF_RANK_BANK with TF_RANK_NO_HALO / TF_RANK_INV_NORM)", fn, base);
    TF_ARG(slot >= 0 && slot < TF_RANK_SLOTS, TF_ERR_SHAPE, "%s: slot %d outside [0, %d)", fn, slot, TF_RANK_SLOTS);
    TF_ARG(!(want_inv && no_halo), TF_ERR_SHAPE, "%s: TF_RANK_INV_NORM needs the propagation state (no TF_RANK_NO_HALO)", fn);
    TF_ARG(!(flags & (TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY)), TF_ERR_SHAPE, "%s: the part flags are the executor's own", fn);
    if (radius >= rk->K - 1)   // every window is the whole bank: today's pass -- the same launches, the same bits
        return tf_rank_pivotal(rk, q, k, v, st_in, piv_ext, inv_ext, kfo_ext, S, H, Dh, scale, flags, dtype, TF_RANK_BANK | mods,
                               slot, ws, ws_bytes, stream);
    TF_ARG(rk->Kl <= TF_MAX_WINDOW_FRAMES, TF_ERR_SHAPE, "%s: %d local keyframes (at most %d carry a window)", fn, rk->Kl,
           TF_MAX_WINDOW_FRAMES);
    TF_ARG(!(flags & TF_ATTN_FOLD_SCALE), TF_ERR_SHAPE, "%s: TF_ATTN_FOLD_SCALE has no windowed form", fn);
    const WinGeom G = window_geometry(rk, radius);
    TF_ARG(G.F < (1 << 16), TF_ERR_SHAPE, "%s: a halo-extended bank of %d frames (below 65536)", fn, G.F);
    TF_ARG(ws_bytes >= tf_rank_pivotal_window_workspace_bytes(rk, S, H, Dh, dtype, radius), TF_ERR_WORKSPACE,
           "%s: workspace %zu < %zu bytes", fn, ws_bytes, tf_rank_pivotal_window_workspace_bytes(rk, S, H, Dh, dtype, radius));

    const int W = rk->world, Kl = rk->Kl, K = rk->K, o = (W > 1 && !no_halo) ? 1 : 0;
    const int64_t D = (int64_t)H * Dh, SD = (int64_t)S * D;
    const int64_t q_bs = st_in[0], q_fs = st_in[1], k_bs = st_in[2], k_fs = st_in[3], v_bs = st_in[4], v_fs = st_in[5],
                  ld_q = st_in[6], ld = st_in[7];
    typedef unsigned short E;   // any 16-bit element: only pointer arithmetic happens here
    const E* ke = static_cast<const E*>(k);
    const E* ve = static_cast<const E*>(v);
    E* kfo = static_cast<E*>(kfo_ext);
    E* piv = static_cast<E*>(piv_ext);
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t o_bs = (int64_t)(Kl + o) * SD;   // branch stride of the halo-extended attention output
    E* out_loc = kfo + (int64_t)o * SD;            // its local slots
    const int inject = flags & TF_ATTN_INJECT;
    if (!no_halo) rk->halo_set[slot] = false;
    if (want_inv)   // (a launch of its own: the halo pack kernel carries no inverse norms)
        if (const int rc = do_inv_norm(piv + (int64_t)o * SD, inv_ext + (int64_t)o * S, (int64_t)Kl * S, (int)D, dtype, stream))
            return rc;
    if (W == 1) {   // one rank: the windowed single-GPU call straight into kfo_ext
        const int64_t strides[9] = {q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, SD, ld_q};
        return tf_ext_attn_fwd_windows(q, k, v, out_loc, K, K, 0, S, H, Dh, ld, strides, scale, flags, dtype, G.win_lo, G.win_n, ws,
                                       ws_bytes, stream);
    }
    const WinLayout L = window_layout(rk, G, S, H, Dh, dtype);
    E* send = reinterpret_cast<E*>(wsb + L.send);
    E* recv = reinterpret_cast<E*>(wsb + L.recv);
    // 1. pack only what PEERS read (the choice of TF_RANK_BANK_RUNS): [k1, k2, v1, v2], under injection [k0, v1, v2]; a local
    //    frame several peers need is written to each of their segments, the rank's own frames to its self rows
    const void* slabs[4];
    int64_t fss[4];
    int ns;
    if (inject) {
        ns = 3;
        slabs[0] = ke, slabs[1] = ve + v_bs, slabs[2] = ve + 2 * v_bs;
        fss[0] = k_fs, fss[1] = fss[2] = v_fs;
    } else {
        ns = 4;
        slabs[0] = ke + k_bs, slabs[1] = ke + 2 * k_bs, slabs[2] = ve + v_bs, slabs[3] = ve + 2 * v_bs;
        fss[0] = fss[1] = k_fs, fss[2] = fss[3] = v_fs;
    }
    if (const int rc = do_halo_pack(slabs, fss, ns, send, rk, G, S, (int)D, ld, dtype, stream)) return rc;
    // 2. the source part of the local frames (window-free: own-frame keys), read from q / k / v in place, on the auxiliary
    //    compute stream: forked behind the pack, in FRONT of the exchange, joined behind the bank part.
    //    TOKENFLOW_RANK_SRC_AUX=0: in line on the caller's stream, behind the exchange (a recorded plan lists that order)
    const int64_t src_strides[9] = {q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, SD, ld_q};
    auto source_part = [&](hipStream_t on) {
        return tf_ext_attn_fwd_strided(q, k, v, out_loc, Kl, Kl, 0, S, H, Dh, ld, src_strides, scale, flags | TF_ATTN_SOURCE_ONLY,
                                       dtype, wsb + L.ws_src, L.ws_src_bytes, on);
    };
    const bool fork = src_aux_enabled() && !tf_plan_rec;
    if (fork) {
        if (const int rc = order(rk, st, rk->as, fn)) return rc;
        if (const int rc = source_part(rk->as)) return rc;
    }
    // 3. the sparse exchange on the caller's stream (every collective of a communicator on ONE stream)
    if (const int rc = do_a2a_rows(rk, send, recv, G, ns, SD, dtype, st)) return rc;
    if (!fork)
        if (const int rc = source_part(st)) return rc;
    // 4. the windowed bank part over the receive buffer [F][ns][S][D] in place (the base of a tensor whose branch 0 does not
    //    exist lies one slab in front of its first slab: formed as an integer, never dereferenced there)
    auto shifted = [](const E* b, int64_t elems) {
        return reinterpret_cast<const E*>(reinterpret_cast<uintptr_t>(b) + (uintptr_t)(elems * (int64_t)sizeof(E)));
    };
    const int64_t fs_r = ns * SD;
    const E* kb = inject ? recv : shifted(recv, -SD);   // [k0 | ...] or [k1, k2 | ...]
    const E* vb = inject ? recv : shifted(recv, SD);    // [k0, v1, v2] or [k1, k2, v1, v2]
    const int64_t strides[9] = {q_bs, q_fs, SD, fs_r, SD, fs_r, o_bs, SD, ld_q};
    if (const int rc = tf_ext_attn_fwd_windows_part(q, kb, vb, out_loc, G.F, Kl, G.hl, S, H, Dh, D, strides, scale,
                                                    flags | TF_ATTN_BANK_ONLY, dtype, G.win_lo, G.win_n, wsb + L.ws_bank,
                                                    L.ws_bank_bytes, stream))
        return rc;
    // 5. join
    if (fork)
        if (const int rc = order(rk, rk->as, st, fn)) return rc;
    // 6. the neighbour halo for the propagation, as in every mode
    if (!no_halo)
        if (const int rc = halo_exchange(rk, piv, inv_ext, kfo, 3, o_bs, SD, S, slot, st, fn)) return rc;
    return 0;
}

// The sequence one windowed call issues, recorded by the call itself on a rank that owns no device object (host only).
extern "C" int tf_rank_pivotal_window_plan(int world, int rank, int K, int S, int H, int Dh, int radius, int mode, int flags,
                                           int dtype, char* buf, size_t len) {
    TF_ARG(world >= 1 && world <= TF_MAX_WORLD && rank >= 0 && rank < world && K >= world && S > 0 && H > 0 && Dh > 0,
           TF_ERR_SHAPE, "tf_rank_pivotal_window_plan: rank %d of %d over %d keyframes, S=%d H=%d Dh=%d", rank, world, K, S, H, Dh);
    tf_rank rk{};
    partition(&rk, K, world, rank);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 40);   // never dereferenced
    const int64_t D = (int64_t)H * Dh, SD = (int64_t)S * D;
    const int64_t strides[8] = {rk.Kl * SD, SD, rk.Kl * SD, SD, rk.Kl * SD, SD, D, D};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_rank_pivotal_window(&rk, ph, ph, ph, strides, ph, static_cast<float*>(ph), ph, S, H, Dh, 1.0f, flags, dtype,
                                          mode, 0, radius, ph, (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_rank_pivotal_window_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// ---------------------------------------------------------------------------------------------
// One rank's pivotal pass over an ANCHORED sliding-window bank (include/tokenflow_hip.h): tf_rank_pivotal_window plus global
// anchor keyframes that every keyframe sees.  What `sharded.frame_set_halo_plan` computes in Python: rank r reads the set
// U = [lo, hi) + anchors (ascending, F frames, at most 64: a set is a mask over the EXTENDED bank, so K itself is free); peer p
// sends it U & own(p), it sends peer p own(r) & U_p -- a mask of local frames; its own frames travel as its self rows and are
// contiguous in U at q_frame0 = the members of U below kf0.  Local query i gets (window of kf0 + i) + anchors as a mask over
// the positions in U.
namespace {

struct SetGeom {
    WinGeom w;   // lo / hi / F, the row counts and send_total of the exchange (the window table is not used)
    int q_frame0;
    uint64_t send_mask[TF_MAX_WORLD];             // per peer: the LOCAL frames it reads
    uint64_t sets[TF_MAX_WINDOW_FRAMES];          // per local query: its members, positions in U
};

// anchors: sorted, unique, inside [0, K); Kl <= 64 (the caller's checks).  Returns false where U holds more than 64 frames.
bool frame_set_geometry(const tf_rank* rk, int R, const int* anc, int na, SetGeom* out) {
    SetGeom& g = *out;
    g = SetGeom{};
    const int K = rk->K, Kl = rk->Kl, kf0 = rk->kf0;
    const int64_t Rl = R;
    auto reach_lo = [&](int f0) { return (int)(f0 - Rl > 0 ? f0 - Rl : 0); };
    auto reach_hi = [&](int f1) { return (int)(f1 + Rl < K ? f1 + Rl : K); };
    auto is_anchor = [&](int f) {
        int a = 0, b = na;
        while (a < b) {
            const int m = (a + b) / 2;
            if (anc[m] < f) a = m + 1; else b = m;
        }
        return a < na && anc[a] == f;
    };
    const int lo = reach_lo(kf0), hi = reach_hi(kf0 + Kl);
    int nlow = 0, nhigh = 0;
    for (int j = 0; j < na; ++j) nlow += anc[j] < lo, nhigh += anc[j] >= hi;
    g.w.lo = lo, g.w.hi = hi, g.w.hl = kf0 - lo, g.w.hr = hi - kf0 - Kl;
    const int64_t F = (int64_t)nlow + (hi - lo) + nhigh;
    if (F > 64) return false;
    g.w.F = (int)F;
    g.q_frame0 = nlow + (kf0 - lo);
    int off = 0;
    for (int p = 0; p < rk->world; ++p) {
        const int p0 = off, p1 = off + rk->counts[p];
        off = p1;
        // what arrives from p: own(p) & U
        const int a = imax(p0, lo), b = imin(p1, hi);
        int n = b > a ? b - a : 0;
        for (int j = 0; j < na; ++j) n += anc[j] >= p0 && anc[j] < p1 && (anc[j] < lo || anc[j] >= hi);
        g.w.recv_rows[p] = n;
        // what goes to p: own(r) & U_p
        const int lo_p = reach_lo(p0), hi_p = reach_hi(p1);
        uint64_t m = 0;
        for (int i = 0; i < Kl; ++i) {
            const int f = kf0 + i;
            if ((f >= lo_p && f < hi_p) || is_anchor(f)) m |= (uint64_t)1 << i;
        }
        g.send_mask[p] = m;
        g.w.send_rows[p] = __builtin_popcountll(m);
        g.w.send_total += g.w.send_rows[p];
    }
    // the anchors as positions in U: those outside [lo, hi) fill the two ends, those inside sit at their offset
    uint64_t am = 0;
    for (int j = 0, below = 0, above = 0; j < na; ++j) {
        const int a = anc[j];
        const int pos = a < lo ? below++ : a >= hi ? nlow + (hi - lo) + above++ : nlow + (a - lo);
        am |= (uint64_t)1 << pos;
    }
    for (int i = 0; i < Kl; ++i) {
        const int64_t gi = kf0 + i;
        const int w0 = (int)(gi - Rl > 0 ? gi - Rl : 0), w1 = (int)(gi + Rl < K - 1 ? gi + Rl : K - 1);
        const int n = w1 - w0 + 1;
        g.sets[i] = ((n == 64 ? ~(uint64_t)0 : ((uint64_t)1 << n) - 1) << (nlow + (w0 - lo))) | am;
    }
    return true;
}

// the anchors of a call validated, sorted and without duplicates (n_out <= n): a bad index is TF_ERR_SHAPE
int sorted_anchors(const char* fn, int K, const int* anchors, int n, int* out, int* n_out) {
    for (int j = 0; j < n; ++j) {
        TF_ARG(anchors[j] >= 0 && anchors[j] < K, TF_ERR_SHAPE, "%s: anchor %d outside the %d keyframes", fn, anchors[j], K);
        int i = j;   // insertion sort: a handful of anchors
        for (; i > 0 && out[i - 1] > anchors[j]; --i) out[i] = out[i - 1];
        out[i] = anchors[j];
    }
    int m = 0;
    for (int j = 0; j < n; ++j)
        if (!m || out[m - 1] != out[j]) out[m++] = out[j];
    *n_out = m;
    return 0;
}

constexpr int MAX_ANCHORS = 4096;   // of one call (duplicates included); at most 64 distinct ones can lie in a rank's bank anyway

int do_set_pack(const void* const* slabs, const int64_t* fss, int ns, void* send, const tf_rank* rk, const SetGeom& g, int S,
                int D, int64_t ld, int dtype, void* stream) {
    if (tf_plan_note("set_pack[ns=%d]", ns)) return 0;
    return tf_frame_set_halo_pack(slabs, fss, ns, send, rk->world, g.send_mask, rk->Kl, S, D, ld, dtype, stream);
}

}  // namespace

extern "C" size_t tf_rank_pivotal_frame_sets_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int dtype, int radius,
                                                             const int* anchors, int n_anchors) {
    const size_t win = tf_rank_pivotal_window_workspace_bytes(rk, S, H, Dh, dtype, radius);   // (0 for what that call refuses)
    if (n_anchors == 0 || !win) return win;   // no anchors IS the windowed call
    if (n_anchors < 0 || n_anchors > MAX_ANCHORS || !anchors) return 0;
    if (rk->world == 1 || radius >= rk->K - 1 || rk->Kl > TF_MAX_WINDOW_FRAMES) return win;
    int anc[MAX_ANCHORS], na = 0;
    for (int j = 0; j < n_anchors; ++j)
        if (anchors[j] < 0 || anchors[j] >= rk->K) return 0;
    sorted_anchors("", rk->K, anchors, n_anchors, anc, &na);
    SetGeom G;
    if (!frame_set_geometry(rk, radius, anc, na, &G)) return 0;
    const size_t set = window_layout(rk, G.w, S, H, Dh, dtype).total;
    return set > win ? set : win;   // never below the windowed call's for the same radius
}

extern "C" int tf_rank_pivotal_frame_sets(tf_rank* rk, const void* q, const void* k, const void* v, const int64_t* st_in,
                                          void* piv_ext, float* inv_ext, void* kfo_ext, int S, int H, int Dh, float scale,
                                          int flags, int dtype, int mode, int slot, int radius, const int* anchors,
                                          int n_anchors, void* ws, size_t ws_bytes, void* stream) {
    const char* const fn = "tf_rank_pivotal_frame_sets";
    const bool no_halo = (mode & TF_RANK_NO_HALO) != 0, want_inv = (mode & TF_RANK_INV_NORM) != 0;
    const int mods = mode & (TF_RANK_NO_HALO | TF_RANK_INV_NORM), base = mode & ~(TF_RANK_NO_HALO | TF_RANK_INV_NORM);
    // ---- arguments first: nothing below this block's end has touched the device
    TF_ARG(rk && q && k && v && st_in && kfo_ext && ws && (no_halo || (piv_ext && inv_ext)) && (anchors || n_anchors == 0),
           TF_ERR_NULL, "%s: null pointer", fn);
    TF_ARG(n_anchors >= 0 && n_anchors <= MAX_ANCHORS, TF_ERR_SHAPE, "%s: %d anchors (0 .. %d)", fn, n_anchors, MAX_ANCHORS);
    if (n_anchors == 0)   // no anchors: the windowed pass -- the same launches, the same bits, the same plan tokens
        return tf_rank_pivotal_window(rk, q, k, v, st_in, piv_ext, inv_ext, kfo_ext, S, H, Dh, scale, flags, dtype, mode, slot,
                                      radius, ws, ws_bytes, stream);
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "%s: dtype %d (bf16/f16 only)", fn, dtype);
    TF_ARG(radius >= 0, TF_ERR_SHAPE, "%s: radius %d (>= 0)", fn, radius);
    TF_ARG(base == 0 || base == TF_RANK_BANK, TF_ERR_SHAPE,
           "%s: mode %d (the anchored pass has the bank form only: TF_RANK_BANK with TF_RANK_NO_HALO / TF_RANK_INV_NORM)", fn, base);
    TF_ARG(slot >= 0 && slot < TF_RANK_SLOTS, TF_ERR_SHAPE, "%s: slot %d outside [0, %d)", fn, slot, TF_RANK_SLOTS);
    TF_ARG(!(want_inv && no_halo), TF_ERR_SHAPE, "%s: TF_RANK_INV_NORM needs the propagation state (no TF_RANK_NO_HALO)", fn);
    TF_ARG(!(flags & (TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY)), TF_ERR_SHAPE, "%s: the part flags are the executor's own", fn);
    int anc[MAX_ANCHORS], na = 0;
    if (const int rc = sorted_anchors(fn, rk->K, anchors, n_anchors, anc, &na)) return rc;
    if (radius >= rk->K - 1)   // every window is the whole bank: today's pass whatever the anchors
        return tf_rank_pivotal(rk, q, k, v, st_in, piv_ext, inv_ext, kfo_ext, S, H, Dh, scale, flags, dtype, TF_RANK_BANK | mods,
                               slot, ws, ws_bytes, stream);
    TF_ARG(rk->Kl <= TF_MAX_WINDOW_FRAMES, TF_ERR_SHAPE, "%s: %d local keyframes (at most %d carry a set)", fn, rk->Kl,
           TF_MAX_WINDOW_FRAMES);
    TF_ARG(!(flags & TF_ATTN_FOLD_SCALE), TF_ERR_SHAPE, "%s: TF_ATTN_FOLD_SCALE has no frame-set form", fn);
    SetGeom G;
    TF_ARG(frame_set_geometry(rk, radius, anc, na, &G), TF_ERR_SHAPE,
           "%s: window reach plus anchors exceed 64 frames on rank %d (a set is a 64-bit mask over the rank's extended bank)", fn,
           rk->rank);
    const size_t ws_need = tf_rank_pivotal_frame_sets_workspace_bytes(rk, S, H, Dh, dtype, radius, anchors, n_anchors);
    TF_ARG(ws_bytes >= ws_need, TF_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, ws_need);

    const int W = rk->world, Kl = rk->Kl, K = rk->K, o = (W > 1 && !no_halo) ? 1 : 0;
    const int64_t D = (int64_t)H * Dh, SD = (int64_t)S * D;
    const int64_t q_bs = st_in[0], q_fs = st_in[1], k_bs = st_in[2], k_fs = st_in[3], v_bs = st_in[4], v_fs = st_in[5],
                  ld_q = st_in[6], ld = st_in[7];
    typedef unsigned short E;   // any 16-bit element: only pointer arithmetic happens here
    const E* ke = static_cast<const E*>(k);
    const E* ve = static_cast<const E*>(v);
    E* kfo = static_cast<E*>(kfo_ext);
    E* piv = static_cast<E*>(piv_ext);
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t o_bs = (int64_t)(Kl + o) * SD;   // branch stride of the halo-extended attention output
    E* out_loc = kfo + (int64_t)o * SD;            // its local slots
    const int inject = flags & TF_ATTN_INJECT;
    if (!no_halo) rk->halo_set[slot] = false;
    if (want_inv)   // (a launch of its own: the pack kernel carries no inverse norms)
        if (const int rc = do_inv_norm(piv + (int64_t)o * SD, inv_ext + (int64_t)o * S, (int64_t)Kl * S, (int)D, dtype, stream))
            return rc;
    if (W == 1) {   // one rank: U is the whole bank, the single-GPU frame-set call straight into kfo_ext (K <= 64 there)
        const int64_t strides[9] = {q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, SD, ld_q};
        return tf_ext_attn_fwd_frame_sets(q, k, v, out_loc, K, K, 0, S, H, Dh, ld, strides, scale, flags, dtype, G.sets, ws, ws_bytes,
                                          stream);
    }
    const WinLayout L = window_layout(rk, G.w, S, H, Dh, dtype);
    E* send = reinterpret_cast<E*>(wsb + L.send);
    E* recv = reinterpret_cast<E*>(wsb + L.recv);
    // 1. pack only what PEERS read: [k1, k2, v1, v2], under injection [k0, v1, v2]; per peer the members of its mask in ascending
    //    order (an anchor this rank owns goes to every peer), the rank's own frames to its self rows
    const void* slabs[4];
    int64_t fss[4];
    int ns;
    if (inject) {
        ns = 3;
        slabs[0] = ke, slabs[1] = ve + v_bs, slabs[2] = ve + 2 * v_bs;
        fss[0] = k_fs, fss[1] = fss[2] = v_fs;
    } else {
        ns = 4;
        slabs[0] = ke + k_bs, slabs[1] = ke + 2 * k_bs, slabs[2] = ve + v_bs, slabs[3] = ve + 2 * v_bs;
        fss[0] = fss[1] = k_fs, fss[2] = fss[3] = v_fs;
    }
    if (const int rc = do_set_pack(slabs, fss, ns, send, rk, G, S, (int)D, ld, dtype, stream)) return rc;
    // 2. the source part of the local frames (set-free), as in the windowed call
    const int64_t src_strides[9] = {q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, SD, ld_q};
    auto source_part = [&](hipStream_t on) {
        return tf_ext_attn_fwd_strided(q, k, v, out_loc, Kl, Kl, 0, S, H, Dh, ld, src_strides, scale, flags | TF_ATTN_SOURCE_ONLY,
                                       dtype, wsb + L.ws_src, L.ws_src_bytes, on);
    };
    const bool fork = src_aux_enabled() && !tf_plan_rec;
    if (fork) {
        if (const int rc = order(rk, st, rk->as, fn)) return rc;
        if (const int rc = source_part(rk->as)) return rc;
    }
    // 3. the sparse exchange on the caller's stream: the receive buffer is U in ascending order
    if (const int rc = do_a2a_rows(rk, send, recv, G.w, ns, SD, dtype, st)) return rc;
    if (!fork)
        if (const int rc = source_part(st)) return rc;
    // 4. the frame-set bank part over the receive buffer [F][ns][S][D] in place (a table of ranges: the windowed part)
    auto shifted = [](const E* b, int64_t elems) {
        return reinterpret_cast<const E*>(reinterpret_cast<uintptr_t>(b) + (uintptr_t)(elems * (int64_t)sizeof(E)));
    };
    const int64_t fs_r = ns * SD;
    const E* kb = inject ? recv : shifted(recv, -SD);   // [k0 | ...] or [k1, k2 | ...]
    const E* vb = inject ? recv : shifted(recv, SD);    // [k0, v1, v2] or [k1, k2, v1, v2]
    const int64_t strides[9] = {q_bs, q_fs, SD, fs_r, SD, fs_r, o_bs, SD, ld_q};
    if (const int rc = tf_ext_attn_fwd_frame_sets_part(q, kb, vb, out_loc, G.w.F, Kl, G.q_frame0, S, H, Dh, D, strides, scale,
                                                       flags | TF_ATTN_BANK_ONLY, dtype, G.sets, wsb + L.ws_bank, L.ws_bank_bytes,
                                                       stream))
        return rc;
    // 5. join
    if (fork)
        if (const int rc = order(rk, rk->as, st, fn)) return rc;
    // 6. the neighbour halo for the propagation, as in every mode
    if (!no_halo)
        if (const int rc = halo_exchange(rk, piv, inv_ext, kfo, 3, o_bs, SD, S, slot, st, fn)) return rc;
    return 0;
}

// The sequence one anchored call issues, recorded by the call itself on a rank that owns no device object (host only).
extern "C" int tf_rank_pivotal_frame_sets_plan(int world, int rank, int K, int S, int H, int Dh, int radius, const int* anchors,
                                               int n_anchors, int mode, int flags, int dtype, char* buf, size_t len) {
    TF_ARG(world >= 1 && world <= TF_MAX_WORLD && rank >= 0 && rank < world && K >= world && S > 0 && H > 0 && Dh > 0,
           TF_ERR_SHAPE, "tf_rank_pivotal_frame_sets_plan: rank %d of %d over %d keyframes, S=%d H=%d Dh=%d", rank, world, K, S, H,
           Dh);
    tf_rank rk{};
    partition(&rk, K, world, rank);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 40);   // never dereferenced
    const int64_t D = (int64_t)H * Dh, SD = (int64_t)S * D;
    const int64_t strides[8] = {rk.Kl * SD, SD, rk.Kl * SD, SD, rk.Kl * SD, SD, D, D};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_rank_pivotal_frame_sets(&rk, ph, ph, ph, strides, ph, static_cast<float*>(ph), ph, S, H, Dh, 1.0f, flags,
                                              dtype, mode, 0, radius, anchors, n_anchors, ph, (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_rank_pivotal_frame_sets_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

extern "C" int tf_rank_halo_wait(tf_rank* rk, int slot, void* stream) {
    TF_ARG(rk, TF_ERR_NULL, "tf_rank_halo_wait: null pointer");
    TF_ARG(slot >= 0 && slot < TF_RANK_SLOTS, TF_ERR_SHAPE, "tf_rank_halo_wait: slot %d outside [0, %d)", slot,
           TF_RANK_SLOTS);
    if (rk->halo_set[slot])
        TF_HIP(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), rk->halo_done[slot], 0), "tf_rank_halo_wait");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The same pass for a multi-edit batch (include/tokenflow_hip.h): B = 1 + 2E branches [source | uncond_1 | cond_1 | ...], the
// C++ form of FrameShard._pivotal_heads_edits / _pivotal_bank_edits (tokenflow_amd/sharded.py) with their buffer layouts.  Per
// block the collectives and the launches stay at the single-edit count; only their payload grows with E.
namespace {

struct EditsLayout {   // exchange buffers of one call inside the caller's workspace; slab counts at their largest
    size_t send, recv, send2, recv2, stage, ws_bank, ws_src, total;
    size_t ws_bank_bytes, ws_src_bytes;
};

EditsLayout edits_layout(const tf_rank* rk, int S, int H, int Dh, int E, int dtype, int mode) {
    const size_t eb = 2;
    const int W = rk->world, Kl = rk->Kl, K = rk->K;
    const size_t D = (size_t)H * Dh;
    EditsLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += up256(bytes);
        return at;
    };
    if (mode == TF_RANK_HEADS) {   // [q slots | k slots | v_1 .. v_2E]: 6E slabs where no edit injects
        const size_t hd = D / W;
        L.send = take((size_t)W * Kl * 6 * E * S * hd * eb);
        L.recv = take((size_t)K * 6 * E * S * hd * eb);
        L.send2 = take((size_t)K * 2 * E * S * hd * eb);
        L.recv2 = take((size_t)W * Kl * 2 * E * S * hd * eb);
        L.ws_bank_bytes = tf_ext_attn_edits_workspace_bytes(K, S, H / W, Dh, E, dtype);
    } else {                       // [k slots | v_1 .. v_2E]: 4E slabs; the compact q of a mixed mask is staged (< 2E slots)
        L.send = take((size_t)Kl * 4 * E * S * D * eb);
        L.recv = take((size_t)K * 4 * E * S * D * eb);
        L.stage = take((size_t)Kl * 2 * E * S * D * eb);
        L.ws_bank_bytes = tf_ext_attn_edits_workspace_bytes(K, S, H, Dh, E, dtype);
    }
    // the bank part and the source part may run concurrently: a workspace each
    L.ws_src_bytes = tf_ext_attn_edits_workspace_bytes(Kl, S, H, Dh, E, dtype);
    L.ws_bank = take(L.ws_bank_bytes);
    L.ws_src = take(L.ws_src_bytes);
    L.total = off;
    return L;
}

// TF_RANK_BANK_EDIT_RUNS: the exchange buffers of the bank form ([k slots | v_1 .. v_2E]: 4E slabs where no edit injects) and
// ONE run-set workspace of the multi-edit run calls (tf_ext_attn_run_edits)
struct EditRunsLayout {
    size_t send, recv, ws_runs, total, ws_runs_bytes;
};

EditRunsLayout edit_runs_layout(const tf_rank* rk, int S, int H, int Dh, int E, int dtype) {
    const size_t eb = 2, D = (size_t)H * Dh;
    EditRunsLayout L{};
    L.send = 0;
    L.recv = up256((size_t)rk->Kl * 4 * E * S * D * eb);
    L.ws_runs = L.recv + up256((size_t)rk->K * 4 * E * S * D * eb);
    L.ws_runs_bytes = tf_ext_attn_runs_edits_workspace_bytes(rk->K, rk->Kl, S, H, Dh, rank_runs(rk).n, E, dtype);
    L.total = L.ws_runs + up256(L.ws_runs_bytes);
    return L;
}

}  // namespace

// Workspace of tf_rank_pivotal_edits with TF_RANK_BANK_EDIT_RUNS (the other modes: tf_rank_pivotal_edits_workspace_bytes).
extern "C" size_t tf_rank_pivotal_edit_runs_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int n_edits, int dtype) {
    if (!rk || S <= 0 || H <= 0 || Dh <= 0 || dtype == TF_F32 || n_edits < 1 || n_edits > TF_MAX_EDITS) return 0;
    if (n_edits == 1) return tf_rank_pivotal_workspace_bytes(rk, S, H, Dh, dtype);
    if (rk->world == 1) return up256(tf_ext_attn_edits_workspace_bytes(rk->K, S, H, Dh, n_edits, dtype));
    if (!(Dh == 40 || Dh == 64 || Dh == 80 || Dh == 160)) return 0;
    return edit_runs_layout(rk, S, H, Dh, n_edits, dtype).total;
}

extern "C" size_t tf_rank_pivotal_edits_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int n_edits, int dtype) {
    if (!rk || S <= 0 || H <= 0 || Dh <= 0 || dtype == TF_F32 || n_edits < 1 || n_edits > TF_MAX_EDITS) return 0;
    if (n_edits == 1) return tf_rank_pivotal_workspace_bytes(rk, S, H, Dh, dtype);
    if (rk->world == 1) return up256(tf_ext_attn_edits_workspace_bytes(rk->K, S, H, Dh, n_edits, dtype));
    const size_t bank = edits_layout(rk, S, H, Dh, n_edits, dtype, TF_RANK_BANK).total;   // ONE workspace for both modes
    const size_t heads = H % rk->world == 0 ? edits_layout(rk, S, H, Dh, n_edits, dtype, TF_RANK_HEADS).total : 0;
    return bank > heads ? bank : heads;
}

extern "C" int tf_rank_pivotal_edits(tf_rank* rk, const void* q, const void* k, const void* v, const int64_t* st_in,
                                     void* piv_ext, float* inv_ext, void* kfo_ext, int S, int H, int Dh, float scale,
                                     int flags, int dtype, int mode_in, int slot, int n_edits, unsigned inject_mask, void* ws,
                                     size_t ws_bytes, void* stream) {
    const char* const fn = "tf_rank_pivotal_edits";
    const bool no_halo = (mode_in & TF_RANK_NO_HALO) != 0, want_inv = (mode_in & TF_RANK_INV_NORM) != 0;
    const int mode = mode_in & ~(TF_RANK_NO_HALO | TF_RANK_INV_NORM);
    // ---- arguments first: nothing below this block's end has touched the device
    TF_ARG(rk && q && k && v && st_in && kfo_ext && ws && (no_halo || (piv_ext && inv_ext)), TF_ERR_NULL, "%s: null pointer", fn);
    TF_ARG(n_edits >= 1 && n_edits <= TF_MAX_EDITS, TF_ERR_SHAPE, "%s: n_edits=%d (1 .. %d)", fn, n_edits, TF_MAX_EDITS);
    TF_ARG(!(flags & TF_ATTN_INJECT), TF_ERR_SHAPE, "%s: TF_ATTN_INJECT beside a mask (the mask is the injection state)", fn);
    TF_ARG(!(inject_mask >> n_edits), TF_ERR_SHAPE, "%s: inject_mask=0x%x has bits at or above n_edits=%d", fn, inject_mask,
           n_edits);
    TF_ARG(!(flags & (TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY)), TF_ERR_SHAPE, "%s: the part flags are the executor's own", fn);
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "%s: dtype %d (bf16/f16 only)", fn, dtype);
    TF_ARG(mode == TF_RANK_HEADS || mode == TF_RANK_BANK || mode == TF_RANK_BANK_RUNS || mode == TF_RANK_BANK_EDIT_RUNS,
           TF_ERR_SHAPE, "%s: mode %d", fn, mode);
    TF_ARG(!(mode == TF_RANK_BANK_RUNS && n_edits > 1), TF_ERR_SHAPE,
           "%s: TF_RANK_BANK_RUNS has no multi-edit form (TF_RANK_BANK, TF_RANK_HEADS or TF_RANK_BANK_EDIT_RUNS)", fn);
    const bool edit_runs = mode == TF_RANK_BANK_EDIT_RUNS;
    TF_ARG(!(mode == TF_RANK_HEADS && rk->world > 1 && H % rk->world), TF_ERR_SHAPE,
           "%s: %d heads do not divide over %d ranks (use TF_RANK_BANK)", fn, H, rk->world);
    TF_ARG(slot >= 0 && slot < TF_RANK_SLOTS, TF_ERR_SHAPE, "%s: slot %d outside [0, %d)", fn, slot, TF_RANK_SLOTS);
    TF_ARG(!(want_inv && no_halo), TF_ERR_SHAPE, "%s: TF_RANK_INV_NORM needs the propagation state (no TF_RANK_NO_HALO)", fn);
    if (n_edits == 1)   // one edit: the single-edit executor itself -- the same launches, the same bits (the multi-edit run
                        // form of one edit is TF_RANK_BANK_RUNS)
        return tf_rank_pivotal(rk, q, k, v, st_in, piv_ext, inv_ext, kfo_ext, S, H, Dh, scale,
                               flags | (inject_mask ? TF_ATTN_INJECT : 0), dtype,
                               edit_runs ? (mode_in & (TF_RANK_NO_HALO | TF_RANK_INV_NORM)) | TF_RANK_BANK_RUNS : mode_in, slot, ws,
                               ws_bytes, stream);
    {
        const size_t need = edit_runs ? tf_rank_pivotal_edit_runs_workspace_bytes(rk, S, H, Dh, n_edits, dtype)
                                      : tf_rank_pivotal_edits_workspace_bytes(rk, S, H, Dh, n_edits, dtype);
        TF_ARG(!edit_runs || need, TF_ERR_SHAPE, "%s: head dim %d not in {40,64,80,160}", fn, Dh);
        TF_ARG(ws_bytes >= need, TF_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    }

    const int E = n_edits, B = 1 + 2 * E;
    const int W = rk->world, Kl = rk->Kl, K = rk->K, o = (W > 1 && !no_halo) ? 1 : 0;
    const int64_t D = (int64_t)H * Dh, SD = (int64_t)S * D;
    const int64_t q_bs = st_in[0], q_fs = st_in[1], k_bs = st_in[2], k_fs = st_in[3], v_bs = st_in[4], v_fs = st_in[5],
                  ld_q = st_in[6], ld = st_in[7];
    typedef unsigned short El;   // any 16-bit element: only pointer arithmetic happens here
    const El* qe = static_cast<const El*>(q);
    const El* ke = static_cast<const El*>(k);
    const El* ve = static_cast<const El*>(v);
    El* kfo = static_cast<El*>(kfo_ext);
    El* piv = static_cast<El*>(piv_ext);
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t o_bs = (int64_t)(Kl + o) * SD;   // branch stride of the halo-extended attention output
    El* out_loc = kfo + (int64_t)o * SD;           // its local slots
    if (!no_halo) rk->halo_set[slot] = false;
    const El* piv_loc = want_inv ? piv + (int64_t)o * SD : nullptr;
    float* inv_loc = want_inv ? inv_ext + (int64_t)o * S : nullptr;
    const int64_t loc_strides[9] = {q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, SD, ld_q};

    if (W == 1) {
        if (want_inv)
            if (const int rc = do_inv_norm(piv_loc, inv_loc, (int64_t)Kl * S, (int)D, dtype, stream)) return rc;
        return tf_ext_attn_fwd_edits_masked(q, k, v, out_loc, K, K, 0, S, H, Dh, ld, loc_strides, scale, flags, dtype, E,
                                            inject_mask, ws, ws_bytes, stream);
    }
    int64_t cnt[TF_MAX_WORLD], own[TF_MAX_WORLD];
    for (int p = 0; p < W; ++p) cnt[p] = rk->counts[p], own[p] = Kl;

    // the compact q / k layout of tf_ext_attn_fwd_edits_part: slot 0 the source where some edit injects, then (uncond, cond)
    // of every edit that does not, ascending; b0 = the first slot that exists
    int slots[1 + 2 * TF_MAX_EDITS], nq = 0;
    if (inject_mask) slots[nq++] = 0;
    for (int e = 0; e < E; ++e)
        if (!((inject_mask >> e) & 1u)) slots[nq++] = 1 + 2 * e, slots[nq++] = 2 + 2 * e;
    const int b0 = inject_mask ? 0 : 1;
    const bool mixed = inject_mask && nq > 1;   // some edits inject, some do not
    // base such that slab `first_slab` of a buffer of `unit`-element slabs is branch `first_branch` (the strided entry points'
    // convention): a slot that does not exist is never addressed, so the base may lie in front of the buffer -- an integer
    auto slab = [](const El* buf, int64_t first_slab, int first_branch, int64_t unit) {
        return reinterpret_cast<const El*>(reinterpret_cast<uintptr_t>(buf) +
                                           (uintptr_t)((first_slab - first_branch) * unit * (int64_t)sizeof(El)));
    };
    const void* slabs[6 * TF_MAX_EDITS];
    int64_t fss[6 * TF_MAX_EDITS];
    if (edit_runs) {
        // ---- the bank in runs for E edits: the schedule of TF_RANK_BANK_RUNS over tf_ext_attn_run_edits / _runs_merge_edits
        const EditRunsLayout L = edit_runs_layout(rk, S, H, Dh, E, dtype);
        El* send = reinterpret_cast<El*>(wsb + L.send);
        El* recv = reinterpret_cast<El*>(wsb + L.recv);
        void* wsr = wsb + L.ws_runs;
        const Runs R = rank_runs(rk);
        // 1. ONE pack (W = 1) of exactly what TF_RANK_BANK packs: the compact k slots and the 2E value slabs
        const int ns = nq + 2 * E;
        for (int i = 0; i < nq; ++i) slabs[i] = ke + slots[i] * k_bs, fss[i] = k_fs;
        for (int j = 0; j < 2 * E; ++j) slabs[nq + j] = ve + (1 + j) * v_bs, fss[nq + j] = v_fs;
        if (const int rc = do_pack(slabs, fss, ns, send, 1, Kl, S, (int)D, ld, piv_loc, inv_loc, (int64_t)Kl * S, (int)D,
                                   dtype, stream))
            return rc;
        // 2. the LOCAL run on the auxiliary compute stream, forked behind the pack and in FRONT of the gather: the source
        //    branch and every edit's bank partials against the rank's own keyframes, from q / k / v in place, dense (bank
        //    frame f of the caller's k / v at base + (f - kf0) * frame stride: the shifted base is formed as an integer)
        auto shifted = [](const El* base, int64_t elems) {
            return reinterpret_cast<const El*>(reinterpret_cast<uintptr_t>(base) + (uintptr_t)(elems * (int64_t)sizeof(El)));
        };
        // (TF_ATTN_RUN_MULTI_V: the four-bank run launches for pairs of injecting edits, the same in every call of the set)
        const int run_flags = flags & (TF_ATTN_FOLD_SCALE | TF_ATTN_HINT_MIX | TF_ATTN_NO_SPLIT | TF_ATTN_RUN_MULTI_V);
        auto local_run = [&](hipStream_t on) {
            return tf_ext_attn_run_edits(q, shifted(ke, -(int64_t)rk->kf0 * k_fs), shifted(ve, -(int64_t)rk->kf0 * v_fs), out_loc,
                                         K, Kl, rk->kf0, R.f0[0], R.len[0], 0, R.n, S, H, Dh, ld, loc_strides, scale, run_flags,
                                         dtype, E, inject_mask, 0, wsr, L.ws_runs_bytes, on);
        };
        const bool fork = !tf_plan_rec;   // (a recorded plan lists the in-line order: the local run behind the gather)
        if (fork) {
            if (const int rc = order(rk, st, rk->as, fn)) return rc;
            if (const int rc = local_run(rk->as)) return rc;
        }
        // 3. the gather on the caller's stream: every collective of a communicator on ONE stream
        if (const int rc = do_gather(rk->comm, send, recv, cnt, ns, SD, dtype, st)) return rc;
        if (!fork)
            if (const int rc = local_run(st)) return rc;
        // 4. behind it the remote runs: bank branches only, k compact from the receive buffer [K][ns][S][D] in place, q from
        //    the local tensors (dense: no staging copy under a mixed mask)
        const int64_t fs_r = ns * SD;
        const El* kb = slab(recv, 0, b0, SD);
        const El* vb = slab(recv, nq, 1, SD);
        const int64_t rstrides[9] = {q_bs, q_fs, SD, fs_r, SD, fs_r, o_bs, SD, ld_q};
        for (int r = 1; r < R.n; ++r)
            if (const int rc = tf_ext_attn_run_edits(q, kb, vb, out_loc, K, Kl, rk->kf0, R.f0[r], R.len[r], r, R.n, S, H, Dh, D,
                                                     rstrides, scale, run_flags | TF_ATTN_BANK_ONLY, dtype, E, inject_mask, 2,
                                                     wsr, L.ws_runs_bytes, stream))
                return rc;
        // 5. join the local run, ONE merge over all 2E bank branches into the local slots of kfo_ext
        if (fork)
            if (const int rc = order(rk, rk->as, st, fn)) return rc;
        if (const int rc = tf_ext_attn_runs_merge_edits(out_loc, K, Kl, S, H, Dh, R.n, E, inject_mask, o_bs, SD, run_flags, dtype,
                                                        wsr, L.ws_runs_bytes, stream))
            return rc;
        // 6. the halo of 2 + B messages
        if (!no_halo)
            if (const int rc = halo_exchange(rk, piv, inv_ext, kfo, B, o_bs, SD, S, slot, st, fn)) return rc;
        return 0;
    }
    // the source part of the rank's own frames on the local tensors
    const EditsLayout L = edits_layout(rk, S, H, Dh, E, dtype, mode);
    auto source_part = [&](hipStream_t on) {
        return tf_ext_attn_fwd_edits_part(q, k, v, out_loc, Kl, Kl, 0, S, H, Dh, ld, loc_strides, scale,
                                          flags | TF_ATTN_SOURCE_ONLY, dtype, E, inject_mask, 0, wsb + L.ws_src, L.ws_src_bytes,
                                          on);
    };
    El* send = reinterpret_cast<El*>(wsb + L.send);
    El* recv = reinterpret_cast<El*>(wsb + L.recv);

    if (mode == TF_RANK_HEADS) {
        TF_ARG(ld_q == ld, TF_ERR_SHAPE, "%s: the head re-sharding packs q, k, v with one token stride", fn);
        const int Hl = H / W;
        const int64_t hd = D / W, Shd = (int64_t)S * hd;
        El* send2 = reinterpret_cast<El*>(wsb + L.send2);
        El* recv2 = reinterpret_cast<El*>(wsb + L.recv2);
        // ---- ONE pack: head group w of [q slots | k slots | v_1 .. v_2E], frame-major; the inverse norms in the same launch
        const int ns = 2 * nq + 2 * E;
        for (int i = 0; i < nq; ++i) {
            slabs[i] = qe + slots[i] * q_bs, fss[i] = q_fs;
            slabs[nq + i] = ke + slots[i] * k_bs, fss[nq + i] = k_fs;
        }
        for (int j = 0; j < 2 * E; ++j) slabs[2 * nq + j] = ve + (1 + j) * v_bs, fss[2 * nq + j] = v_fs;
        if (const int rc = do_pack(slabs, fss, ns, send, W, Kl, S, (int)hd, ld, piv_loc, inv_loc, (int64_t)Kl * S, (int)D,
                                   dtype, stream))
            return rc;
        // ---- the source part beside the first exchange where it is a streaming launch (the single-edit rule: forked HERE,
        //      behind the pack and in front of the exchange, joined in front of the second exchange); where it takes the fused
        //      small-problem kernel, in line behind the exchange.  Every rank of the block must decide alike: the decision of
        //      the source-only call (ext_attn.hip) with the largest local run ceil(K / W) standing for Kl.
        TfAttnSet probe{};
        probe.q = q, probe.k = k, probe.v = v, probe.out = out_loc;
        probe.q_bs = q_bs, probe.q_fs = q_fs, probe.ld_q = ld_q, probe.k_bs = k_bs, probe.k_fs = k_fs;
        probe.v_bs = v_bs, probe.v_fs = v_fs, probe.ld = ld, probe.o_bs = o_bs, probe.o_fs = SD;
        probe.H = H, probe.Kq = probe.Kb = (K + W - 1) / W, probe.q_frame0 = 0, probe.b0 = 0, probe.nb = 1;
        const int src_flags = flags | TF_ATTN_SOURCE_ONLY | (nq == 1 ? TF_ATTN_INJECT : 0);   // (every edit injects)
        const bool src_fused = tf_attn_fused_plan(&probe, 1, S, Dh, dtype, src_flags).use != 0;
        const bool fork = !src_fused && src_aux_enabled() && !tf_plan_rec;   // (a recorded plan lists the in-line order)
        if (fork) {
            if (const int rc = order(rk, st, rk->as, fn)) return rc;
            if (const int rc = source_part(rk->as)) return rc;
        }
        // ---- ONE first all-to-all; every collective of the communicator on the caller's stream
        if (const int rc = do_a2a(rk->comm, send, recv, own, cnt, ns, Shd, dtype, st)) return rc;
        // ---- the bank part of every edit on this rank's head group over all K frames: reads `recv` [K][ns][S][hd], writes
        //      `send2` [K][2E][S][hd], both in place
        const int64_t fs_r = ns * Shd;
        const El* qb = slab(recv, 0, b0, Shd);
        const El* kb = slab(recv, nq, b0, Shd);
        const El* vb = slab(recv, 2 * nq, 1, Shd);
        El* ob = const_cast<El*>(slab(send2, 0, 1, Shd));
        const int64_t strides[9] = {Shd, fs_r, Shd, fs_r, Shd, fs_r, Shd, 2 * E * Shd, hd};
        if (const int rc = tf_ext_attn_fwd_edits_part(qb, kb, vb, ob, K, K, 0, S, Hl, Dh, hd, strides, scale,
                                                      flags | TF_ATTN_BANK_ONLY, dtype, E, inject_mask, 1, wsb + L.ws_bank,
                                                      L.ws_bank_bytes, stream))
            return rc;
        if (fork) {
            if (const int rc = order(rk, rk->as, st, fn)) return rc;
        } else if (const int rc = source_part(st)) {
            return rc;
        }
        // ---- ONE second all-to-all: the outputs back to the frame owners; ONE unpack into the 2E bank slabs of kfo_ext
        if (const int rc = do_a2a(rk->comm, send2, recv2, cnt, own, 2 * E, Shd, dtype, st)) return rc;
        void* dsts[2 * TF_MAX_EDITS];
        int64_t dfs[2 * TF_MAX_EDITS];
        for (int j = 0; j < 2 * E; ++j) dsts[j] = out_loc + (1 + j) * o_bs, dfs[j] = SD;
        if (const int rc = do_unpack(recv2, dsts, dfs, 2 * E, W, Kl, S, (int)hd, D, stream)) return rc;
    } else {
        // ---- ONE pack (W = 1) of exactly the compact k slots and the 2E value slabs: the source's v and every q stay at home
        const int ns = nq + 2 * E;
        for (int i = 0; i < nq; ++i) slabs[i] = ke + slots[i] * k_bs, fss[i] = k_fs;
        for (int j = 0; j < 2 * E; ++j) slabs[nq + j] = ve + (1 + j) * v_bs, fss[nq + j] = v_fs;
        if (const int rc = do_pack(slabs, fss, ns, send, 1, Kl, S, (int)D, ld, piv_loc, inv_loc, (int64_t)Kl * S, (int)D,
                                   dtype, stream))
            return rc;
        // ---- q in the same compact layout: the dense tensor IS that layout unless the mask is mixed; then the slots are
        //      copied into the staging region [Kl][nq][S][D] (the pack kernel with W = 1, one launch)
        const El* qp = qe;
        int64_t cq_bs = q_bs, cq_fs = q_fs, cq_ld = ld_q;
        if (mixed) {
            El* stage = reinterpret_cast<El*>(wsb + L.stage);
            const void* qs[1 + 2 * TF_MAX_EDITS];
            int64_t qfs[1 + 2 * TF_MAX_EDITS];
            for (int i = 0; i < nq; ++i) qs[i] = qe + slots[i] * q_bs, qfs[i] = q_fs;
            if (!tf_plan_note("qcompact[ns=%d]", nq))
                if (const int rc = tf_head_pack(qs, qfs, nq, stage, 1, Kl, S, (int)D, ld_q, 2, stream)) return rc;
            qp = stage, cq_bs = SD, cq_fs = nq * SD, cq_ld = D;
        }
        // ---- ONE gather into [K][ns][S][D], on the caller's stream: the attention needs it at once
        if (const int rc = do_gather(rk->comm, send, recv, cnt, ns, SD, dtype, st)) return rc;
        // ---- the bank part of the local keyframes' queries on the gathered buffer in place, then the source part
        const int64_t fs_r = ns * SD;
        const El* kb = slab(recv, 0, b0, SD);
        const El* vb = slab(recv, nq, 1, SD);
        const int64_t strides[9] = {cq_bs, cq_fs, SD, fs_r, SD, fs_r, o_bs, SD, cq_ld};
        if (const int rc = tf_ext_attn_fwd_edits_part(qp, kb, vb, out_loc, K, Kl, rk->kf0, S, H, Dh, D, strides, scale,
                                                      flags | TF_ATTN_BANK_ONLY, dtype, E, inject_mask, 1, wsb + L.ws_bank,
                                                      L.ws_bank_bytes, stream))
            return rc;
        if (const int rc = source_part(st)) return rc;
    }

    // ---- neighbour halo: 2 + B messages in ONE grouped exchange
    if (!no_halo)
        if (const int rc = halo_exchange(rk, piv, inv_ext, kfo, B, o_bs, SD, S, slot, st, fn)) return rc;
    return 0;
}

// The sequence one call issues, recorded by the call itself on a rank that owns no device object (host only).
extern "C" int tf_rank_pivotal_edits_plan(int world, int rank, int K, int S, int H, int Dh, int n_edits, unsigned inject_mask,
                                          int mode, int flags, int dtype, char* buf, size_t len) {
    TF_ARG(world >= 1 && world <= TF_MAX_WORLD && rank >= 0 && rank < world && K >= world && S > 0 && H > 0 && Dh > 0,
           TF_ERR_SHAPE, "tf_rank_pivotal_edits_plan: rank %d of %d over %d keyframes, S=%d H=%d Dh=%d", rank, world, K, S, H, Dh);
    tf_rank rk{};
    partition(&rk, K, world, rank);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 40);   // never dereferenced
    const int64_t D = (int64_t)H * Dh, SD = (int64_t)S * D;
    const int64_t strides[8] = {rk.Kl * SD, SD, rk.Kl * SD, SD, rk.Kl * SD, SD, D, D};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_rank_pivotal_edits(&rk, ph, ph, ph, strides, ph, static_cast<float*>(ph), ph, S, H, Dh, 1.0f, flags,
                                         dtype, mode, 0, n_edits, inject_mask, ph, (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_rank_pivotal_edits_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// ---------------------------------------------------------------------------------------------
// One rank's pivotal pass of a MULTI-EDIT batch over a windowed / anchored bank (include/tokenflow_hip.h): the schedule of
// tf_rank_pivotal_frame_sets with the payload of tf_rank_pivotal_edits(TF_RANK_BANK) -- per block ONE pack, ONE sparse exchange,
// ONE bank part over all E edits (tf_ext_attn_fwd_windows_edits_part / tf_ext_attn_fwd_frame_sets_edits_part), the source part
// beside the exchange.  The geometry does not depend on E: window_geometry / frame_set_geometry as in the single-edit calls.
namespace {

struct WinEditsLayout {   // exchange buffers of one call inside the caller's workspace; slab counts at their largest
    size_t send, recv, stage, ws_bank, ws_src, total;
    size_t ws_bank_bytes, ws_src_bytes;
};

WinEditsLayout window_edits_layout(const tf_rank* rk, const WinGeom& g, int S, int H, int Dh, int E, int dtype) {
    const size_t eb = 2, D = (size_t)H * Dh;
    WinEditsLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += up256(bytes);
        return at;
    };
    // [k slots | v_1 .. v_2E]: 4E slabs where no edit injects; the compact q of a mixed mask is staged (< 2E slots)
    L.send = take((size_t)g.send_total * 4 * E * S * D * eb);
    L.recv = take((size_t)g.F * 4 * E * S * D * eb);
    L.stage = take((size_t)rk->Kl * 2 * E * S * D * eb);
    // the bank part and the source part may run concurrently: a workspace each
    L.ws_bank_bytes = tf_ext_attn_edits_workspace_bytes(g.F, S, H, Dh, E, dtype);
    L.ws_src_bytes = tf_ext_attn_edits_workspace_bytes(rk->Kl, S, H, Dh, E, dtype);
    L.ws_bank = take(L.ws_bank_bytes);
    L.ws_src = take(L.ws_src_bytes);
    L.total = off;
    return L;
}

// the geometry of a call: the anchored one, or -- without anchors -- the windowed one with its segments as contiguous masks
bool window_edits_geometry(const tf_rank* rk, int R, const int* anc, int na, SetGeom* G) {
    if (na) return frame_set_geometry(rk, R, anc, na, G);
    *G = SetGeom{};
    G->w = window_geometry(rk, R);
    G->q_frame0 = G->w.hl;
    for (int p = 0; p < rk->world; ++p) {
        const int n = G->w.seg_n[p];
        G->send_mask[p] = n ? (n == 64 ? ~(uint64_t)0 : ((uint64_t)1 << n) - 1) << G->w.seg_f0[p] : 0;
    }
    return G->w.F < (1 << 16);
}

}  // namespace

extern "C" size_t tf_rank_pivotal_frame_sets_edits_workspace_bytes(const tf_rank* rk, int S, int H, int Dh, int dtype, int radius,
                                                                   const int* anchors, int n_anchors, int n_edits) {
    if (n_edits < 1 || n_edits > TF_MAX_EDITS) return 0;
    // never below either parent's for the same arguments, 0 for what either refuses
    const size_t sets = tf_rank_pivotal_frame_sets_workspace_bytes(rk, S, H, Dh, dtype, radius, anchors, n_anchors);
    if (!sets) return 0;
    const size_t edits = tf_rank_pivotal_edits_workspace_bytes(rk, S, H, Dh, n_edits, dtype);
    if (!edits) return 0;
    const size_t base = sets > edits ? sets : edits;
    if (n_edits == 1 || rk->world == 1 || radius >= rk->K - 1 || rk->Kl > TF_MAX_WINDOW_FRAMES) return base;
    int anc[MAX_ANCHORS], na = 0;
    if (n_anchors) sorted_anchors("", rk->K, anchors, n_anchors, anc, &na);   // (validated by the size query above)
    SetGeom G;
    if (!window_edits_geometry(rk, radius, anc, na, &G)) return 0;
    const size_t own = window_edits_layout(rk, G.w, S, H, Dh, n_edits, dtype).total;
    return own > base ? own : base;
}

extern "C" int tf_rank_pivotal_frame_sets_edits(tf_rank* rk, const void* q, const void* k, const void* v, const int64_t* st_in,
                                                void* piv_ext, float* inv_ext, void* kfo_ext, int S, int H, int Dh, float scale,
                                                int flags, int dtype, int mode, int slot, int radius, const int* anchors,
                                                int n_anchors, int n_edits, unsigned inject_mask, void* ws, size_t ws_bytes,
                                                void* stream) {
    const char* const fn = "tf_rank_pivotal_frame_sets_edits";
    const bool no_halo = (mode & TF_RANK_NO_HALO) != 0, want_inv = (mode & TF_RANK_INV_NORM) != 0;
    const int mods = mode & (TF_RANK_NO_HALO | TF_RANK_INV_NORM), base = mode & ~(TF_RANK_NO_HALO | TF_RANK_INV_NORM);
    // ---- arguments first: nothing below this block's end has touched the device
    TF_ARG(rk && q && k && v && st_in && kfo_ext && ws && (no_halo || (piv_ext && inv_ext)) && (anchors || n_anchors == 0),
           TF_ERR_NULL, "%s: null pointer", fn);
    TF_ARG(n_anchors >= 0 && n_anchors <= MAX_ANCHORS, TF_ERR_SHAPE, "%s: %d anchors (0 .. %d)", fn, n_anchors, MAX_ANCHORS);
    TF_ARG(n_edits >= 1 && n_edits <= TF_MAX_EDITS, TF_ERR_SHAPE, "%s: n_edits=%d (1 .. %d)", fn, n_edits, TF_MAX_EDITS);
    TF_ARG(!(flags & TF_ATTN_INJECT), TF_ERR_SHAPE, "%s: TF_ATTN_INJECT beside a mask (the mask is the injection state)", fn);
    TF_ARG(!(inject_mask >> n_edits), TF_ERR_SHAPE, "%s: inject_mask=0x%x has bits at or above n_edits=%d", fn, inject_mask,
           n_edits);
    TF_ARG(!(flags & (TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY)), TF_ERR_SHAPE, "%s: the part flags are the executor's own", fn);
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "%s: dtype %d (bf16/f16 only)", fn, dtype);
    TF_ARG(radius >= 0, TF_ERR_SHAPE, "%s: radius %d (>= 0)", fn, radius);
    TF_ARG(base == TF_RANK_BANK, TF_ERR_SHAPE,
           "%s: mode %d (a windowed multi-edit pass has the bank form only: TF_RANK_BANK with TF_RANK_NO_HALO / TF_RANK_INV_NORM)",
           fn, base);
    TF_ARG(slot >= 0 && slot < TF_RANK_SLOTS, TF_ERR_SHAPE, "%s: slot %d outside [0, %d)", fn, slot, TF_RANK_SLOTS);
    TF_ARG(!(want_inv && no_halo), TF_ERR_SHAPE, "%s: TF_RANK_INV_NORM needs the propagation state (no TF_RANK_NO_HALO)", fn);
    int anc[MAX_ANCHORS], na = 0;
    if (const int rc = sorted_anchors(fn, rk->K, anchors, n_anchors, anc, &na)) return rc;
    if (n_edits == 1)   // one edit: the single-edit anchored / windowed pass -- the same launches, the same bits
        return tf_rank_pivotal_frame_sets(rk, q, k, v, st_in, piv_ext, inv_ext, kfo_ext, S, H, Dh, scale,
                                          flags | (inject_mask ? TF_ATTN_INJECT : 0), dtype, mode, slot, radius, anchors, n_anchors,
                                          ws, ws_bytes, stream);
    if (radius >= rk->K - 1)   // every window is the whole bank: the multi-edit bank pass whatever the anchors
        return tf_rank_pivotal_edits(rk, q, k, v, st_in, piv_ext, inv_ext, kfo_ext, S, H, Dh, scale, flags, dtype,
                                     TF_RANK_BANK | mods, slot, n_edits, inject_mask, ws, ws_bytes, stream);
    TF_ARG(rk->Kl <= TF_MAX_WINDOW_FRAMES, TF_ERR_SHAPE, "%s: %d local keyframes (at most %d carry a window or set)", fn, rk->Kl,
           TF_MAX_WINDOW_FRAMES);
    TF_ARG(!(flags & TF_ATTN_FOLD_SCALE), TF_ERR_SHAPE, "%s: TF_ATTN_FOLD_SCALE has no windowed form", fn);
    SetGeom G;
    TF_ARG(window_edits_geometry(rk, radius, anc, na, &G), TF_ERR_SHAPE,
           "%s: the extended bank of rank %d exceeds %d frames (anchors: a set is a 64-bit mask; none: below 65536)", fn, rk->rank,
           na ? 64 : 65535);
    const size_t ws_need =
        tf_rank_pivotal_frame_sets_edits_workspace_bytes(rk, S, H, Dh, dtype, radius, anchors, n_anchors, n_edits);
    TF_ARG(ws_need, TF_ERR_SHAPE, "%s: S=%d H=%d Dh=%d", fn, S, H, Dh);
    TF_ARG(ws_bytes >= ws_need, TF_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, ws_need);

    const int E = n_edits, B = 1 + 2 * E;
    const int W = rk->world, Kl = rk->Kl, K = rk->K, o = (W > 1 && !no_halo) ? 1 : 0;
    const int64_t D = (int64_t)H * Dh, SD = (int64_t)S * D;
    const int64_t q_bs = st_in[0], q_fs = st_in[1], k_bs = st_in[2], k_fs = st_in[3], v_bs = st_in[4], v_fs = st_in[5],
                  ld_q = st_in[6], ld = st_in[7];
    typedef unsigned short El;   // any 16-bit element: only pointer arithmetic happens here
    const El* qe = static_cast<const El*>(q);
    const El* ke = static_cast<const El*>(k);
    const El* ve = static_cast<const El*>(v);
    El* kfo = static_cast<El*>(kfo_ext);
    El* piv = static_cast<El*>(piv_ext);
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t o_bs = (int64_t)(Kl + o) * SD;   // branch stride of the halo-extended attention output
    El* out_loc = kfo + (int64_t)o * SD;           // its local slots
    if (!no_halo) rk->halo_set[slot] = false;
    // 0. the inverse norms: a launch of their own (the halo pack kernel carries none)
    if (want_inv)
        if (const int rc = do_inv_norm(piv + (int64_t)o * SD, inv_ext + (int64_t)o * S, (int64_t)Kl * S, (int)D, dtype, stream))
            return rc;
    const int64_t loc_strides[9] = {q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, SD, ld_q};
    if (W == 1) {   // one rank: the single-GPU multi-edit call straight into kfo_ext (with anchors K <= 64 there)
        if (na)
            return tf_ext_attn_fwd_frame_sets_edits(q, k, v, out_loc, K, K, 0, S, H, Dh, ld, loc_strides, scale, flags, dtype, E,
                                                    inject_mask, G.sets, ws, ws_bytes, stream);
        return tf_ext_attn_fwd_windows_edits(q, k, v, out_loc, K, K, 0, S, H, Dh, ld, loc_strides, scale, flags, dtype, E,
                                             inject_mask, G.w.win_lo, G.w.win_n, ws, ws_bytes, stream);
    }
    const WinEditsLayout L = window_edits_layout(rk, G.w, S, H, Dh, E, dtype);
    El* send = reinterpret_cast<El*>(wsb + L.send);
    El* recv = reinterpret_cast<El*>(wsb + L.recv);
    // the compact q / k layout of tf_ext_attn_fwd_edits_part: slot 0 the source where some edit injects, then (uncond, cond) of
    // every edit that does not, ascending; b0 = the first slot that exists
    int slots[1 + 2 * TF_MAX_EDITS], nq = 0;
    if (inject_mask) slots[nq++] = 0;
    for (int e = 0; e < E; ++e)
        if (!((inject_mask >> e) & 1u)) slots[nq++] = 1 + 2 * e, slots[nq++] = 2 + 2 * e;
    const int b0 = inject_mask ? 0 : 1;
    const bool mixed = inject_mask && nq > 1;   // some edits inject, some do not
    auto slab = [](const El* buf, int64_t first_slab, int first_branch, int64_t unit) {
        return reinterpret_cast<const El*>(reinterpret_cast<uintptr_t>(buf) +
                                           (uintptr_t)((first_slab - first_branch) * unit * (int64_t)sizeof(El)));
    };
    // 1. ONE pack of what PEERS read: the compact k slots and the 2E value slabs, per peer the members of its mask in ascending
    //    order; the source's v and every q stay at home.  Under a mixed mask the same launch copies the compact q slots into the
    //    staging region [nq][Kl][S][D] (the dense q IS the compact layout otherwise)
    const void* slabs[4 * TF_MAX_EDITS];
    int64_t fss[4 * TF_MAX_EDITS];
    const int ns = nq + 2 * E;
    for (int i = 0; i < nq; ++i) slabs[i] = ke + slots[i] * k_bs, fss[i] = k_fs;
    for (int j = 0; j < 2 * E; ++j) slabs[nq + j] = ve + (1 + j) * v_bs, fss[nq + j] = v_fs;
    const void* qs[1 + 2 * TF_MAX_EDITS];
    int64_t qfs[1 + 2 * TF_MAX_EDITS];
    const El* qp = qe;
    int64_t cq_bs = q_bs, cq_fs = q_fs, cq_ld = ld_q;
    El* stage = reinterpret_cast<El*>(wsb + L.stage);
    if (mixed) {
        for (int i = 0; i < nq; ++i) qs[i] = qe + slots[i] * q_bs, qfs[i] = q_fs;
        qp = stage, cq_bs = (int64_t)Kl * SD, cq_fs = SD, cq_ld = D;
    }
    if (!tf_plan_note("edit_pack[ns=%d,nq=%d]", ns, mixed ? nq : 0))
        if (const int rc = tf_edit_halo_pack(slabs, fss, ns, send, W, G.send_mask, mixed ? qs : nullptr, mixed ? qfs : nullptr,
                                             mixed ? nq : 0, mixed ? stage : nullptr, Kl, S, (int)D, ld, ld_q, dtype, stream))
            return rc;
    // 2. the source part of the local frames (table-free), on the auxiliary compute stream: forked behind the pack, in FRONT of
    //    the exchange, joined behind the bank part.  TOKENFLOW_RANK_SRC_AUX=0: in line behind the exchange (a recorded plan lists
    //    that order)
    auto source_part = [&](hipStream_t on) {
        return tf_ext_attn_fwd_edits_part(q, k, v, out_loc, Kl, Kl, 0, S, H, Dh, ld, loc_strides, scale,
                                          flags | TF_ATTN_SOURCE_ONLY, dtype, E, inject_mask, 0, wsb + L.ws_src, L.ws_src_bytes,
                                          on);
    };
    const bool fork = src_aux_enabled() && !tf_plan_rec;
    if (fork) {
        if (const int rc = order(rk, st, rk->as, fn)) return rc;
        if (const int rc = source_part(rk->as)) return rc;
    }
    // 3. ONE sparse exchange on the caller's stream: the receive buffer is the extended bank in ascending order
    if (const int rc = do_a2a_rows(rk, send, recv, G.w, ns, SD, dtype, st)) return rc;
    if (!fork)
        if (const int rc = source_part(st)) return rc;
    // 4. the bank part of ALL edits over the receive buffer [F][ns][S][D] in place: q / k compact, v and out addressed as
    //    [source | uncond_1 | cond_1 | ...]; no anchors: the windows form, anchors: the set form
    const int64_t fs_r = ns * SD;
    const El* kb = slab(recv, 0, b0, SD);
    const El* vb = slab(recv, nq, 1, SD);
    const int64_t strides[9] = {cq_bs, cq_fs, SD, fs_r, SD, fs_r, o_bs, SD, cq_ld};
    if (na) {
        if (const int rc = tf_ext_attn_fwd_frame_sets_edits_part(qp, kb, vb, out_loc, G.w.F, Kl, G.q_frame0, S, H, Dh, D, strides,
                                                                 scale, flags | TF_ATTN_BANK_ONLY, dtype, E, inject_mask, 1, G.sets,
                                                                 wsb + L.ws_bank, L.ws_bank_bytes, stream))
            return rc;
    } else if (const int rc = tf_ext_attn_fwd_windows_edits_part(qp, kb, vb, out_loc, G.w.F, Kl, G.w.hl, S, H, Dh, D, strides, scale,
                                                                 flags | TF_ATTN_BANK_ONLY, dtype, E, inject_mask, 1, G.w.win_lo,
                                                                 G.w.win_n, wsb + L.ws_bank, L.ws_bank_bytes, stream)) {
        return rc;
    }
    // 5. join
    if (fork)
        if (const int rc = order(rk, rk->as, st, fn)) return rc;
    // 6. the neighbour halo of 2 + B messages
    if (!no_halo)
        if (const int rc = halo_exchange(rk, piv, inv_ext, kfo, B, o_bs, SD, S, slot, st, fn)) return rc;
    return 0;
}

// The sequence one call issues, recorded by the call itself on a rank that owns no device object (host only).
extern "C" int tf_rank_pivotal_frame_sets_edits_plan(int world, int rank, int K, int S, int H, int Dh, int radius,
                                                     const int* anchors, int n_anchors, int n_edits, unsigned inject_mask, int mode,
                                                     int flags, int dtype, char* buf, size_t len) {
    TF_ARG(world >= 1 && world <= TF_MAX_WORLD && rank >= 0 && rank < world && K >= world && S > 0 && H > 0 && Dh > 0,
           TF_ERR_SHAPE, "tf_rank_pivotal_frame_sets_edits_plan: rank %d of %d over %d keyframes, S=%d H=%d Dh=%d", rank, world, K,
           S, H, Dh);
    tf_rank rk{};
    partition(&rk, K, world, rank);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 40);   // never dereferenced
    const int64_t D = (int64_t)H * Dh, SD = (int64_t)S * D;
    const int64_t strides[8] = {rk.Kl * SD, SD, rk.Kl * SD, SD, rk.Kl * SD, SD, D, D};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_rank_pivotal_frame_sets_edits(&rk, ph, ph, ph, strides, ph, static_cast<float*>(ph), ph, S, H, Dh, 1.0f, flags,
                                                    dtype, mode, 0, radius, anchors, n_anchors, n_edits, inject_mask, ph,
                                                    (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_rank_pivotal_frame_sets_edits_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}
