"""Frame-sharded multi-GPU execution of the hot path (one process per GPU).

The reference is single-process (no parallelism of any kind); this is new.
Rank r of W owns the contiguous chunks [r*C/W, (r+1)*C/W) of the video and the keyframes
drawn from them (K = C keyframes, one per chunk, run_tokenflow_pnp.py:224).  Per block there
are two exchange steps, both through torch.distributed (backend "nccl" = RCCL over xGMI on
MI355X; "gloo" in the CPU tests) -- or, with `FrameShard(K, comm=HipComm(...))`, through the library's own C-ABI
exchange entry points (tokenflow_amd/comm.py: RCCL without torch.distributed on the data path; the calls run on a
side stream ordered against the compute stream with events):

 1. pivotal pass -- every query of a keyframe attends to the keys/values of ALL K keyframes
    of its branch (tokenflow_utils.py:133-138).  Two exchange patterns, same results:

    "heads" (default when heads % W == 0): the bank branches are re-sharded from frames to
        heads for the attention and back.  Rank r sends, to every rank w, head group w of its
        keyframes' q, k, v (uncond + cond; with q/k injection, 124-130, the source q, k and
        the uncond/cond v), receives head group r of everybody's keyframes, runs
        `ops.ext_attn(part="bank")` on [3,K,S,D/W], and returns the outputs the same way.
        Two all-to-alls per block; a rank sends (6+2)*(W-1)/W (injection: (4+2)*(W-1)/W) of
        its local [K/W,S,D] slabs -- under 8 local slabs whatever W -- and on a fully
        connected xGMI mesh every pair uses its own link.  The source branch (own-frame
        keys only, 173/177) never leaves the rank: `ops.ext_attn(part="source")` runs on the
        local frames while the first exchange is in flight.
    "bank": ONE all-gather of the key/value slabs of the local keyframes (6 slabs of [K/W,S,D]
        per rank; 4 with injection), packed by one launch and gathered straight into the
        [K,slabs,S,D] buffer that ONE `ops.ext_attn_views(q_local, k_bank, v_bank, q_frame0=...)`
        call reads in place, computing only the local keyframes' queries.  A rank receives
        6*(W-1) local slabs -- several times the "heads" volume at W = 8 -- for one collective,
        one pack and one attention call per block instead of two collectives, pack, unpack and two
        calls: chosen per block (`auto_mode`) where the exchange is latency-bound (the mid block),
        and whenever the heads do not divide over the ranks.
    "bank_runs" (opt-in: `bank_runs=True` / TOKENFLOW_SHARD_BANK_RUNS=1 lets `auto_mode` answer it in place of "bank"
        for S >= BANK_RUNS_MIN_S; or mode="bank_runs"): the bank form in RUNS of keyframes.  Only the slabs PEERS read
        are gathered (4 instead of 6; 3 instead of 4 with injection: the source branch's k and v stay at home), the
        LOCAL run -- source branch + bank branches against the rank's own keyframes, read in place -- needs nothing
        from the gather and starts in front of it (NativeShard: on the auxiliary compute stream), the remote runs
        (frames left of the rank's own, then right) follow when the gather has landed, and one merge folds the runs'
        partial results in the fixed order local, left, right (`ops.ext_attn_runs_views`).  The merge re-associates
        fp32 sums: this mode equals a single-process `ops.ext_attn_runs` with the same runs bit for bit and the
        oracle within the attention bound -- NOT the bit-stable single-GPU call.  For a multi-edit batch the mode
        needs an opt-in of its own (`edit_runs=True` / TOKENFLOW_SHARD_EDIT_RUNS=1): the gather of the multi-edit "bank"
        form, the same runs through `ops.ext_attn_runs_edits_views`, the same guarantee per edit.  With
        `edit_runs_multi_v=True` / TOKENFLOW_SHARD_EDIT_RUNS_MULTI_V=1 on top of it, pairs of injecting edits share one
        four-bank launch per run (head dims 40 and 64): those edits then equal `ops.ext_attn_runs_edits(multi_v=True)` bit
        for bit and the oracle within the attention bound.

 2. propagation passes -- chunk c needs keyframes c and c-1 (331-333): the first local chunk's
    left neighbour lives on rank r-1, so each rank sends its LAST keyframe's pivot features,
    inverse norms and attention output to rank r+1: one grouped point-to-point exchange per block
    (`pivotal_block`, the in-place form: the block's propagation state lives in halo-extended buffers
    from `ext_alloc` that the producers write directly) or two (`halo_start` before the attention,
    `halo_finish` after it), on a communicator / process group and side stream of its own when the
    host provides one (`halo_comm` / `halo_group`).

Three hosts run this sequence with identical results: `FrameShard` over torch.distributed, `FrameShard`
over the library's exchange entry points (`comm=`), and `NativeShard` (bottom of this file), whose
pivotal pass of a block is ONE library call (tf_rank_pivotal, csrc/rank_exec.hip; `NativeEditShard`: the same for multi-edit
batches, tf_rank_pivotal_edits).  The hook API
reaches them through `tokenflow_amd.hooks.register_frame_shard`.

Work is partitioned, not re-associated: every output element is produced by exactly the same
kernel arithmetic as on one GPU IN THE BIT-STABLE MODE (the attention of one (query, head) visits the
K frames in the same order, whoever computes it).  That is the default: `FrameShard` asks the attention
for its one-pass form (TF_ATTN_NO_SPLIT), in which kernel choice and in-workgroup key split are functions
of the shape alone; a sharded run then equals a single-GPU run with TOKENFLOW_ATTN_NO_SPLIT=1 (and a
world-1 `FrameShard`) bit for bit.  The single-GPU DEFAULT mode is free to choose per grid (large grids of
<= 256-token frames run without the key split: cfg2 level 2, +26 % faster there, profiles/r05_attn_nosplit_ab.txt)
and agrees with the sharded results within the attention's parity bound, like any two correct launches.
`FrameShard(..., attn_split=True)` (or TOKENFLOW_SHARD_ATTN_SPLIT=1) lets the small grid of a rank split
the bank over extra workgroups and merge: faster, held to the ORACLE's bound.
"""
import collections
import ctypes
import os
from typing import Optional

import torch
import torch.distributed as dist

from . import ops


class _Done:
    def wait(self):
        return True


class _EventRing:
    """A few reusable events for ordering the exchange stream against the compute stream.  Creating a
    `torch.cuda.Event` costs tens of microseconds on this stack (`Stream.wait_stream` creates one per call: it was
    half of a rank's host time per block, profiles/r03_rank_step_v1.txt); recording an existing one costs ~1 us.  A
    wait captures the record that is current when it is issued, so an event may be re-recorded while earlier waits on
    it are still queued; a handle that is waited on only after its event has been re-recorded (the ring wrapped)
    waits for that LATER point of the same in-order stream -- still correct, never early.  That argument needs every
    event of a ring to be recorded on ONE stream: there is one ring per recording stream (the compute stream's "start"
    events, each side stream's "done" events), never a shared one.  256 events cover more than two passes over the 16
    blocks (<= 6 per block), longer than any handle lives (a halo is waited for in the propagation pass that follows
    its pivotal pass)."""

    def __init__(self, n: int = 256):
        self._ev = [torch.cuda.Event() for _ in range(n)]
        self._i = 0

    def next(self):
        e = self._ev[self._i]
        self._i = (self._i + 1) % len(self._ev)
        return e


class _StreamWork:
    """Completion handle of exchanges issued on the side stream: wait() orders the CURRENT stream behind them
    (no host blocking -- the semantics of a c10d work object on the NCCL backend)."""

    def __init__(self, event, device):
        self.event, self.device = event, device

    def wait(self):
        # current_stream(device): the device-less form resolves the device through torch.cuda.is_available(),
        # ~30 us per call on this stack -- it was two thirds of a rank's host time per block
        torch.cuda.current_stream(self.device).wait_event(self.event)
        return True


def _all_to_all(recv: torch.Tensor, send: torch.Tensor, group, out_rows=None, in_rows=None, async_op: bool = False):
    """dist.all_to_all_single over dim 0 (row counts per peer; None = equal).  gloo (development boxes, the
    single-GPU tests) moves host memory only, so device tensors are staged through the host there.  RCCL
    takes the device buffers directly."""
    if send.is_cuda and dist.get_backend(group) == "gloo":
        host = torch.empty(recv.shape, dtype=recv.dtype)
        dist.all_to_all_single(host, send.cpu(), out_rows, in_rows, group=group)
        recv.copy_(host)
        return _Done() if async_op else None
    return dist.all_to_all_single(recv, send, out_rows, in_rows, group=group, async_op=async_op)


WindowHaloPlan = collections.namedtuple(
    "WindowHaloPlan", "K world rank radius counts offsets kf0 Kl lo hi hl hr F send recv send_rows recv_rows windows")


def window_halo_plan(K: int, world: int, rank: int, radius: int) -> WindowHaloPlan:
    """Exchange geometry of a sliding-window bank on a frame shard (pure arithmetic; csrc/rank_exec.hip computes the same from
    the same four numbers).  Rank r owns the keyframes [kf0, kf0 + Kl) (`FrameShard.counts` / `offsets`); with radius R it reads
    the global frames [lo, hi) = [max(0, kf0 - R), min(K, kf0 + Kl + R)): hl = kf0 - lo halo frames on the left, hr on the
    right, F = hl + Kl + hr in all.
      send[p] = (first LOCAL frame, frames) of own(r) & [lo_p, hi_p): what peer p reads of this rank's frames (for R > Kl a
                frame goes to several peers); send[r] = (0, Kl), the rank's own frames as its self rows
      recv[p] = (first GLOBAL frame, frames) of own(p) & [lo, hi): what arrives from peer p -- in rank order these are the
                frames lo .. hi - 1 in ascending order, so the receive buffer of ONE row all-to-all IS the extended bank
      send_rows / recv_rows: the frame counts of the two, the row counts of that exchange
      windows[i] = (first frame, frames) of local query i (global keyframe kf0 + i) in the extended bank's coordinates:
                `ops.bank_windows(K, R)[kf0 + i]` shifted by -lo; the queries are the bank frames hl .. hl + Kl - 1."""
    K, W, r, R = int(K), int(world), int(rank), int(radius)
    if W < 1 or not 0 <= r < W or K < W:
        raise ValueError(f"window_halo_plan: rank {r} of {W} over {K} keyframes (every rank owns at least one)")
    if R < 0:
        raise ValueError(f"window_halo_plan: radius={R} (>= 0)")
    counts = [K // W + (1 if p < K % W else 0) for p in range(W)]
    offsets = [sum(counts[:p]) for p in range(W)]
    reach = lambda p: (max(0, offsets[p] - R), min(K, offsets[p] + counts[p] + R))      # noqa: E731
    kf0, Kl = offsets[r], counts[r]
    lo, hi = reach(r)
    send, recv = [], []
    for p in range(W):
        a, b = max(offsets[p], lo), min(offsets[p] + counts[p], hi)
        recv.append((a, b - a) if b > a else (0, 0))
        lo_p, hi_p = reach(p)
        c, d = max(kf0, lo_p), min(kf0 + Kl, hi_p)
        send.append((c - kf0, d - c) if d > c else (0, 0))
    windows = [(w0 - lo, n) for w0, n in ops.bank_windows(K, R)[kf0:kf0 + Kl]]
    return WindowHaloPlan(K, W, r, R, counts, offsets, kf0, Kl, lo, hi, kf0 - lo, hi - kf0 - Kl, hi - lo, send, recv,
                          [n for _, n in send], [n for _, n in recv], windows)


FrameSetHaloPlan = collections.namedtuple(
    "FrameSetHaloPlan", "K world rank radius anchors counts offsets kf0 Kl lo hi U F q_frame0 send recv send_rows recv_rows sets")


def _anchor_list(what: str, anchors, K: int) -> list:
    """The anchors of a call as a sorted list of distinct ints inside [0, K) (None = none)."""
    out = set()
    for a in (anchors or ()):
        if isinstance(a, bool) or int(a) != a or not 0 <= int(a) < K:
            raise ValueError(f"{what}: anchor {a!r} (keyframe indices 0 <= a < {K})")
        out.add(int(a))
    return sorted(out)


def frame_set_halo_plan(K: int, world: int, rank: int, radius: int, anchors=()):
    """Exchange geometry of an ANCHORED sliding-window bank on a frame shard (pure arithmetic; csrc/rank_exec.hip computes the
    same from the same inputs).  `anchors`: global keyframe indices 0 <= a < K that every keyframe sees beside its window
    (duplicates are fine; K may exceed 64).  With [lo, hi) as in `window_halo_plan` rank r reads the set
    U = [lo, hi) | anchors (ascending), F = |U| <= 64 frames: a set is a 64-bit mask over the rank's EXTENDED bank.
      recv[p] = the members of U that peer p owns, ascending (GLOBAL indices) -- in rank order these are U ascending, so the
                receive buffer of ONE row all-to-all IS the extended bank [F][ns][S][D]
      send[p] = the LOCAL frames of this rank that lie in U_p, as an int mask over the Kl local frames; send[r] = all Kl
      send_rows / recv_rows: the frame counts of the two, the row counts of that exchange
      q_frame0 = the members of U below kf0: the own frames are contiguous in U, the queries are the bank frames
                q_frame0 .. q_frame0 + Kl - 1
      sets[i] = (window of global keyframe kf0 + i) | anchors, as an int mask over the POSITIONS in U
    No anchors (None, empty): the plan IS `window_halo_plan(K, world, rank, radius)`, returned as that type."""
    K, W, r, R = int(K), int(world), int(rank), int(radius)
    if W < 1 or not 0 <= r < W or K < W:
        raise ValueError(f"frame_set_halo_plan: rank {r} of {W} over {K} keyframes (every rank owns at least one)")
    if R < 0:
        raise ValueError(f"frame_set_halo_plan: radius={R} (>= 0)")
    anc = _anchor_list("frame_set_halo_plan", anchors, K)
    if not anc:
        return window_halo_plan(K, W, r, R)
    from . import _lib
    counts = [K // W + (1 if p < K % W else 0) for p in range(W)]
    offsets = [sum(counts[:p]) for p in range(W)]
    if counts[r] > _lib.TF_MAX_WINDOW_FRAMES:
        raise ValueError(f"frame_set_halo_plan: {counts[r]} local keyframes (at most {_lib.TF_MAX_WINDOW_FRAMES} carry a set)")

    def reads(p):      # U_p, ascending
        lo_p, hi_p = max(0, offsets[p] - R), min(K, offsets[p] + counts[p] + R)
        return sorted(set(range(lo_p, hi_p)) | set(anc))
    kf0, Kl = offsets[r], counts[r]
    U = reads(r)
    if len(U) > 64:
        raise ValueError(f"frame_set_halo_plan: rank {r} reads {len(U)} frames (window reach plus anchors: at most 64, a set is "
                         "a 64-bit mask over the rank's extended bank)")
    pos = {g: j for j, g in enumerate(U)}
    send, recv = [], []
    for p in range(W):
        recv.append([g for g in U if offsets[p] <= g < offsets[p] + counts[p]])
        Up = set(reads(p))
        send.append(sum(1 << i for i in range(Kl) if kf0 + i in Up))
    sets = []
    for g in range(kf0, kf0 + Kl):
        members = set(range(max(0, g - R), min(K - 1, g + R) + 1)) | set(anc)
        sets.append(sum(1 << pos[m] for m in members))
    return FrameSetHaloPlan(K, W, r, R, tuple(anc), counts, offsets, kf0, Kl, max(0, kf0 - R), min(K, kf0 + Kl + R), U, len(U),
                            pos[kf0], send, recv, [bin(m).count("1") for m in send], [len(x) for x in recv], sets)


# (an explicit "bank_runs" for several edits on a shard built without the opt-in)
_NO_EDIT_RUNS = ("FrameShard: the \"bank_runs\" pattern has no multi-edit form (use \"bank\" or \"heads\") unless the shard "
                 "opts in: edit_runs=True / TOKENFLOW_SHARD_EDIT_RUNS=1")


class FrameShard:
    """K keyframes (= chunks) over the ranks of `group` in contiguous runs; the first K % W ranks hold one more
    (cfg5's 25 chunks over 8 ranks -> 4,3,3,3,3,3,3,3)."""

    # `auto_mode` under the bank_runs opt-in: "bank_runs" in place of "bank" from this many tokens per frame on.  A run set is
    # three pre-passes, three launches and a merge where "bank" is one of each, so the coarse levels keep the one-call form.
    # profiles/r07_rank_bank_runs_ab.txt (cfg5, rank 0 and 1 of 8, native executor on the loopback transport): levels 0 and 1
    # (S = 4096, 1024) are ahead of "bank" under both wire models AND with the wire off; level 2 (S = 256) only under the wire
    # model (not measured without), level 3 a tie; a step with this threshold equals the forced "bank_runs" step within the spread.
    BANK_RUNS_MIN_S = 1024

    # Multi-edit batches (`hooks.register_edits`): every method below takes n_edits (and inject_mask where injection is an
    # argument); B = 1 + 2E branches [source | uncond_1 | cond_1 | ...].  Per block the collectives and the launches stay at
    # the single-edit count -- only their payload grows with E; n_edits = 1 issues exactly the single-edit ops.
    supports_edits = True

    def __init__(self, K: int, group: Optional[dist.ProcessGroup] = None, comm=None,
                 attn_split: Optional[bool] = None, halo_group: Optional[dist.ProcessGroup] = None, halo_comm=None,
                 bank_runs: Optional[bool] = None, edit_runs: Optional[bool] = None,
                 edit_runs_multi_v: Optional[bool] = None, window_edits: Optional[bool] = None,
                 window_edits_multi_v: Optional[bool] = None):
        # window_edits: opt-in for a MULTI-EDIT batch over a sliding-window / anchored bank (`_pivotal_window_edits`): window=
        # with n_edits > 1 runs instead of raising.  None reads TOKENFLOW_SHARD_WINDOW_EDITS.  Off: today's answers.
        if window_edits is None:
            window_edits = os.environ.get("TOKENFLOW_SHARD_WINDOW_EDITS", "0") not in ("", "0")
        self.window_edits = bool(window_edits)
        # window_edits_multi_v: the four-bank launches of that pass for pairs of injecting edits (TF_ATTN_MULTI_V at head dim
        # 40, TF_ATTN_MULTI_V64 at 64; within the attention bound, not bit-stable per edit).  Without it the pass sets
        # TF_ATTN_NO_MULTI_V.  None reads TOKENFLOW_SHARD_WINDOW_EDITS_MULTI_V.
        if window_edits_multi_v is None:
            window_edits_multi_v = os.environ.get("TOKENFLOW_SHARD_WINDOW_EDITS_MULTI_V", "0") not in ("", "0")
        self.window_edits_multi_v = bool(window_edits_multi_v)
        # bank_runs: opt-in for `auto_mode` (mode=None callers, the hook path): "bank_runs" where it would answer "bank"
        # and S >= BANK_RUNS_MIN_S.  None reads TOKENFLOW_SHARD_BANK_RUNS.  Off: today's answers.
        if bank_runs is None:
            bank_runs = os.environ.get("TOKENFLOW_SHARD_BANK_RUNS", "0") not in ("", "0")
        self.bank_runs = bool(bank_runs)
        # edit_runs: opt-in for the "bank_runs" form of a MULTI-EDIT batch (`_pivotal_bank_runs_edits`): mode="bank_runs" with
        # n_edits > 1 runs instead of raising, and -- together with bank_runs -- `auto_mode` answers "bank_runs" for
        # n_edits > 1 where it answers it for one edit.  None reads TOKENFLOW_SHARD_EDIT_RUNS.  Off: today's answers.
        if edit_runs is None:
            edit_runs = os.environ.get("TOKENFLOW_SHARD_EDIT_RUNS", "0") not in ("", "0")
        self.edit_runs = bool(edit_runs)
        # edit_runs_multi_v: opt-in for the four-bank run launches of the multi-edit "bank_runs" form (ops.ext_attn_runs_edits_views
        # multi_v= / TF_ATTN_RUN_MULTI_V: pairs of injecting edits share one softmax per run; head dims 40 and 64).  Effective
        # only with edit_runs.  None reads TOKENFLOW_SHARD_EDIT_RUNS_MULTI_V.  Off: today's launches and bits.
        if edit_runs_multi_v is None:
            edit_runs_multi_v = os.environ.get("TOKENFLOW_SHARD_EDIT_RUNS_MULTI_V", "0") not in ("", "0")
        self.edit_runs_multi_v = bool(edit_runs_multi_v)
        # attn_split: let the attention split a rank's small grid over extra workgroups and merge (faster: -15..40 %
        # on a rank's attention at 8 GPUs; results then agree with the single-GPU ones within the
        # output rounding).  Default False: one pass per bank problem, arithmetic independent of the grid, sharded
        # results equal to single-GPU results bit for bit.  None reads TOKENFLOW_SHARD_ATTN_SPLIT.
        # A WORLD-1 shard follows the same rule (it equals a world-W shard bit for bit), which means it runs the
        # bit-stable mode and loses the single-GPU default's per-grid kernel choice (+26 % at cfg2 level 2): pass
        # attn_split=True when a world-1 shard is registered for speed, not for bit stability.
        if attn_split is None:
            attn_split = os.environ.get("TOKENFLOW_SHARD_ATTN_SPLIT", "0") not in ("", "0")
        self.attn_split = bool(attn_split)
        # TOKENFLOW_SHARD_SRC_AUX=1: the source-branch attention of the head re-sharding on an auxiliary stream, beside
        # the bank attention (in-place form only).  Measured on a rank of 8 (profiles/r03_rank_step_v3.txt): no gain at
        # the coarse levels and -4 % at level 0 (its workgroups take slots from the chip-filling bank grid) -> off.
        self.src_aux = os.environ.get("TOKENFLOW_SHARD_SRC_AUX", "0") not in ("", "0")
        self.group = group
        self.comm = comm                       # tokenflow_amd.comm.HipComm: exchanges through the C ABI instead
        self._cs = None                        # its side stream
        # The neighbour halo on a communicator (and side stream) of its own: collectives of ONE RCCL communicator run
        # in issue order, so on the pivotal pass's communicator the ~10 MB halo message of block b (one xGMI link) would
        # sit in front of block b+1's first all-to-all.  None = share the pivotal pass's.
        self.halo_group, self.halo_comm = halo_group, halo_comm
        self._hs = None
        if comm is not None:
            self.world, self.rank = comm.world, comm.rank
        else:
            self.world = dist.get_world_size(group) if dist.is_initialized() else 1
            self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        if K < self.world:
            raise ValueError(f"{K} keyframes cannot be sharded over {self.world} ranks (a rank would own none)")
        self.K = K
        self.counts = [K // self.world + (1 if r < K % self.world else 0) for r in range(self.world)]
        self.offsets = [sum(self.counts[:r]) for r in range(self.world)]
        self.even = K % self.world == 0
        self.Kl = self.counts[self.rank]       # local keyframes == local chunks
        self.kf0 = self.offsets[self.rank]     # first global keyframe / chunk of this rank
        self._bufs = {}                        # exchange buffers by (tag, shape, dtype, device): reused block after block

    def _buf(self, tag, shape, dtype, device):
        """Receive / send scratch of the exchanges.  Every use is complete (the collective waited for, the consumer
        kernel enqueued on the same stream) before the next block touches the buffer again, so one buffer per shape
        serves all blocks -- and saves an allocator round trip per buffer and block on the host."""
        key = (tag, tuple(shape), dtype, device)
        b = getattr(self, "_bufs", None)
        if b is None:
            b = self._bufs = {}
        t = b.get(key)
        if t is None:
            t = b[key] = torch.empty(shape, dtype=dtype, device=device)
        return t

    def _side(self, tensors, fn, halo: bool = False):
        """HipComm path: run `fn(stream)` (RCCL calls through the C ABI, asynchronous on the stream they are handed)
        on the exchange stream, ordered after everything already enqueued on the compute stream; returns the handle
        to wait on.  No stream context manager and no device-less torch.cuda query on this path: both cost tens of
        microseconds of host time per call, several times per block."""
        if not tensors[0].is_cuda:             # host tensors (the CPU tests' stand-in comm): no streams to order
            fn(None)
            return _Done()
        dev = tensors[0].device
        cur = torch.cuda.current_stream(dev)
        if getattr(self, "_cs", None) is None:
            self._cs = torch.cuda.Stream(device=dev)
            self._ring = _EventRing()          # "start" events: recorded on the compute stream only
            self._cs_done = _EventRing()       # "done" events of the exchange stream
        side, done_ring = self._cs, self._cs_done
        if halo and getattr(self, "halo_comm", None) is not None:
            if getattr(self, "_hs", None) is None:
                self._hs = torch.cuda.Stream(device=dev)
                self._hs_done = _EventRing()   # "done" events of the halo stream
            side, done_ring = self._hs, self._hs_done
        e = self._ring.next()
        e.record(cur)
        side.wait_event(e)
        fn(side.cuda_stream)
        for t in tensors:
            t.record_stream(side)              # allocator: not reusable before the exchange stream is done with it
        done = done_ring.next()
        done.record(side)
        return _StreamWork(done, dev)

    def _on_aux(self, dev, tensors, fn):
        """Run `fn(raw stream)` on this rank's auxiliary compute stream, ordered after everything already enqueued on
        the current stream; returns the handle whose wait() orders the current stream behind it."""
        cur = torch.cuda.current_stream(dev)
        if getattr(self, "_aux", None) is None:
            self._aux = torch.cuda.Stream(device=dev)
            self._aux_ring = _EventRing(64)    # recorded on the compute stream
            self._aux_done = _EventRing(64)    # recorded on the auxiliary stream
        e = self._aux_ring.next()
        e.record(cur)
        self._aux.wait_event(e)
        fn(self._aux.cuda_stream)
        for t in tensors:
            t.record_stream(self._aux)
        done = self._aux_done.next()
        done.record(self._aux)
        return _StreamWork(done, dev)

    def _a2a(self, recv: torch.Tensor, send: torch.Tensor, out_rows=None, in_rows=None, async_op: bool = False):
        """Row all-to-all over dim 0: out_rows[p] rows arrive from peer p, in_rows[p] rows go to peer p (None = equal)."""
        comm = getattr(self, "comm", None)
        if comm is None:
            return _all_to_all(recv, send, self.group, out_rows, in_rows, async_op=async_op)
        work = self._side([recv, send], lambda st: comm.all_to_all_rows(send, recv, in_rows, out_rows, stream=st))
        if async_op:
            return work
        work.wait()
        return None

    # ------------------------------------------------------------------ pivotal pass
    def _bank_gather(self, k_local: torch.Tensor, v_local: torch.Tensor, inject: bool, peers_only: bool = False):
        """ONE collective per block: the slabs of the local keyframes that the attention reads across frames --
        without injection k and v of all three branches ([k0,k1,k2,v0,v1,v2]: the source slabs ride along so that the
        gathered buffer is the whole [3,K,S,D] bank of ONE attention call), with injection [k0,v0,v1,v2] -- are packed
        frame-major by one `tf_head_pack` launch (W = 1: a plain slab pack), gathered straight into
        [K (global frame order), slabs, S, D], and read there in place through strided views.  Runs of different
        lengths (K % W != 0) use the row form of the all-gather (no padding, no compaction copies).
        Returns (k view [3 or 1, K, S, D], v view [3, K, S, D]).
        peers_only (the "bank_runs" form): only the slabs PEERS read travel -- [k1,k2,v1,v2], with injection [k0,v1,v2];
        returns (k view [2 or 1, K, S, D] = branches 1.. or 0, v view [2, K, S, D] = branches 1.., local k view
        [3, Kl, S, D], local v view): the rank's own frames are read where they are."""
        B, S, D = k_local.shape
        Kl, K, W = self.Kl, self.K, self.world
        dev, dt = k_local.device, k_local.dtype

        def frames(t):     # [3*Kl, S, D] (token stride free) -> [3, Kl, S, D] view
            if t.stride(2) != 1 or t.stride(0) != S * t.stride(1):
                t = t.contiguous()
            return t.view(3, Kl, S, D) if t.is_contiguous() else t.unflatten(0, (3, Kl))
        k3, v3 = frames(k_local), frames(v_local)
        if k3.stride(2) != v3.stride(2):
            k3, v3 = k3.contiguous(), v3.contiguous()
        if peers_only:
            slabs = [k3[0], v3[1], v3[2]] if inject else [k3[1], k3[2], v3[1], v3[2]]
        else:
            slabs = [k3[0], v3[0], v3[1], v3[2]] if inject else [k3[0], k3[1], k3[2], v3[0], v3[1], v3[2]]
        rp = self._gather_slabs(slabs, "runs" if peers_only else "bank")
        if peers_only:
            return ((rp[0:1], rp[1:3]) if inject else (rp[0:2], rp[2:4])) + (k3, v3)
        return (rp[0:1], rp[1:4]) if inject else (rp[0:3], rp[3:6])

    def _gather_slabs(self, slabs, tag: str):
        """ONE pack (W = 1) and ONE all-gather of `slabs` ([Kl,S,D] views sharing a token stride) of the local keyframes:
        returns the [len(slabs), K, S, D] view of the receive buffer (global frame order).  The collective of `_bank_gather`."""
        Kl, K, W = self.Kl, self.K, self.world
        _, S, D = slabs[0].shape
        dev, dt = slabs[0].device, slabs[0].dtype
        ns = len(slabs)
        send = ops.head_pack(slabs, 1, out=self._buf(tag + "_send", (1, Kl, ns, S, D), dt, dev)).view(Kl, ns * S * D)
        recv = self._buf(tag + "_recv", (K, ns * S * D), dt, dev)
        comm = getattr(self, "comm", None)
        if self.even:
            if comm is None:
                if send.is_cuda and dist.get_backend(self.group) == "gloo":     # development boxes: host staging
                    host = torch.empty(recv.shape, dtype=dt)
                    dist.all_gather_into_tensor(host, send.cpu(), group=self.group)
                    recv.copy_(host)
                else:
                    dist.all_gather_into_tensor(recv, send, group=self.group)
            else:
                self._side([recv, send], lambda st: comm.allgather(send, recv, stream=st)).wait()
        elif comm is None:       # one grouped point-to-point exchange: my rows to every peer, theirs into place
            staged = send.is_cuda and dist.get_backend(self.group) == "gloo"
            src = send.cpu() if staged else send
            dst = torch.empty(recv.shape, dtype=dt) if staged else recv
            opsl = []
            for r in range(W):
                if r == self.rank:
                    continue
                peer = self._peer(r)
                opsl.append(dist.P2POp(dist.isend, src, peer, self.group))
                opsl.append(dist.P2POp(dist.irecv, dst[self.offsets[r]:self.offsets[r] + self.counts[r]], peer,
                                       self.group))
            reqs = dist.batch_isend_irecv(opsl)
            dst[self.kf0:self.kf0 + Kl].copy_(src)
            for r in reqs:
                r.wait()
            if staged:
                recv.copy_(dst)
        else:
            self._side([recv, send], lambda st: comm.allgather_rows(send, recv, self.counts, stream=st)).wait()
        return recv.view(K, ns, S, D).permute(1, 0, 2, 3)        # [ns, K, S, D] views: frame stride ns*S*D

    def auto_mode(self, heads: int, S: int, n_edits: int = 1) -> str:
        """Exchange pattern of the pivotal pass for one block.  "heads" moves the least data (under 8 local slabs
        per rank whatever W) and is the choice wherever the block has real work; it needs heads % W == 0.  "bank"
        is ONE collective and ONE attention call instead of two collectives, a pack, an unpack and two calls: the
        choice where a block is a few tens of microseconds of work (S <= 64: the mid block) and the exchange is
        latency-, not volume-bound -- and the only one when the heads do not divide over the ranks."""
        mode = "bank" if (heads % self.world or S <= 64) else "heads"
        if (mode == "bank" and getattr(self, "bank_runs", False) and S >= self.BANK_RUNS_MIN_S
                and (n_edits == 1 or getattr(self, "edit_runs", False))):
            return "bank_runs"     # opt-in (bank_runs=True / TOKENFLOW_SHARD_BANK_RUNS=1): the bank in runs, see the module text
        return mode

    def pivotal_attention(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool,
                          mode: Optional[str] = None, out4: Optional[torch.Tensor] = None, n_edits: int = 1,
                          inject_mask: Optional[int] = None, window: Optional[int] = None, anchors=None):
        """Extended attention for the local keyframes against all K keyframes -> [3*Kl,S,D].
        window = R: a sliding-window bank (`_pivotal_window`; NOT TokenFlow's result): the bank branches of keyframe g attend
        to the keyframes g - R .. g + R only, of which the rank fetches just those within R of its own run.  None, or a radius
        that covers the bank (R >= K - 1), is the pass without the keyword; one edit only unless the shard was built with
        `window_edits=True` (`_pivotal_window_edits`: n_edits > 1 in ONE windowed / anchored pass).
        anchors (beside window): GLOBAL keyframe indices every keyframe sees beside its window (`_pivotal_frame_sets`); none
        is the windowed pass itself.
        mode: "heads" | "bank" | "bank_runs" | None (= `auto_mode`, chosen per block).
        out4: a [3,Kl,S,D] view (dense frames, free branch stride) the result is written into in place -- the
        keyframe slots 1.. of a halo-extended buffer (`ext_alloc`); returned as is.
        n_edits = E > 1: a multi-edit batch, tensors [B*Kl,S,D] / out4 [B,Kl,S,D] with B = 1 + 2E; inject_mask = the
        injection state per edit (bit e = edit e uses the source's q and k; None = `inject` for every edit).  Modes "heads"
        and "bank"; the slices of edit e equal the single-edit pass on [source | uncond_e | cond_e] bit for bit in the
        one-pass form."""
        anc = self._anchors(window, anchors)
        if self._window(window, n_edits, mode) is not None:
            if int(n_edits) != 1:      # (the window_edits opt-in)
                return self._pivotal_window_edits(q_local, k_local, v_local, heads, scale, inject, int(window), anc, out4,
                                                  int(n_edits), inject_mask)
            if anc:
                return self._pivotal_frame_sets(q_local, k_local, v_local, heads, scale, inject, int(window), anc, out4)
            return self._pivotal_window(q_local, k_local, v_local, heads, scale, inject, int(window), out4)
        if n_edits != 1:
            return self._pivotal_edits(q_local, k_local, v_local, heads, scale, inject, mode, out4, int(n_edits), inject_mask)
        if self.world == 1:
            # the same mode as a rank of a larger world: a world-1 shard equals a world-W shard bit for bit by default.
            # COST: with attn_split unset this is the bit-stable mode (no_split), which gives up the single-GPU default's
            # per-grid kernel choice (cfg2 level 2: 124 against 98 us per block, profiles/r05_attn_nosplit_ab.txt).  A
            # single-GPU user who registers a world-1 shard for speed passes attn_split=True.
            ns = not self.attn_split
            if out4 is None:
                return ops.ext_attn(q_local, k_local, v_local, heads, scale, inject, no_split=ns)
            return ops.ext_attn(q_local, k_local, v_local, heads, scale, inject, out=out4.view(q_local.shape), no_split=ns)
        if mode is None:
            mode = self.auto_mode(heads, q_local.shape[1])
        if mode == "heads":
            return self._pivotal_heads(q_local, k_local, v_local, heads, scale, inject, out4)
        if mode == "bank_runs":
            return self._pivotal_bank_runs(q_local, k_local, v_local, heads, scale, inject, out4)
        return self._pivotal_bank(q_local, k_local, v_local, heads, scale, inject, out4)

    # ------------------------------------------------------------------ pivotal pass over a sliding-window bank
    supports_window = True      # `pivotal_attention` / `pivotal_block` take window= (hooks.register_bank_window(shard=True))

    def _window(self, window, n_edits: int = 1, mode=None):
        """The radius of a windowed pass, or None where the pass is the one without the keyword (no window, or one that covers
        the bank); the combinations that are out of scope raise.  The windowed pass has ONE exchange pattern: an explicit
        `mode` beside a window that does not cover the bank is an error, not ignored."""
        if window is None:
            return None
        R = int(window)
        if R < 0:
            raise ValueError(f"FrameShard: window={window} (a radius >= 0, or None for the whole bank)")
        if R >= self.K - 1:
            return None
        if mode is not None:
            raise ValueError(f"FrameShard: mode={mode!r} beside window={R}: the windowed pass has one exchange pattern of its "
                             "own (pass mode=None)")
        if int(n_edits) != 1 and not getattr(self, "window_edits", False):      # (opt-in: window_edits=True)
            raise ValueError("FrameShard: a sliding-window bank on a frame shard runs one edit (n_edits > 1 with window= is "
                             "not supported)")
        from . import _lib
        if self.Kl > _lib.TF_MAX_WINDOW_FRAMES:
            raise ValueError(f"FrameShard: {self.Kl} local keyframes (at most {_lib.TF_MAX_WINDOW_FRAMES} carry a window)")
        return R

    def _pivotal_window(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool, R: int, out4=None):
        """The windowed pass (module text of `window_halo_plan`): the same packing, exchange and two attention calls as the
        native executor's tf_rank_pivotal_window -- the same bits on the same transport, and the bits of ONE process issuing
        `ops.ext_attn_windows_views(part="bank")` with `ops.bank_windows(K, R)` plus the source-only call on the full tensors.
          1. ONE `ops.window_halo_pack` of the slabs PEERS read ([k1,k2,v1,v2]; under injection [k0,v1,v2]: the choice of
             `_bank_gather(peers_only=True)`) for the frames each peer's windows reach, own frames as self rows;
          2. ONE row all-to-all with the sparse counts: the receive buffer is the extended bank [F, slabs, S, D];
          3. the source part of the local frames, window-free, on the caller's own tensors;
          4. the bank part over the receive buffer in place, Kq = Kl, q_frame0 = hl, the local window table.
        No overlap here (through gloo the exchange is staged through the host anyway)."""
        B, S, D = q_local.shape
        Kl = self.Kl
        ns_ = not self.attn_split
        if self.world == 1:
            out = None if out4 is None else out4.view(q_local.shape)
            return ops.ext_attn_windows(q_local, k_local, v_local, heads, scale, inject, ops.bank_windows(self.K, R), out=out,
                                        no_split=ns_)
        plan = window_halo_plan(self.K, self.world, self.rank, R)
        dev, dt = q_local.device, q_local.dtype

        def frames(t):     # [3*Kl, S, D] (token stride free) -> [3, Kl, S, D] view
            if t.stride(2) != 1 or t.stride(0) != S * t.stride(1):
                t = t.contiguous()
            return t.view(3, Kl, S, D) if t.is_contiguous() else t.unflatten(0, (3, Kl))
        q3, k3, v3 = frames(q_local), frames(k_local), frames(v_local)
        if k3.stride(2) != v3.stride(2):
            k3, v3 = k3.contiguous(), v3.contiguous()
        slabs = [k3[0], v3[1], v3[2]] if inject else [k3[1], k3[2], v3[1], v3[2]]
        ns = len(slabs)
        send = ops.window_halo_pack(slabs, plan.send, out=self._buf("win_send", (sum(plan.send_rows), ns, S, D), dt, dev))
        recv = self._buf("win_recv", (plan.F, ns, S, D), dt, dev)
        self._a2a(recv.view(plan.F, -1), send.view(send.shape[0], -1), plan.recv_rows, plan.send_rows)
        out = torch.empty(3, Kl, S, D, dtype=dt, device=dev) if out4 is None else out4
        ops.ext_attn_views(q3, k3, v3, out, heads, scale, inject, "source", no_split=ns_)
        rp = recv.permute(1, 0, 2, 3)                                   # [ns, F, S, D] views: frame stride ns*S*D
        if inject:     # k holds the source slab alone (branch 0), v the two value banks (branches 1, 2)
            ops.ext_attn_windows_views(q3, rp[0:1], rp[1:3], out, heads, scale, True, plan.windows, "bank",
                                       branch0=(0, 0, 1, 0), q_frame0=plan.hl, no_split=ns_)
        else:
            ops.ext_attn_windows_views(q3, rp[0:2], rp[2:4], out, heads, scale, False, plan.windows, "bank",
                                       branch0=(0, 1, 1, 0), q_frame0=plan.hl, no_split=ns_)
        return out.view(3 * Kl, S, D) if out4 is None else out4

    # ------------------------------------------------------------------ ... plus global anchor keyframes
    supports_window_anchors = True      # `pivotal_attention` / `pivotal_block` take anchors= beside window=

    def _anchors(self, window, anchors) -> tuple:
        """The anchors of a pass as sorted distinct global indices (() = none), checked against the shard's WHOLE bank;
        `anchors` without `window` is an error."""
        if anchors is None:
            return ()
        if window is None:
            raise ValueError("FrameShard: anchors= without window= (anchor keyframes stand beside a sliding-window bank)")
        return tuple(_anchor_list("FrameShard", anchors, self.K))

    def _pivotal_frame_sets(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool, R: int, anchors, out4=None):
        """The anchored windowed pass (`frame_set_halo_plan`): `_pivotal_window` with a set instead of a range on both sides of
        the exchange -- the same packing, exchange and two attention calls as the native executor's tf_rank_pivotal_frame_sets:
          1. ONE `ops.frame_set_halo_pack` of the slabs peers read, per peer the members of its mask, own frames as self rows;
          2. ONE row all-to-all with the sparse counts: the receive buffer is the extended bank U [F, slabs, S, D];
          3. the source part of the local frames, set-free;
          4. `ops.ext_attn_frame_sets_views(part="bank")` over the receive buffer in place, Kq = Kl, q_frame0 and the sets of
             the plan (masks over U's positions: F <= 64 whatever K)."""
        B, S, D = q_local.shape
        Kl = self.Kl
        ns_ = not self.attn_split
        if self.world == 1:
            out = None if out4 is None else out4.view(q_local.shape)
            return ops.ext_attn_frame_sets(q_local, k_local, v_local, heads, scale, inject,
                                           ops.bank_frame_sets(self.K, R, anchors), out=out, no_split=ns_)
        plan = frame_set_halo_plan(self.K, self.world, self.rank, R, anchors)
        dev, dt = q_local.device, q_local.dtype

        def frames(t):     # [3*Kl, S, D] (token stride free) -> [3, Kl, S, D] view
            if t.stride(2) != 1 or t.stride(0) != S * t.stride(1):
                t = t.contiguous()
            return t.view(3, Kl, S, D) if t.is_contiguous() else t.unflatten(0, (3, Kl))
        q3, k3, v3 = frames(q_local), frames(k_local), frames(v_local)
        if k3.stride(2) != v3.stride(2):
            k3, v3 = k3.contiguous(), v3.contiguous()
        slabs = [k3[0], v3[1], v3[2]] if inject else [k3[1], k3[2], v3[1], v3[2]]
        ns = len(slabs)
        send = ops.frame_set_halo_pack(slabs, plan.send, out=self._buf("set_send", (sum(plan.send_rows), ns, S, D), dt, dev))
        recv = self._buf("set_recv", (plan.F, ns, S, D), dt, dev)
        self._a2a(recv.view(plan.F, -1), send.view(send.shape[0], -1), plan.recv_rows, plan.send_rows)
        out = torch.empty(3, Kl, S, D, dtype=dt, device=dev) if out4 is None else out4
        ops.ext_attn_views(q3, k3, v3, out, heads, scale, inject, "source", no_split=ns_)
        rp = recv.permute(1, 0, 2, 3)                                   # [ns, F, S, D] views: frame stride ns*S*D
        if inject:     # k holds the source slab alone (branch 0), v the two value banks (branches 1, 2)
            ops.ext_attn_frame_sets_views(q3, rp[0:1], rp[1:3], out, heads, scale, True, plan.sets, "bank",
                                          branch0=(0, 0, 1, 0), q_frame0=plan.q_frame0, no_split=ns_)
        else:
            ops.ext_attn_frame_sets_views(q3, rp[0:2], rp[2:4], out, heads, scale, False, plan.sets, "bank",
                                          branch0=(0, 1, 1, 0), q_frame0=plan.q_frame0, no_split=ns_)
        return out.view(3 * Kl, S, D) if out4 is None else out4

    # ------------------------------------------------------------------ ... for a multi-edit batch (the window_edits opt-in)
    supports_window_edits = True      # window= / anchors= beside n_edits > 1 (hooks.register_bank_window(edit_shard=True))

    def _window_edits_hints(self, dh: int) -> dict:
        """The four-bank keywords of the windowed multi-edit pass: off (bit-stable per edit) unless the shard opts in."""
        if not getattr(self, "window_edits_multi_v", False):
            return dict(multi_v=False)
        return dict(multi_v=True) if dh == 40 else dict(multi_v64=True) if dh == 64 else {}

    def _pivotal_window_edits(self, q_local, k_local, v_local, heads, scale, inject, R, anchors, out4, E, inject_mask):
        """`_pivotal_window` / `_pivotal_frame_sets` for E edits: the same pack, exchange and two part calls as the native
        executor's tf_rank_pivotal_frame_sets_edits, filling the same buffers with the same bits on the same transport:
          1. ONE `ops.edit_halo_pack` of the compact k slots and the 2E value slabs for the frames each peer reads (the source's
             v and every q stay at home); under a mixed mask the same launch stages the compact q slots;
          2. ONE row all-to-all with the sparse counts: the receive buffer is the extended bank [F, slabs, S, D];
          3. the source part of the local frames, table-free (`ops.ext_attn_edits_views(part="source")`);
          4. the bank part of ALL edits over the receive buffer in place: `ops.ext_attn_windows_edits_views` (no anchors) or
             `ops.ext_attn_frame_sets_edits_views`, compact q / k, Kq = Kl, q_frame0 and the table of the plan."""
        B = 1 + 2 * E
        if inject_mask is None:
            mask = (1 << E) - 1 if inject else 0
        else:
            mask = int(inject_mask)
            if inject or mask < 0 or mask >> E:
                raise ValueError(f"FrameShard.pivotal_attention: inject_mask {mask:#x} for {E} edits (bits below n_edits; "
                                 f"`inject` must be False beside a mask)")
        _, S, D = q_local.shape
        Kl = self.Kl
        ns_ = not self.attn_split
        mv = self._window_edits_hints(D // heads)
        if self.world == 1:
            out = None if out4 is None else out4.view(q_local.shape)
            if anchors:
                return ops.ext_attn_frame_sets_edits(q_local, k_local, v_local, heads, scale, False, E,
                                                     ops.bank_frame_sets(self.K, R, anchors), inject_mask=mask, out=out,
                                                     no_split=ns_, **mv)
            return ops.ext_attn_windows_edits(q_local, k_local, v_local, heads, scale, False, E, ops.bank_windows(self.K, R),
                                              inject_mask=mask, out=out, no_split=ns_, **mv)
        plan = frame_set_halo_plan(self.K, self.world, self.rank, R, anchors)      # (no anchors: the windowed plan)
        dev, dt = q_local.device, q_local.dtype

        def frames(t):     # [B*Kl, S, D] (token stride free) -> [B, Kl, S, D] view
            if t.stride(2) != 1 or t.stride(0) != S * t.stride(1):
                t = t.contiguous()
            return t.view(B, Kl, S, D) if t.is_contiguous() else t.unflatten(0, (B, Kl))
        q4, k4, v4 = frames(q_local), frames(k_local), frames(v_local)
        if k4.stride(2) != v4.stride(2):
            k4, v4 = k4.contiguous(), v4.contiguous()
        slots = ([0] if mask else []) + [b for e in range(E) if not (mask >> e) & 1 for b in (1 + 2 * e, 2 + 2 * e)]
        b0 = 0 if mask else 1
        nq = len(slots)
        mixed = bool(mask) and nq > 1
        slabs = [k4[b] for b in slots] + [v4[b] for b in range(1, B)]
        ns = len(slabs)
        # what each peer reads of this rank, as a mask over the local frames (a plain window's ranges are contiguous masks)
        masks = plan.send if anchors else [((1 << n) - 1) << f0 for f0, n in plan.send]
        send, qst = ops.edit_halo_pack(slabs, masks, [q4[b] for b in slots] if mixed else (),
                                       out=self._buf("wine_send", (sum(plan.send_rows), ns, S, D), dt, dev),
                                       q_out=self._buf("wine_q", (nq, Kl, S, D), dt, dev) if mixed else None)
        recv = self._buf("wine_recv", (plan.F, ns, S, D), dt, dev)
        self._a2a(recv.view(plan.F, -1), send.view(send.shape[0], -1), plan.recv_rows, plan.send_rows)
        out = torch.empty(B, Kl, S, D, dtype=dt, device=dev) if out4 is None else out4
        ops.ext_attn_edits_views(q4[0:1], k4[0:1], v4[0:1], out[0:1], heads, scale, E, mask, "source", no_split=ns_)
        rp = recv.permute(1, 0, 2, 3)                                   # [ns, F, S, D] views: frame stride ns*S*D
        qc = qst if mixed else q4[b0:]      # the dense tensor is the compact layout already unless the mask is mixed
        if anchors:
            ops.ext_attn_frame_sets_edits_views(qc, rp[0:nq], rp[nq:], out[1:], heads, scale, E, mask, plan.sets, "bank", True,
                                                branch0=(b0, b0, 1, 1), q_frame0=plan.q_frame0, no_split=ns_, **mv)
        else:
            ops.ext_attn_windows_edits_views(qc, rp[0:nq], rp[nq:], out[1:], heads, scale, E, mask, plan.windows, "bank", True,
                                             branch0=(b0, b0, 1, 1), q_frame0=plan.hl, no_split=ns_, **mv)
        return out.view(B * Kl, S, D) if out4 is None else out4

    # ------------------------------------------------------------------ pivotal pass of a multi-edit batch
    def _pivotal_edits(self, q_local, k_local, v_local, heads, scale, inject, mode, out4, E, inject_mask):
        B = 1 + 2 * E
        if inject_mask is None:
            mask = (1 << E) - 1 if inject else 0
        else:
            mask = int(inject_mask)
            if inject or mask < 0 or mask >> E:
                raise ValueError(f"FrameShard.pivotal_attention: inject_mask {mask:#x} for {E} edits (bits below n_edits; "
                                 f"`inject` must be False beside a mask)")
        if self.world == 1:
            out = None if out4 is None else out4.view(q_local.shape)
            return ops.ext_attn_edits(q_local, k_local, v_local, heads, scale, False, E, out=out,
                                      no_split=not self.attn_split, inject_mask=mask)
        if mode is None:
            mode = self.auto_mode(heads, q_local.shape[1], E)
        if mode == "bank_runs" and not getattr(self, "edit_runs", False):
            raise ValueError(_NO_EDIT_RUNS)
        _, S, D = q_local.shape
        Kl = self.Kl

        def frames(t):     # [B*Kl, S, D] (token stride free) -> [B, Kl, S, D] view
            if t.stride(2) != 1 or t.stride(0) != S * t.stride(1):
                t = t.contiguous()
            return t.view(B, Kl, S, D) if t.is_contiguous() else t.unflatten(0, (B, Kl))
        q4, k4, v4 = frames(q_local), frames(k_local), frames(v_local)
        if not (q4.stride(2) == k4.stride(2) == v4.stride(2)):
            q4, k4, v4 = (t.contiguous() for t in (q4, k4, v4))
        out = torch.empty(B, Kl, S, D, dtype=q4.dtype, device=q4.device) if out4 is None else out4
        # the compact q / k layout of tf_ext_attn_fwd_edits_part: the source slot where some edit injects, then the slots of
        # the edits that do not; b0 = the first slot that exists
        slots = ([0] if mask else []) + [b for e in range(E) if not (mask >> e) & 1 for b in (1 + 2 * e, 2 + 2 * e)]
        b0 = 0 if mask else 1
        if mode == "heads":
            self._pivotal_heads_edits(q4, k4, v4, out, heads, scale, E, mask, slots, b0)
        elif mode == "bank_runs":
            self._pivotal_bank_runs_edits(q4, k4, v4, out, heads, scale, E, mask, slots, b0)
        else:
            self._pivotal_bank_edits(q4, k4, v4, out, heads, scale, E, mask, slots, b0)
        return out.view(B * Kl, S, D) if out4 is None else out4

    def _pivotal_heads_edits(self, q4, k4, v4, out, heads, scale, E, mask, slots, b0):
        """`_pivotal_heads` for E edits: ONE pack of [q slots | k slots | v_1 .. v_2E] (2 * len(slots) + 2E slabs), ONE first
        all-to-all, the bank part of every edit on the receive buffer in place (`ops.ext_attn_edits_views`, compact q / k),
        ONE second all-to-all of [K][2E][S][hd], ONE unpack into the 2E bank slabs of `out`; the source branch of the
        rank's own frames beside the first exchange."""
        W, Kl, K = self.world, self.Kl, self.K
        B, _, S, D = q4.shape
        if heads % W:
            raise ValueError(f"{heads} heads do not divide over {W} ranks")
        hd, dev, dt = D // W, q4.device, q4.dtype
        even, ns_ = self.even, not self.attn_split
        nq = len(slots)
        slabs = [q4[b] for b in slots] + [k4[b] for b in slots] + [v4[b] for b in range(1, B)]
        ns = len(slabs)
        send = ops.head_pack(slabs, W, out=self._buf("send", (W, Kl, ns, S, hd), dt, dev))
        recv = self._buf("recv", (K, ns, S, hd), dt, dev)
        work = self._a2a(recv.view(K, -1), send.view(W * Kl, -1),
                         None if even else self.counts, None if even else [Kl] * W, async_op=True)
        src_done = None
        if q4.is_cuda and getattr(self, "src_aux", False):
            src_done = self._on_aux(dev, [q4, k4, v4, out], lambda st: ops.ext_attn_edits_views(
                q4[0:1], k4[0:1], v4[0:1], out[0:1], heads, scale, E, mask, "source", no_split=ns_, stream=st))
        else:
            ops.ext_attn_edits_views(q4[0:1], k4[0:1], v4[0:1], out[0:1], heads, scale, E, mask, "source", no_split=ns_)
        work.wait()
        rp = recv.permute(1, 0, 2, 3)                                   # [ns, K, S, hd] view
        send2 = self._buf("send2", (K, B - 1, S, hd), dt, dev)        # [frame][uncond_1|cond_1|...]: rows of rank w's run -> w
        o4 = send2.permute(1, 0, 2, 3)                                  # [2E, K, S, hd] view = branches 1 ..
        ops.ext_attn_edits_views(rp[0:nq], rp[nq:2 * nq], rp[2 * nq:], o4, heads // W, scale, E, mask, "bank", True,
                                 branch0=(b0, b0, 1, 1), no_split=ns_)
        recv2 = self._buf("recv2", (W, Kl, B - 1, S, hd), dt, dev)
        self._a2a(recv2.view(W * Kl, -1), send2.view(K, -1),
                  None if even else [Kl] * W, None if even else self.counts)
        ops.head_unpack(recv2, [out[b] for b in range(1, B)])
        if src_done is not None:
            src_done.wait()

    def _pivotal_bank_edits(self, q4, k4, v4, out, heads, scale, E, mask, slots, b0):
        """`_pivotal_bank` for E edits: ONE gather of exactly the compact k slots and the 2E value slabs (the source branch's
        v and every q stay at home), the bank part on the gathered buffer in place, the source part on the local tensors."""
        Kl, K = self.Kl, self.K
        B, _, S, D = q4.shape
        nq, ns_ = len(slots), not self.attn_split
        rp = self._gather_slabs([k4[b] for b in slots] + [v4[b] for b in range(1, B)], "bank_e")
        # q in the same compact layout: the dense tensor is that layout already unless the mask is mixed
        qc = q4[b0:] if len(slots) in (1, B - 1) else q4[slots]
        ops.ext_attn_edits_views(qc, rp[0:nq], rp[nq:], out[1:], heads, scale, E, mask, "bank", True,
                                 branch0=(b0, b0, 1, 1), q_frame0=self.kf0, no_split=ns_)
        ops.ext_attn_edits_views(q4[0:1], k4[0:1], v4[0:1], out[0:1], heads, scale, E, mask, "source", no_split=ns_)

    def _pivotal_bank_runs_edits(self, q4, k4, v4, out, heads, scale, E, mask, slots, b0):
        """`_pivotal_bank_runs` for E edits (the `edit_runs` opt-in): ONE gather of exactly what `_pivotal_bank_edits` gathers
        -- the compact k slots and the 2E value slabs -- then the runs of `bank_runs_of_rank()` in slot order local, left,
        right: the local run reads the caller's tensors in place (dense q, k, v; it also computes the source branch), the
        remote runs the receive buffer in place (k compact) against the same dense q; then the ONE merge over all 2E bank
        branches.  No overlap here, as in `_pivotal_bank_runs`.  Per edit the bits of that form on [source | uncond_e |
        cond_e]; the same bits as the native executor's TF_RANK_BANK_EDIT_RUNS on the same transport."""
        B = q4.shape[0]
        nq = len(slots)
        rp = self._gather_slabs([k4[b] for b in slots] + [v4[b] for b in range(1, B)], "bank_e")
        runs = self.bank_runs_of_rank()
        kv_runs = [(k4, v4, 0, 0, False)]
        for f0, n in runs[1:]:
            kv_runs.append((rp[0:nq, f0:f0 + n], rp[nq:, f0:f0 + n], b0, 1, True))
        # (the keyword only with the opt-in: without it the call is the one it was)
        mv = dict(multi_v=True) if getattr(self, "edit_runs_multi_v", False) else {}
        ops.ext_attn_runs_edits_views(q4, kv_runs, out, heads, scale, E, mask, runs, self.K, q_frame0=self.kf0,
                                      no_split=not self.attn_split, **mv)

    def bank_runs_of_rank(self):
        """The runs of the bank this rank computes in the "bank_runs" form, in SLOT order: its own keyframes, the frames
        to their left, the frames to their right (empty ones dropped).  The order fixes the merge's arithmetic."""
        runs = [(self.kf0, self.Kl)]
        if self.kf0 > 0:
            runs.append((0, self.kf0))
        if self.kf0 + self.Kl < self.K:
            runs.append((self.kf0 + self.Kl, self.K - self.kf0 - self.Kl))
        return runs

    def _pivotal_bank_runs(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool, out4=None):
        """The bank form in runs (module text): the same packing, runs and slot order as the native executor's
        TF_RANK_BANK_RUNS -- the same bits on the same transport.  The schedule here does not overlap (the gather is
        waited for before the first run is issued; through gloo it is staged through the host anyway)."""
        B, S, D = q_local.shape
        Kl = self.Kl
        kr, vr, k3, v3 = self._bank_gather(k_local, v_local, inject, peers_only=True)
        q = q_local
        if q.stride(2) != 1 or q.stride(0) != S * q.stride(1):
            q = q.contiguous()
        q4 = q.view(3, Kl, S, D) if q.is_contiguous() else q.unflatten(0, (3, Kl))
        out = torch.empty(3, Kl, S, D, dtype=q.dtype, device=q.device) if out4 is None else out4
        runs = self.bank_runs_of_rank()
        kv_runs = [(k3, v3, 0, 0)]          # the local run: the caller's own projections, in place
        for f0, n in runs[1:]:              # remote runs: the receive buffer in place; k holds branch 0 alone under injection
            kv_runs.append((kr[:, f0:f0 + n], vr[:, f0:f0 + n], 0 if inject else 1, 1))
        ops.ext_attn_runs_views(q4, kv_runs, out, heads, scale, inject, runs, self.K, q_frame0=self.kf0,
                                no_split=not self.attn_split)
        return out.view(3 * Kl, S, D) if out4 is None else out4

    def _pivotal_bank(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool, out4=None):
        """One gather (`_bank_gather`), one attention call on the gathered buffer in place; q keeps its own layout
        (its token stride is independent of the bank's)."""
        B, S, D = q_local.shape
        Kl = self.Kl
        kv, vv = self._bank_gather(k_local, v_local, inject)
        q = q_local
        if q.stride(2) != 1 or q.stride(0) != S * q.stride(1):
            q = q.contiguous()
        q4 = q.view(3, Kl, S, D) if q.is_contiguous() else q.unflatten(0, (3, Kl))
        out = torch.empty(3, Kl, S, D, dtype=q.dtype, device=q.device) if out4 is None else out4
        ops.ext_attn_views(q4, kv, vv, out, heads, scale, inject, "all", q_frame0=self.kf0,
                           no_split=not self.attn_split)
        return out.view(3 * Kl, S, D) if out4 is None else out4

    def _pivotal_heads(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool, out4=None):
        """Frames <-> heads re-sharding.  Launches per block on this rank: ONE pack kernel, the source-branch
        attention (overlaps the first all-to-all), the bank attention reading the received buffer IN PLACE and
        writing the second all-to-all's send buffer IN PLACE (strided views, no re-layout copies), ONE unpack
        kernel.  Buffers are laid out for the collectives: what a rank sends to peer w is one contiguous
        [Kl, slabs, S, D/W] piece, so what arrives is [K (global frame order), slabs, S, D/W] whatever the run
        lengths."""
        W, Kl, K = self.world, self.Kl, self.K
        B, S, D = q_local.shape
        if heads % W:
            raise ValueError(f"{heads} heads do not divide over {W} ranks")
        hd, dev, dt = D // W, q_local.device, q_local.dtype
        src_done = None

        def frames(t):     # [3*Kl, S, D] (token stride free) -> [3, Kl, S, D] view
            if t.stride(2) != 1 or t.stride(0) != S * t.stride(1):
                t = t.contiguous()
            return t.view(3, Kl, S, D) if t.is_contiguous() else t.unflatten(0, (3, Kl))
        q3, k3, v3 = frames(q_local), frames(k_local), frames(v_local)
        if not (q3.stride(2) == k3.stride(2) == v3.stride(2)):      # one token stride for the pack kernel
            q3, k3, v3 = (t.contiguous() for t in (q3, k3, v3))
        even = self.even
        # ---- pack: head group w of every slab the bank branches read, frame-major, slab order [q.., k.., v..]
        if inject:       # source q, k (what uncond and cond use, 124-130) and the two value banks
            slabs = [q3[0], k3[0], v3[1], v3[2]]
        else:
            slabs = [q3[1], q3[2], k3[1], k3[2], v3[1], v3[2]]
        ns = len(slabs)
        send = ops.head_pack(slabs, W, out=self._buf("send", (W, Kl, ns, S, hd), dt, dev))
        recv = self._buf("recv", (K, ns, S, hd), dt, dev)
        work = self._a2a(recv.view(K, -1), send.view(W * Kl, -1),
                         None if even else self.counts, None if even else [Kl] * W, async_op=True)
        # ---- source branch: own-frame keys, all heads, stays local (overlaps the exchange)
        if out4 is None:
            out = torch.empty(3, Kl, S, D, dtype=dt, device=dev)
            ops.ext_attn(q_local, k_local, v_local, heads, scale, inject, out=out.view(3 * Kl, S, D), part="source",
                         no_split=not self.attn_split)
        else:            # straight into the caller's (strided) slots: the strided entry point
            out = out4
            if q3.is_cuda and getattr(self, "src_aux", False):
                # on its own stream: the source problems of a rank are a fraction of a chip-filling grid (one frame's
                # queries: 32..128 workgroups), so they run BESIDE the exchange and the bank attention that follows it,
                # not in front of it; joined before the block's results leave (below)
                src_done = self._on_aux(dev, [q3, k3, v3, out], lambda st: ops.ext_attn_views(
                    q3, k3, v3, out, heads, scale, inject, "source", no_split=not self.attn_split, stream=st))
            else:
                ops.ext_attn_views(q3, k3, v3, out, heads, scale, inject, "source", no_split=not self.attn_split)
        work.wait()
        # ---- bank branches on this rank's head group, all K frames: read `recv`, write `send2`, both in place
        rp = recv.permute(1, 0, 2, 3)                                   # [ns, K, S, hd] view
        send2 = self._buf("send2", (K, 2, S, hd), dt, dev)            # [frame][uncond|cond]: rows of rank w's run -> w
        o4 = send2.permute(1, 0, 2, 3)                                  # [2, K, S, hd] view = branches 1, 2
        if inject:
            ops.ext_attn_views(rp[0:1], rp[1:2], rp[2:4], o4, heads // W, scale, True, "bank", branch0=(0, 0, 1, 1),
                               no_split=not self.attn_split)
        else:
            ops.ext_attn_views(rp[0:2], rp[2:4], rp[4:6], o4, heads // W, scale, False, "bank", branch0=(1, 1, 1, 1),
                               no_split=not self.attn_split)
        # ---- outputs back to the frame owners
        recv2 = self._buf("recv2", (W, Kl, 2, S, hd), dt, dev)        # [head group][my frames][uncond|cond]
        self._a2a(recv2.view(W * Kl, -1), send2.view(K, -1),
                  None if even else [Kl] * W, None if even else self.counts)
        ops.head_unpack(recv2, [out[1], out[2]])
        if src_done is not None:
            src_done.wait()
        return out.view(3 * Kl, S, D) if out4 is None else out4

    # ------------------------------------------------------------------ pivotal pass of one block, in place
    def ext_alloc(self, S: int, D: int, dtype: torch.dtype, device, n_edits: int = 1):
        """Per-block state of the propagation, halo slot included: (pivots [Kl+o,S,D], inverse norms [Kl+o,S] fp32,
        cached attention output [3,Kl+o,S,D]) with o = 1 when there is a left neighbour to hear from (world > 1), else
        0.  The producers write the local keyframes straight into slots o.. (norm1 -> pivots and inverse norms, the
        attention -> its output): no staging copy on either side of the halo exchange.  n_edits = E: the cached attention
        output holds all 1 + 2E branches, [1+2E,Kl+o,S,D]."""
        o = 1 if self.world > 1 else 0
        Kl = self.Kl
        return (torch.empty(Kl + o, S, D, dtype=dtype, device=device),
                torch.empty(Kl + o, S, dtype=torch.float32, device=device),
                torch.empty(1 + 2 * int(n_edits), Kl + o, S, D, dtype=dtype, device=device))

    def pivotal_block(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool, ext,
                      mode: Optional[str] = None, inv_norm: bool = False, n_edits: int = 1,
                      inject_mask: Optional[int] = None, window: Optional[int] = None, anchors=None):
        """n_edits / inject_mask / window / anchors: as `pivotal_attention`; `ext` from `ext_alloc(..., n_edits=)`; the ONE grouped exchange
        carries the last keyframe of all 1 + 2E branches of the attention output.
        The pivotal pass of one block on this rank, for the reference's call order (one pivotal pass over all
        blocks, then the chunk passes): `ext` = `ext_alloc(...)` whose pivot / inverse-norm slots o.. the caller has
        filled.  The attention writes its output into ext's slots o.. in place, then ONE grouped neighbour exchange
        carries the last local keyframe's pivots, inverse norms and attention output to slot 0 of rank r+1 (it has the
        rest of the pivotal pass to arrive; nothing waits for it before the propagation).
        inv_norm=True: the inverse-norm slots o.. are filled HERE from the pivot slots (callers whose norm1 is not the
        fused LayerNorm producer; the native executor does it inside its pack launch).
        Returns (pivots ext, inverse norms ext, attention output ext [3(Kl+o),S,D], pending requests) -- the
        arguments of `propagate_all(..., halo_reqs=)`."""
        piv, inv, kfo = ext
        o = 1 if self.world > 1 else 0
        Kl = self.Kl
        S, D = piv.shape[1:]
        if inv_norm:
            ops.pivot_inv_norm(piv[o:], out=inv[o:])
        nbr = 1 + 2 * int(n_edits)
        anc = self._anchors(window, anchors)
        if self._window(window, n_edits, mode) is not None:
            self.pivotal_attention(q_local, k_local, v_local, heads, scale, inject, out4=kfo[:, o:], window=window,
                                   anchors=anc or None, **(dict(n_edits=n_edits, inject_mask=inject_mask) if n_edits != 1 else {}))
        elif n_edits == 1:
            self.pivotal_attention(q_local, k_local, v_local, heads, scale, inject, mode=mode, out4=kfo[:, o:])
        else:
            self.pivotal_attention(q_local, k_local, v_local, heads, scale, inject, mode=mode, out4=kfo[:, o:],
                                   n_edits=n_edits, inject_mask=inject_mask)
        reqs = []
        if self.world > 1:
            reqs = self._p2p([piv[-1], inv[-1]] + [kfo[b, -1] for b in range(nbr)],
                             [piv[0], inv[0]] + [kfo[b, 0] for b in range(nbr)])
        return piv, inv, kfo.view(nbr * (Kl + o), S, D), reqs

    def halo_block(self, piv_ext: torch.Tensor, inv_ext: torch.Tensor, kfo_ext: torch.Tensor, n_edits: int = 1):
        """ONE grouped neighbour exchange on halo-extended per-block state the producers have written in place
        (`ext_alloc` layout: slot 0 = the left neighbour's last keyframe): the last local keyframe's pivots, inverse
        norms and attention output go to rank r+1, the neighbour's arrive in slot 0.  Returns the pending requests
        (`halo_wait`).  What `pivotal_block` issues behind its attention; the hook path calls it behind `to_out`."""
        if self.world == 1:
            return []
        nbr = 1 + 2 * int(n_edits)       # kfo_ext [1+2E, Kl+1, S, D]: the last keyframe of every branch in the same exchange
        return self._p2p([piv_ext[-1], inv_ext[-1]] + [kfo_ext[b, -1] for b in range(nbr)],
                         [piv_ext[0], inv_ext[0]] + [kfo_ext[b, 0] for b in range(nbr)])

    # ------------------------------------------------------------------ halo for propagation
    def exchange_halo(self, pivots_local: torch.Tensor, inv_local: torch.Tensor, kf_out_local: torch.Tensor,
                      n_edits: int = 1):
        """pivots_local [Kl,S,D], inv_local [Kl,S], kf_out_local [3*Kl,S,D] (this rank's keyframes).
        Returns the same three with ONE extra leading keyframe slot = the previous rank's last
        keyframe (unset and unread on rank 0: global chunk 0 matches a single keyframe, 331-333)."""
        h = self.halo_start(pivots_local, inv_local)
        return self.halo_finish(h, kf_out_local, n_edits=n_edits)

    def halo_start(self, pivots_local: torch.Tensor, inv_local: torch.Tensor, n_edits: int = 1):
        """First half of the halo exchange: the pivot features and inverse norms of the last local keyframe go to
        rank r+1.  They exist as soon as norm1 has run, BEFORE the attention, so this is issued first and travels
        under the attention; `halo_finish` then sends the attention output."""
        if self.world == 1:
            return (pivots_local, inv_local, None)
        Kl = self.Kl
        _, S, D = pivots_local.shape
        # slot 0 = the left neighbour's last keyframe; on rank 0 it stays unset and is never read
        piv = torch.empty(Kl + 1, S, D, dtype=pivots_local.dtype, device=pivots_local.device)
        inv = torch.empty(Kl + 1, S, dtype=inv_local.dtype, device=inv_local.device)
        piv[1:].copy_(pivots_local)
        inv[1:].copy_(inv_local)
        reqs = self._p2p([pivots_local[-1], inv_local[-1]], [piv[0], inv[0]])
        return (piv, inv, reqs)

    def halo_finish(self, handle, kf_out_local: torch.Tensor, wait: bool = True, n_edits: int = 1):
        """Second half: the attention output of the last local keyframe to rank r+1.  wait=False returns the
        pending requests as a 4th element (call `halo_wait`): the propagation of the local chunks 1.. does not read
        the halo slot and can be issued before."""
        piv, inv, reqs = handle
        if self.world == 1:
            return (piv, inv, kf_out_local) if wait else (piv, inv, kf_out_local, [])
        Kl = self.Kl
        S, D = kf_out_local.shape[1:]
        nbr = 1 + 2 * int(n_edits)       # kf_out_local [(1+2E)*Kl, S, D]
        kf3 = kf_out_local.view(nbr, Kl, S, D)
        kfo = torch.empty(nbr, Kl + 1, S, D, dtype=kf_out_local.dtype, device=kf_out_local.device)
        kfo[:, 1:].copy_(kf3)
        # no staging copies: every message is a contiguous view (the attention output travels as one message per branch)
        reqs = list(reqs) + self._p2p([kf3[b, -1] for b in range(nbr)], [kfo[b, 0] for b in range(nbr)])
        res = (piv, inv, kfo.view(nbr * (Kl + 1), S, D))
        if not wait:
            return res + (reqs,)
        self.halo_wait(reqs)
        return res

    @staticmethod
    def halo_wait(reqs):
        for r in reqs:
            r.wait()

    def _p2p(self, send_tensors, recv_tensors):
        """One grouped point-to-point exchange: `send_tensors` to rank r+1, `recv_tensors` from rank r-1."""
        comm = getattr(self, "halo_comm", None) or getattr(self, "comm", None)
        if comm is not None:
            to = self.rank + 1 if self.rank + 1 < self.world else -1
            frm = self.rank - 1 if self.rank > 0 else -1
            if to < 0 and frm < 0:
                return []
            send_tensors = [t.contiguous() for t in send_tensors]

            def go(st):     # one grouped call per element type (the C entry point takes one dtype per call)
                for dt in dict.fromkeys(t.dtype for t in list(send_tensors) + list(recv_tensors)):
                    comm.sendrecv([t for t in send_tensors if t.dtype == dt], to,
                                  [t for t in recv_tensors if t.dtype == dt], frm, stream=st)
            return [self._side(list(send_tensors) + list(recv_tensors), go, halo=True)]
        opsl = []
        grp = getattr(self, "halo_group", None) or self.group
        if self.rank + 1 < self.world:
            peer = self._peer(self.rank + 1)
            opsl += [dist.P2POp(dist.isend, t, peer, grp) for t in send_tensors]
        if self.rank > 0:
            peer = self._peer(self.rank - 1)
            opsl += [dist.P2POp(dist.irecv, t, peer, grp) for t in recv_tensors]
        return dist.batch_isend_irecv(opsl) if opsl else []

    def _peer(self, group_rank: int) -> int:
        return dist.get_global_rank(self.group, group_rank) if self.group is not None else group_rank

    # ------------------------------------------------------------------ propagation pass
    def propagate(self, j: int, tgt: torch.Tensor, residual: torch.Tensor, piv_ext, inv_ext, kf_out_ext,
                  w: torch.Tensor, n: int, out_dtype_two: torch.dtype = torch.float32, n_edits: int = 1):
        """Local chunk j (global chunk kf0 + j): NN search + gather/blend/residual.
        tgt [n*S, D] 16-bit source-branch features, residual [3n,S,D] ([(1+2E)n,S,D] with n_edits = E: one search, one
        gather over all branches)."""
        c = self.kf0 + j
        o = 1 if self.world > 1 else 0                   # halo slot offset
        ids = [j + o] if c == 0 else [j + o, j + o - 1]  # slots of keyframes [c, c-1] (tokenflow_utils.py:331-333)
        blend_dtype = out_dtype_two if len(ids) == 2 else kf_out_ext.dtype
        out_dtype = torch.promote_types(blend_dtype, residual.dtype) if residual is not None else blend_dtype
        if n_edits != 1:
            return ops.propagate_chunks_edits(tgt, piv_ext, inv_ext, kf_out_ext, w if len(ids) == 2 else None, n, 1, j + o,
                                              c == 0, residual, out_dtype, n_edits)
        return ops.propagate(tgt, piv_ext, inv_ext, ids, kf_out_ext, w if len(ids) == 2 else None, n, residual,
                             out_dtype)

    def propagate_all(self, tgt_all: torch.Tensor, residual_all: torch.Tensor, piv_ext, inv_ext, kf_out_ext,
                      w: torch.Tensor, n: int, out_dtype: torch.dtype = torch.float32, halo_reqs=None, n_edits: int = 1):
        """ALL local chunks (tf_nn_gather_blend_chunks): tgt_all [Kl*n*S, D] chunk-major, residual_all
        [3*Kl*n, S, D] (frames chunk-major inside each branch).  Same results as Kl calls of `propagate`, bit for
        bit; the one-keyframe chunk 0 of the video (rank 0) is rounded to the dtype its own call would produce.
        halo_reqs (from `halo_finish(wait=False)`): the local chunks 1.. read no halo slot and are issued FIRST,
        the first local chunk after the halo has landed; returns (first chunk [3n,S,D], rest [3(Kl-1)n,S,D] or None)."""
        o = 1 if self.world > 1 else 0
        if n_edits != 1:     # [(1+2E)*Kl*n, S, D] residual and result; one search and one gather over all branches per call
            E, nbr = int(n_edits), 1 + 2 * int(n_edits)
            if halo_reqs is None:
                return ops.propagate_chunks_edits(tgt_all, piv_ext, inv_ext, kf_out_ext, w, n, self.Kl, o, self.kf0 == 0,
                                                  residual_all, out_dtype, E)
            Kl, S, D = self.Kl, piv_ext.shape[1], piv_ext.shape[2]
            nS = n * S
            res = residual_all.view(nbr, Kl, n, S, D)
            rest = None
            if Kl > 1:
                rest = ops.propagate_chunks_edits(tgt_all[nS:], piv_ext, inv_ext, kf_out_ext, w, n, Kl - 1, o + 1, False,
                                                  res[:, 1:].reshape(nbr * (Kl - 1) * n, S, D), out_dtype, E)
            self.halo_wait(halo_reqs)
            first = self.propagate(0, tgt_all[:nS], res[:, 0].reshape(nbr * n, S, D), piv_ext, inv_ext, kf_out_ext, w, n,
                                   n_edits=E)
            return first, rest
        if halo_reqs is None:
            return ops.propagate_chunks(tgt_all, piv_ext, inv_ext, kf_out_ext, w, n, self.Kl, o, self.kf0 == 0,
                                        residual_all, out_dtype)
        Kl, S, D = self.Kl, piv_ext.shape[1], piv_ext.shape[2]
        nS = n * S
        res = residual_all.view(3, Kl, n, S, D)
        rest = None
        if Kl > 1:
            rest = ops.propagate_chunks(tgt_all[nS:], piv_ext, inv_ext, kf_out_ext, w, n, Kl - 1, o + 1, False,
                                        res[:, 1:].reshape(3 * (Kl - 1) * n, S, D), out_dtype)
        self.halo_wait(halo_reqs)
        first = self.propagate(0, tgt_all[:nS], res[:, 0].reshape(3 * n, S, D), piv_ext, inv_ext, kf_out_ext, w, n)
        return first, rest


class _SlotWait:
    """Pending neighbour halo of one block of a `NativeShard`: wait() orders the CURRENT stream behind it."""

    def __init__(self, shard, slot, device):
        self.shard, self.slot, self.device = shard, slot, device

    def wait(self):
        from . import _lib
        rc = _lib.load().tf_rank_halo_wait(self.shard._rk, self.slot, torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            _lib.check(rc, "tf_rank_halo_wait")
        return True


class NativeShard(FrameShard):
    """`FrameShard` whose pivotal pass of a block is ONE call into the library (tf_rank_pivotal, csrc/rank_exec.hip):
    pack, exchanges, source and bank attention, unpack and the neighbour halo are issued by native code on the
    library's own streams -- the host cost of a block drops from a dozen Python-level op calls (200-300 us at a rank of
    8, more than the GPU needs for the block at the coarse levels) to one foreign call.  Same results as `FrameShard`
    bit for bit (same kernels, same buffers' layouts).  `comm` / `halo_comm`: `tokenflow_amd.comm.HipComm` objects (RCCL
    through the C ABI; a second communicator lets the halo of one block travel beside the exchanges of the next).
    Only the in-place two-pass API (`ext_alloc`, `pivotal_block`, `propagate_all(..., halo_reqs=)`) goes native; the
    other methods are `FrameShard`'s own on the same communicator.  tf_rank_pivotal runs one edit: no multi-edit batches."""

    supports_edits = False
    supports_window_edits = False      # tf_rank_pivotal_window / _frame_sets run one edit; `NativeEditShard` has the multi-edit call

    def __init__(self, K: int, comm, halo_comm=None, attn_split: Optional[bool] = None, bank_runs: Optional[bool] = None,
                 edit_runs: Optional[bool] = None, edit_runs_multi_v: Optional[bool] = None,
                 window_edits: Optional[bool] = None, window_edits_multi_v: Optional[bool] = None):
        super().__init__(K, comm=comm, attn_split=attn_split, halo_comm=halo_comm, bank_runs=bank_runs, edit_runs=edit_runs,
                         edit_runs_multi_v=edit_runs_multi_v, window_edits=window_edits,
                         window_edits_multi_v=window_edits_multi_v)
        from . import _lib
        lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(lib.tf_rank_create(comm._h if comm is not None else None,
                                      halo_comm._h if halo_comm is not None else None, K, ctypes.byref(h)),
                   "tf_rank_create")
        self._rk, self._halo_comm = h, halo_comm
        assert lib.tf_rank_local_keyframes(h) == self.Kl and lib.tf_rank_first_keyframe(h) == self.kf0
        self._slot = 0
        self._nws = {}

    def close(self):
        rk, self._rk = getattr(self, "_rk", None), None
        if rk is not None:
            from . import _lib
            _lib.load().tf_rank_destroy(rk)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    def pivotal_attention(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool,
                          mode: Optional[str] = None, out4: Optional[torch.Tensor] = None, window: Optional[int] = None,
                          anchors=None):
        """`FrameShard.pivotal_attention` as one library call (tf_rank_pivotal with TF_RANK_NO_HALO): what the hook path
        calls from `attn1` (its cached attention output is the to_out-projected one, so the halo stays the block's).
        window = R: the windowed pass, ONE tf_rank_pivotal_window call; with anchors ONE tf_rank_pivotal_frame_sets call."""
        anc = self._anchors(window, anchors)
        R = self._window(window, 1, mode)
        if self.world == 1 or out4 is not None or not q_local.is_cuda or q_local.dtype not in (torch.bfloat16,
                                                                                                torch.float16):
            if R is not None:
                return FrameShard.pivotal_attention(self, q_local, k_local, v_local, heads, scale, inject, out4=out4, window=R,
                                                    anchors=anc or None)
            return super().pivotal_attention(q_local, k_local, v_local, heads, scale, inject, mode=mode, out4=out4)
        B, S, D = q_local.shape
        out = torch.empty(3, self.Kl, S, D, dtype=q_local.dtype, device=q_local.device)
        self._native(q_local, k_local, v_local, heads, scale, inject, mode, None, None, out, no_halo=True, window=R,
                     anchors=anc if R is not None else ())
        return out.view(B, S, D)

    def pivotal_block(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool, ext,
                      mode: Optional[str] = None, inv_norm: bool = False, window: Optional[int] = None, anchors=None):
        piv, inv, kfo = ext
        B, S, D = q_local.shape
        Kl = self.Kl
        o = 1 if self.world > 1 else 0
        anc = self._anchors(window, anchors)
        R = self._window(window, 1, mode)
        slot = self._native(q_local, k_local, v_local, heads, scale, inject, mode, piv, inv, kfo, no_halo=False,
                            inv_norm=inv_norm, window=R, anchors=anc if R is not None else ())
        reqs = [_SlotWait(self, slot, q_local.device)] if self.world > 1 else []
        return piv, inv, kfo.view(3 * (Kl + o), S, D), reqs

    def _native(self, q_local, k_local, v_local, heads, scale, inject, mode, piv, inv, kfo, no_halo, inv_norm=False,
                window=None, anchors=()):
        from . import _lib
        lib = _lib.load()
        B, S, D = q_local.shape
        Kl = self.Kl
        if mode is None:
            mode = self.auto_mode(heads, S)
        dt = ops._DT.get(q_local.dtype)
        if dt is None or dt == _lib.TF_F32 or not (q_local.is_cuda and kfo.is_contiguous()
                                                    and (no_halo or (piv.is_contiguous() and inv.is_contiguous()))):
            raise TypeError("NativeShard: 16-bit GPU tensors, contiguous (halo-extended) buffers")

        def frames(t):     # [3*Kl, S, D] (token stride free) -> [3, Kl, S, D] view
            if t.stride(2) != 1 or t.stride(0) != S * t.stride(1):
                t = t.contiguous()
            return t.view(3, Kl, S, D) if t.is_contiguous() else t.unflatten(0, (3, Kl))
        q3, k3, v3 = frames(q_local), frames(k_local), frames(v_local)
        if k3.stride(2) != v3.stride(2) or (mode == "heads" and q3.stride(2) != k3.stride(2)):
            q3, k3, v3 = (t.contiguous() for t in (q3, k3, v3))
        strides = (ctypes.c_int64 * 8)(q3.stride(0), q3.stride(1), k3.stride(0), k3.stride(1), v3.stride(0), v3.stride(1),
                                       q3.stride(2), k3.stride(2))
        dh = D // heads
        anchors = tuple(anchors)
        anc = (ctypes.c_int * max(len(anchors), 1))(*anchors)
        key = (S, heads, dh, dt, q_local.device, window) + ((anchors,) if anchors else ())
        ws = self._nws.get(key)
        if ws is None:
            if window is None:
                nbytes = lib.tf_rank_pivotal_workspace_bytes(self._rk, S, heads, dh, dt)
            elif anchors:
                plan = frame_set_halo_plan(self.K, self.world, self.rank, int(window), anchors)      # (raises what is refused)
                nbytes = lib.tf_rank_pivotal_frame_sets_workspace_bytes(self._rk, S, heads, dh, dt, int(window),
                                                                        ctypes.cast(anc, ctypes.c_void_p), len(anchors))
                assert nbytes > 0, plan
            else:
                nbytes = lib.tf_rank_pivotal_window_workspace_bytes(self._rk, S, heads, dh, dt, int(window))
            ws = self._nws[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=q_local.device)
        flags = (_lib.TF_ATTN_INJECT if inject else 0) | (0 if self.attn_split else _lib.TF_ATTN_NO_SPLIT)
        if ops.FOLD_SCALE and window is None:      # (a windowed call has no folded-scale form: `ops.ext_attn_windows`)
            flags |= _lib.TF_ATTN_FOLD_SCALE
        slot = self._slot
        if not no_halo:
            self._slot = (slot + 1) % _lib.TF_RANK_SLOTS
        if window is not None and anchors:      # the anchored windowed pass: ONE tf_rank_pivotal_frame_sets call
            m = _lib.TF_RANK_BANK | (_lib.TF_RANK_NO_HALO if no_halo else 0) | (_lib.TF_RANK_INV_NORM if inv_norm else 0)
            rc = lib.tf_rank_pivotal_frame_sets(self._rk, q3.data_ptr(), k3.data_ptr(), v3.data_ptr(), strides,
                                                None if piv is None else piv.data_ptr(),
                                                None if inv is None else inv.data_ptr(), kfo.data_ptr(), S, heads, dh,
                                                float(scale), flags, dt, m, slot, int(window),
                                                ctypes.cast(anc, ctypes.c_void_p), len(anchors), ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream(q_local.device).cuda_stream)
            if rc:
                _lib.check(rc, "tf_rank_pivotal_frame_sets")
            return slot
        if window is not None:      # the windowed pass: ONE tf_rank_pivotal_window call
            m = _lib.TF_RANK_BANK | (_lib.TF_RANK_NO_HALO if no_halo else 0) | (_lib.TF_RANK_INV_NORM if inv_norm else 0)
            rc = lib.tf_rank_pivotal_window(self._rk, q3.data_ptr(), k3.data_ptr(), v3.data_ptr(), strides,
                                            None if piv is None else piv.data_ptr(), None if inv is None else inv.data_ptr(),
                                            kfo.data_ptr(), S, heads, dh, float(scale), flags, dt, m, slot, int(window),
                                            ws.data_ptr(), ws.numel(), torch.cuda.current_stream(q_local.device).cuda_stream)
            if rc:
                _lib.check(rc, "tf_rank_pivotal_window")
            return slot
        m = ({"heads": _lib.TF_RANK_HEADS, "bank_runs": _lib.TF_RANK_BANK_RUNS}.get(mode, _lib.TF_RANK_BANK)
             | (_lib.TF_RANK_NO_HALO if no_halo else 0)
             | (_lib.TF_RANK_INV_NORM if inv_norm else 0))
        rc = lib.tf_rank_pivotal(self._rk, q3.data_ptr(), k3.data_ptr(), v3.data_ptr(), strides,
                                 None if piv is None else piv.data_ptr(), None if inv is None else inv.data_ptr(),
                                 kfo.data_ptr(), S, heads, dh, float(scale), flags, dt, m, slot, ws.data_ptr(),
                                 ws.numel(), torch.cuda.current_stream(q_local.device).cuda_stream)
        if rc:
            _lib.check(rc, "tf_rank_pivotal")
        return slot


class NativeEditShard(NativeShard):
    """`NativeShard` for multi-edit batches (`hooks.register_edits`): with n_edits = E > 1 the pivotal pass of a block is
    ONE call of tf_rank_pivotal_edits (csrc/rank_exec.hip) -- the native form of `FrameShard._pivotal_heads_edits` /
    `_pivotal_bank_edits`, same buffer layouts, same bits on the same transport.  n_edits = 1 is `NativeShard` itself.
    Modes "heads" and "bank" (`auto_mode` answers "bank" in place of "bank_runs" for E > 1; the explicit "bank_runs" raises as
    on `FrameShard`) -- unless the shard opts in with `edit_runs`: "bank_runs" is then the executor's TF_RANK_BANK_EDIT_RUNS,
    the native form of `FrameShard._pivotal_bank_runs_edits` with the local run beside the gather (`edit_runs_multi_v`: with
    TF_ATTN_RUN_MULTI_V).  `window_edits`: window= / anchors= beside n_edits > 1 is ONE tf_rank_pivotal_frame_sets_edits call,
    the native form of `FrameShard._pivotal_window_edits`.  `ext_alloc`, `halo_block`, `halo_finish`, `propagate_all` are
    `FrameShard`'s, with n_edits."""

    supports_edits = True
    supports_window_edits = True      # window= / anchors= beside n_edits > 1: ONE tf_rank_pivotal_frame_sets_edits call

    def __init__(self, K: int, comm, halo_comm=None, attn_split: Optional[bool] = None, bank_runs: Optional[bool] = None,
                 edit_runs: Optional[bool] = None, edit_runs_multi_v: Optional[bool] = None,
                 window_edits: Optional[bool] = None, window_edits_multi_v: Optional[bool] = None):
        super().__init__(K, comm, halo_comm=halo_comm, attn_split=attn_split, bank_runs=bank_runs, edit_runs=edit_runs,
                         edit_runs_multi_v=edit_runs_multi_v, window_edits=window_edits,
                         window_edits_multi_v=window_edits_multi_v)
        self._news = {}

    @staticmethod
    def _mask(E: int, inject: bool, inject_mask: Optional[int]) -> int:
        if inject_mask is None:
            return (1 << E) - 1 if inject else 0
        mask = int(inject_mask)
        if inject or mask < 0 or mask >> E:
            raise ValueError(f"FrameShard.pivotal_attention: inject_mask {mask:#x} for {E} edits (bits below n_edits; "
                             f"`inject` must be False beside a mask)")
        return mask

    def pivotal_attention(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool,
                          mode: Optional[str] = None, out4: Optional[torch.Tensor] = None, n_edits: int = 1,
                          inject_mask: Optional[int] = None, window: Optional[int] = None, anchors=None):
        """`FrameShard.pivotal_attention` with n_edits / inject_mask; E > 1 is one tf_rank_pivotal_edits call with
        TF_RANK_NO_HALO (what the hook path calls from `attn1`).  window= / anchors=: with one edit `NativeShard`'s passes; with
        E > 1 (the shard's `window_edits` opt-in) ONE tf_rank_pivotal_frame_sets_edits call."""
        E = int(n_edits)
        anc = self._anchors(window, anchors)
        R = self._window(window, E, mode)      # (a windowed multi-edit batch raises without the window_edits opt-in)
        if E == 1:
            return super().pivotal_attention(q_local, k_local, v_local, heads, scale, inject, mode=mode, out4=out4,
                                             window=window, anchors=anchors)
        if self.world == 1 or out4 is not None or not q_local.is_cuda or q_local.dtype not in (torch.bfloat16,
                                                                                                torch.float16):
            win = dict(window=R, anchors=anc or None) if R is not None else {}
            return FrameShard.pivotal_attention(self, q_local, k_local, v_local, heads, scale, inject, mode=mode, out4=out4,
                                                n_edits=E, inject_mask=inject_mask, **win)
        mask = self._mask(E, inject, inject_mask)
        B, S, D = q_local.shape
        out = torch.empty(1 + 2 * E, self.Kl, S, D, dtype=q_local.dtype, device=q_local.device)
        self._native_edits(q_local, k_local, v_local, heads, scale, E, mask, mode, None, None, out, no_halo=True, window=R,
                           anchors=anc if R is not None else ())
        return out.view(B, S, D)

    def pivotal_block(self, q_local, k_local, v_local, heads: int, scale: float, inject: bool, ext,
                      mode: Optional[str] = None, inv_norm: bool = False, n_edits: int = 1,
                      inject_mask: Optional[int] = None, window: Optional[int] = None, anchors=None):
        E = int(n_edits)
        anc = self._anchors(window, anchors)
        R = self._window(window, E, mode)      # (a windowed multi-edit batch raises without the window_edits opt-in)
        if E == 1:
            return super().pivotal_block(q_local, k_local, v_local, heads, scale, inject, ext, mode=mode, inv_norm=inv_norm,
                                         window=window, anchors=anchors)
        mask = self._mask(E, inject, inject_mask)
        piv, inv, kfo = ext
        _, S, D = q_local.shape
        o = 1 if self.world > 1 else 0
        slot = self._native_edits(q_local, k_local, v_local, heads, scale, E, mask, mode, piv, inv, kfo, no_halo=False,
                                  inv_norm=inv_norm, window=R, anchors=anc if R is not None else ())
        reqs = [_SlotWait(self, slot, q_local.device)] if self.world > 1 else []
        return piv, inv, kfo.view((1 + 2 * E) * (self.Kl + o), S, D), reqs

    def _native_edits(self, q_local, k_local, v_local, heads, scale, E, mask, mode, piv, inv, kfo, no_halo, inv_norm=False,
                      window=None, anchors=()):
        from . import _lib
        lib = _lib.load()
        _, S, D = q_local.shape
        Kl, B = self.Kl, 1 + 2 * E
        if window is not None:      # the windowed / anchored multi-edit pass: ONE tf_rank_pivotal_frame_sets_edits call
            return self._native_window_edits(q_local, k_local, v_local, heads, scale, E, mask, piv, inv, kfo, no_halo, inv_norm,
                                             int(window), tuple(anchors))
        if mode is None:
            mode = self.auto_mode(heads, S, E)
        runs = mode == "bank_runs"
        if runs and not self.edit_runs:
            raise ValueError(_NO_EDIT_RUNS)
        dt = ops._DT.get(q_local.dtype)
        if dt is None or dt == _lib.TF_F32 or not (q_local.is_cuda and kfo.is_contiguous()
                                                    and (no_halo or (piv.is_contiguous() and inv.is_contiguous()))):
            raise TypeError("NativeEditShard: 16-bit GPU tensors, contiguous (halo-extended) buffers")

        def frames(t):     # [B*Kl, S, D] (token stride free) -> [B, Kl, S, D] view
            if t.stride(2) != 1 or t.stride(0) != S * t.stride(1):
                t = t.contiguous()
            return t.view(B, Kl, S, D) if t.is_contiguous() else t.unflatten(0, (B, Kl))
        q4, k4, v4 = frames(q_local), frames(k_local), frames(v_local)
        if k4.stride(2) != v4.stride(2) or (mode == "heads" and q4.stride(2) != k4.stride(2)):
            q4, k4, v4 = (t.contiguous() for t in (q4, k4, v4))
        strides = (ctypes.c_int64 * 8)(q4.stride(0), q4.stride(1), k4.stride(0), k4.stride(1), v4.stride(0), v4.stride(1),
                                       q4.stride(2), k4.stride(2))
        dh = D // heads
        key = (S, heads, dh, dt, q_local.device, E, runs)
        ws = self._news.get(key)
        if ws is None:
            size = lib.tf_rank_pivotal_edit_runs_workspace_bytes if runs else lib.tf_rank_pivotal_edits_workspace_bytes
            nbytes = size(self._rk, S, heads, dh, E, dt)
            ws = self._news[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=q_local.device)
        flags = 0 if self.attn_split else _lib.TF_ATTN_NO_SPLIT
        if ops.FOLD_SCALE:
            flags |= _lib.TF_ATTN_FOLD_SCALE
        if runs and self.edit_runs_multi_v:   # the executor hands the bit to the local run, the remote runs and the merge
            flags |= _lib.TF_ATTN_RUN_MULTI_V
        slot = self._slot
        if not no_halo:
            self._slot = (slot + 1) % _lib.TF_RANK_SLOTS
        m = ((_lib.TF_RANK_HEADS if mode == "heads" else _lib.TF_RANK_BANK_EDIT_RUNS if runs else _lib.TF_RANK_BANK)
             | (_lib.TF_RANK_NO_HALO if no_halo else 0)
             | (_lib.TF_RANK_INV_NORM if inv_norm else 0))
        rc = lib.tf_rank_pivotal_edits(self._rk, q4.data_ptr(), k4.data_ptr(), v4.data_ptr(), strides,
                                       None if piv is None else piv.data_ptr(), None if inv is None else inv.data_ptr(),
                                       kfo.data_ptr(), S, heads, dh, float(scale), flags, dt, m, slot, E, mask,
                                       ws.data_ptr(), ws.numel(), torch.cuda.current_stream(q_local.device).cuda_stream)
        if rc:
            _lib.check(rc, "tf_rank_pivotal_edits")
        return slot

    def _native_window_edits(self, q_local, k_local, v_local, heads, scale, E, mask, piv, inv, kfo, no_halo, inv_norm, R, anchors):
        from . import _lib
        lib = _lib.load()
        _, S, D = q_local.shape
        Kl, B = self.Kl, 1 + 2 * E
        dt = ops._DT.get(q_local.dtype)
        if dt is None or dt == _lib.TF_F32 or not (q_local.is_cuda and kfo.is_contiguous()
                                                    and (no_halo or (piv.is_contiguous() and inv.is_contiguous()))):
            raise TypeError("NativeEditShard: 16-bit GPU tensors, contiguous (halo-extended) buffers")

        def frames(t):     # [B*Kl, S, D] (token stride free) -> [B, Kl, S, D] view
            if t.stride(2) != 1 or t.stride(0) != S * t.stride(1):
                t = t.contiguous()
            return t.view(B, Kl, S, D) if t.is_contiguous() else t.unflatten(0, (B, Kl))
        q4, k4, v4 = frames(q_local), frames(k_local), frames(v_local)
        if k4.stride(2) != v4.stride(2):
            k4, v4 = k4.contiguous(), v4.contiguous()
        strides = (ctypes.c_int64 * 8)(q4.stride(0), q4.stride(1), k4.stride(0), k4.stride(1), v4.stride(0), v4.stride(1),
                                       q4.stride(2), k4.stride(2))
        dh = D // heads
        anc = (ctypes.c_int * max(len(anchors), 1))(*anchors)
        key = (S, heads, dh, dt, q_local.device, E, "window", R, anchors)
        ws = self._news.get(key)
        if ws is None:
            plan = frame_set_halo_plan(self.K, self.world, self.rank, R, anchors)      # (raises what is refused)
            nbytes = lib.tf_rank_pivotal_frame_sets_edits_workspace_bytes(self._rk, S, heads, dh, dt, R,
                                                                          ctypes.cast(anc, ctypes.c_void_p), len(anchors), E)
            assert nbytes > 0, plan
            ws = self._news[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=q_local.device)
        # the flags of `FrameShard._pivotal_window_edits`: bit-stable unless attn_split; the four-bank form off unless opted in
        hint = self._window_edits_hints(dh)
        flags = ((0 if self.attn_split else _lib.TF_ATTN_NO_SPLIT)
                 | (_lib.TF_ATTN_NO_MULTI_V if hint.get("multi_v") is False else 0)
                 | (_lib.TF_ATTN_MULTI_V if hint.get("multi_v") else 0) | (_lib.TF_ATTN_MULTI_V64 if hint.get("multi_v64") else 0))
        slot = self._slot
        if not no_halo:
            self._slot = (slot + 1) % _lib.TF_RANK_SLOTS
        m = _lib.TF_RANK_BANK | (_lib.TF_RANK_NO_HALO if no_halo else 0) | (_lib.TF_RANK_INV_NORM if inv_norm else 0)
        rc = lib.tf_rank_pivotal_frame_sets_edits(self._rk, q4.data_ptr(), k4.data_ptr(), v4.data_ptr(), strides,
                                                  None if piv is None else piv.data_ptr(),
                                                  None if inv is None else inv.data_ptr(), kfo.data_ptr(), S, heads, dh,
                                                  float(scale), flags, dt, m, slot, R, ctypes.cast(anc, ctypes.c_void_p),
                                                  len(anchors), E, mask, ws.data_ptr(), ws.numel(),
                                                  torch.cuda.current_stream(q_local.device).cuda_stream)
        if rc:
            _lib.check(rc, "tf_rank_pivotal_frame_sets_edits")
        return slot


def rank_window_edits_plan(world: int, rank: int, K: int, S: int, heads: int, dh: int, radius: int, anchors=(), n_edits: int = 2,
                           inject_mask: int = 0, dtype: torch.dtype = torch.bfloat16, no_split: bool = True,
                           no_halo: bool = False, inv_norm: bool = False, flags: int = 0, mode: Optional[int] = None) -> list:
    """The sequence ONE windowed / anchored multi-edit `NativeEditShard` block call issues on `rank` of `world` ranks, as tokens
    (tf_rank_pivotal_frame_sets_edits_plan: e.g. ['edit_pack[ns=7,nq=3]', 'a2a[slabs=7,send=3/1,recv=3/1]', <source tokens>,
    'fused[qw=1,kw=4,qb=1,prec=1,sets=2,win]', 'halo[n=7]']).  n_edits = 1 gives `rank_frame_sets_plan`, a covering radius
    `rank_edits_plan(mode="bank")`.  Recorded by the executing code itself; host only.  mode: a raw TF_RANK_* value instead of
    TF_RANK_BANK (the refusals)."""
    from . import _lib
    m = ((_lib.TF_RANK_BANK if mode is None else int(mode)) | (_lib.TF_RANK_NO_HALO if no_halo else 0)
         | (_lib.TF_RANK_INV_NORM if inv_norm else 0))
    fl = int(flags) | (_lib.TF_ATTN_NO_SPLIT if no_split else 0)
    anc = [int(a) for a in (anchors or ())]
    tab = (ctypes.c_int * max(len(anc), 1))(*anc)
    return ops._plan_tokens("tf_rank_pivotal_frame_sets_edits_plan", _lib.load().tf_rank_pivotal_frame_sets_edits_plan,
                            int(world), int(rank), int(K), S, heads, dh, int(radius), ctypes.cast(tab, ctypes.c_void_p), len(anc),
                            int(n_edits), int(inject_mask), m, fl, ops._DT[dtype])


def rank_edits_plan(world: int, rank: int, K: int, S: int, heads: int, dh: int, n_edits: int, inject_mask: int,
                    mode: str = "heads", dtype: torch.dtype = torch.bfloat16, no_split: bool = True, no_halo: bool = False,
                    inv_norm: bool = False, flags: int = 0) -> list:
    """The sequence ONE `NativeEditShard` block call issues on `rank` of `world` ranks, as tokens
    (tf_rank_pivotal_edits_plan: e.g. ['pack+inv[ns=10]', 'a2a[slabs=10]', 'vt_pack', ..., 'a2a[slabs=4]', 'unpack[nb=4]',
    'halo[n=7]']).  Recorded by the executing code itself; host only: needs no GPU and no communicator.
    mode: "heads" | "bank" | "bank_runs" (TF_RANK_BANK_RUNS: one edit only) | "bank_edit_runs" (TF_RANK_BANK_EDIT_RUNS: what a
    `NativeEditShard(edit_runs=True)` issues for "bank_runs")."""
    from . import _lib
    m = ({"heads": _lib.TF_RANK_HEADS, "bank": _lib.TF_RANK_BANK, "bank_runs": _lib.TF_RANK_BANK_RUNS,
          "bank_edit_runs": _lib.TF_RANK_BANK_EDIT_RUNS}[mode]
         | (_lib.TF_RANK_NO_HALO if no_halo else 0) | (_lib.TF_RANK_INV_NORM if inv_norm else 0))
    fl = int(flags) | (_lib.TF_ATTN_NO_SPLIT if no_split else 0)
    return ops._plan_tokens("tf_rank_pivotal_edits_plan", _lib.load().tf_rank_pivotal_edits_plan, int(world), int(rank),
                            int(K), S, heads, dh, int(n_edits), int(inject_mask), m, fl, ops._DT[dtype])


def rank_window_plan(world: int, rank: int, K: int, S: int, heads: int, dh: int, radius: int, inject: bool = False,
                     dtype: torch.dtype = torch.bfloat16, no_split: bool = True, no_halo: bool = False,
                     inv_norm: bool = False, flags: int = 0) -> list:
    """The sequence ONE windowed `NativeShard` block call issues on `rank` of `world` ranks, as tokens
    (tf_rank_pivotal_window_plan: e.g. ['halo_pack[ns=4]', 'a2a[slabs=4,send=3/1,recv=3/1]', <source tokens>, <bank tokens with
    ',win'>, 'halo[n=5]']).  Recorded by the executing code itself; host only: needs no GPU and no communicator."""
    from . import _lib
    m = _lib.TF_RANK_BANK | (_lib.TF_RANK_NO_HALO if no_halo else 0) | (_lib.TF_RANK_INV_NORM if inv_norm else 0)
    fl = int(flags) | (_lib.TF_ATTN_NO_SPLIT if no_split else 0) | (_lib.TF_ATTN_INJECT if inject else 0)
    return ops._plan_tokens("tf_rank_pivotal_window_plan", _lib.load().tf_rank_pivotal_window_plan, int(world), int(rank),
                            int(K), S, heads, dh, int(radius), m, fl, ops._DT[dtype])


def rank_frame_sets_plan(world: int, rank: int, K: int, S: int, heads: int, dh: int, radius: int, anchors=(),
                         inject: bool = False, dtype: torch.dtype = torch.bfloat16, no_split: bool = True,
                         no_halo: bool = False, inv_norm: bool = False, flags: int = 0) -> list:
    """The sequence ONE anchored windowed `NativeShard` block call issues on `rank` of `world` ranks, as tokens
    (tf_rank_pivotal_frame_sets_plan: e.g. ['set_pack[ns=4]', 'a2a[slabs=4,send=3/2/1,recv=3/1/0]', <source tokens>, <bank tokens
    with ',set' -- ',win' on a rank whose sets are all ranges in its extended bank>, 'halo[n=5]']).  No anchors give
    `rank_window_plan`, a covering radius the bank pass.  Recorded by the executing code itself; host only."""
    from . import _lib
    m = _lib.TF_RANK_BANK | (_lib.TF_RANK_NO_HALO if no_halo else 0) | (_lib.TF_RANK_INV_NORM if inv_norm else 0)
    fl = int(flags) | (_lib.TF_ATTN_NO_SPLIT if no_split else 0) | (_lib.TF_ATTN_INJECT if inject else 0)
    anc = [int(a) for a in (anchors or ())]
    tab = (ctypes.c_int * max(len(anc), 1))(*anc)
    return ops._plan_tokens("tf_rank_pivotal_frame_sets_plan", _lib.load().tf_rank_pivotal_frame_sets_plan, int(world), int(rank),
                            int(K), S, heads, dh, int(radius), ctypes.cast(tab, ctypes.c_void_p), len(anc), m, fl,
                            ops._DT[dtype])
