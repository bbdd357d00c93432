"""Anchor keyframes on a windowed frame shard on an MI355X: `FrameShard` / `NativeShard` with window=R, anchors=A on processes
sharing cuda:0, exchanges through the library's host-transport entry points carried by gloo (tests/gloo_transport.py).

  I1  a rank's anchored pass in the bit-stable mode equals ONE process issuing the same two calls on the full tensors
      (`ops.ext_attn_frame_sets_views(part="bank")` with `ops.bank_frame_sets(K, R, anchors)` + the source-only call), bit for
      bit wherever the rank's plans and the single process's name the same kernel form (K <= 64);
  I2  ... and that composition equals `ops.ext_attn_frame_sets(no_split=True)` bit for bit where the forms agree;
  I3  every local keyframe lies within the oracle's attention bound of the attention over its member frames gathered in
      ascending order, and equals its OWN CALL (`ops.ext_attn` on the gathered tensors, Kq = 1) bit for bit wherever both name
      the same form -- every K, K > 64 included;
  I4  anchors=() is the windowed pass, a covering radius the "bank" pass, world 1 the single-GPU frame-set call, anchors inside
      every window add nothing.
A rank's kernel form follows ITS largest set; at the geometries of `MUST_AGREE` every rank has the whole bank's, and a
disagreement there fails the test instead of excusing the rank from I1."""
import datetime
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.nn_families import spread_pivots
from tests.test_shard_window_gpu import CASES, _nan_fill
from tests.test_sharded_gpu import _free_port

pytestmark = pytest.mark.gpu

TIMEOUT = datetime.timedelta(seconds=60)      # a rank that fails early ends the test instead of hanging its peer

# (K, world, radius, anchors): every rank's largest set is the bank's largest set (4, 4, 5 and 2 frames): I1 / I2 are required
MUST_AGREE = {(5, 2, 1, (0,)), (7, 3, 1, (0,)), (7, 3, 1, (0, 3, 6)), (7, 3, 0, (0,))}
# (radius, anchors or an int stride); an anchor set that does not fit K is left out of that world
CONFIGS = [(1, (0,)), (1, (0, 3, 6)), (0, (0,)), (2, 3), (1, ()), (6, (0,))]


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


def _members(m):
    return [j for j in range(m.bit_length()) if (m >> j) & 1]


def _strip(plan):
    return [re.sub(r"qw=\d,", "", t.replace(",win", "").replace(",set", "")) for t in plan if t != "vt_pack"]


def same_form(full, bank, src):
    """`same_form` of tests/test_shard_window_gpu.py with the ',set' mark ignored like ',win': a whole call and two parts name
    the same kernel forms."""
    full, bank, src = _strip(full), _strip(bank), _strip(src)
    if len(bank) != 1 or len(src) != 1 or bank[0] != full[0]:
        return False
    if len(full) == 2:
        return full[1] == src[0]
    return len(full) == 1 and (src[0] == full[0].replace("ALL", "SOURCE"))


def _gather(t, K, frames):
    idx = torch.as_tensor(list(frames), device=t.device)
    return t.view(3, K, *t.shape[1:])[:, idx].reshape(3 * len(frames), *t.shape[1:]).contiguous()


def _composition(ops, q, k, v, K, H, scale, inject, sets):
    """ONE process, the same two calls on the full tensors (bit-stable mode)."""
    _, S, D = q.shape
    q4, k4, v4 = (t.view(3, K, S, D) for t in (q, k, v))
    out = torch.empty_like(q4)
    ops.ext_attn_views(q4, k4, v4, out, H, scale, inject, "source", no_split=True)
    if inject:
        ops.ext_attn_frame_sets_views(q4, k4[0:1], v4[1:3], out, H, scale, True, sets, "bank", branch0=(0, 0, 1, 0),
                                      no_split=True)
    else:
        ops.ext_attn_frame_sets_views(q4, k4[1:3], v4[1:3], out, H, scale, False, sets, "bank", branch0=(0, 1, 1, 0),
                                      no_split=True)
    return out.view(3 * K, S, D)


def _rank_forms(ops, sharded, K, world, r, R, anchors, S, H, Dh, inject, dtype):
    """(bank tokens, source tokens) of rank r's two attention calls."""
    pl = sharded.frame_set_halo_plan(K, world, r, R, anchors)
    if not anchors:      # (the windowed plan)
        return (ops.attn_windows_part_plan(pl.F, pl.Kl, pl.hl, pl.windows, S, H, Dh, inject, dtype=dtype, no_split=True),
                ops.attn_plan(pl.Kl, pl.Kl, S, H, Dh, inject, dtype=dtype, part="source", no_split=True))
    return (ops.attn_frame_sets_part_plan(pl.F, pl.Kl, pl.q_frame0, pl.sets, S, H, Dh, inject, dtype=dtype, no_split=True),
            ops.attn_plan(pl.Kl, pl.Kl, S, H, Dh, inject, dtype=dtype, part="source", no_split=True))


def _i3(ops, got, q, k, v, K, f0, Kl, member_lists, rank_plans, S, H, Dh, scale, inject, dtype, what, bad, bound_only=False):
    """I3 on the local frames of one rank: `got` [3*Kl,S,D] against the oracle on the gathered members, and bit for bit against
    each frame's own call where the forms agree.  Returns (worst excess over the bound, frames compared bit for bit)."""
    from tests.test_kernels_gpu import attn_bound, attn_ref
    worst, n_equal = float("-inf"), 0
    D = H * Dh
    for i in range(f0, f0 + Kl):
        fr = member_lists[i - f0]
        r, ra, _ = attn_ref(*(_gather(t, K, fr).float().cpu() for t in (q, k, v)), H, scale, inject, need_sigma=False)
        pick = lambda t: t.view(3, len(fr), S, D)[:, fr.index(i)]      # noqa: E731
        mine = got.view(3, Kl, S, D)[:, i - f0]
        err = (mine.float().cpu() - pick(r)).abs()
        worst = max(worst, float((err - attn_bound(pick(r), pick(ra), dtype=dtype)).max()))
        if bound_only:
            continue
        own_plan = ops.attn_plan(len(fr), 1, S, H, Dh, inject, dtype=dtype, no_split=True)
        if same_form(own_plan, *rank_plans):
            own = ops.ext_attn(_gather(q, K, [i]), _gather(k, K, fr), _gather(v, K, fr), H, scale, inject,
                               q_frame0=fr.index(i), no_split=True)
            n_equal += 1
            if not torch.equal(own.view(3, S, D), mine):
                bad.append(f"{what}: I3, frame {i} != its own call on members {fr}")
    if worst > 0:
        bad.append(f"{what}: I3, exceeds the oracle's attention bound by {worst:.3e}")
    return worst, n_equal


def _worker(rank, world, port, K, configs, cases, ret):
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        bad, n, left_out, pairs = [], 2, 0, 0
        comm = gloo_comm(rank, world)
        shards = [("python", sharded.FrameShard(K, comm=comm)), ("native", sharded.NativeShard(K, comm)),
                  ("native-edit", sharded.NativeEditShard(K, comm)), ("dist", sharded.FrameShard(K))]
        Kl, f0, o = shards[0][1].Kl, shards[0][1].kf0, 1
        for ci, (S, H, Dh, inject, dtype) in enumerate(cases):
            D, scale = H * Dh, Dh ** -0.5
            g = torch.Generator().manual_seed(100 * K + ci)
            q, k, v = (torch.randn(3 * K, S, D, generator=g).to(dtype).cuda() for _ in range(3))
            piv = spread_pivots(K, S, D, dtype, g)[0].cuda()
            inv = ops.pivot_inv_norm(piv)
            tgt = [(piv[c].float()[torch.randperm(S, generator=g).cuda()].repeat(n, 1)
                    + 0.1 * torch.randn(n * S, D, generator=g).cuda()).to(dtype) for c in range(K)]
            res = [torch.randn(3 * n, S, D, generator=g).to(dtype).cuda() for _ in range(K)]
            s = torch.arange(0, n)
            w = torch.sigmoid(torch.abs(s + n - n // 2) / (torch.abs(s - n // 2) + torch.abs(s + n - n // 2))).cuda()
            loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)      # noqa: E731
            tgt_all = torch.cat([tgt[f0 + j] for j in range(Kl)])
            res_all = torch.stack([res[f0 + j].view(3, n, S, D) for j in range(Kl)], dim=1).reshape(3 * Kl * n, S, D)
            for R, spec in configs:
                anchors = tuple(range(0, K, spec)) if isinstance(spec, int) else tuple(spec)
                what = f"K{K} W{world} R{R} anchors{anchors} S{S} H{H} Dh{Dh} inject={inject} {dtype} rank {rank}"
                cover, pairs = R >= K - 1, pairs + 1
                sets = ops.bank_frame_sets(K, R, anchors)
                src_plan = ops.attn_plan(K, K, S, H, Dh, inject, dtype=dtype, part="source", no_split=True)
                # ---- single process, computed once per (case, configuration), never written again
                if cover:      # I4: today's pass
                    comp = ops.ext_attn(q, k, v, H, scale, inject, no_split=True)
                    agree = [True] * world
                else:
                    comp = _composition(ops, q, k, v, K, H, scale, inject, sets)
                    full = ops.ext_attn_frame_sets(q, k, v, H, scale, inject, sets, no_split=True)
                    bank_plan = ops.attn_frame_sets_part_plan(K, K, 0, sets, S, H, Dh, inject, dtype=dtype, no_split=True)
                    plans = (ops.attn_frame_sets_plan(K, sets, S, H, Dh, inject, dtype=dtype, no_split=True), bank_plan, src_plan)
                    if same_form(*plans):
                        if not torch.equal(comp, full):
                            bad.append(f"{what}: I2, the two parts != ext_attn_frame_sets(no_split=True)")
                    elif (K, world, R, anchors) in MUST_AGREE:
                        bad.append(f"{what}: the plans name different kernel forms {plans}")
                    # does every rank name the single process's forms?  (host arithmetic: each rank answers for all)
                    agree = []
                    for r in range(world):
                        rb, rs = _rank_forms(ops, sharded, K, world, r, R, anchors, S, H, Dh, inject, dtype)
                        agree.append(_strip(rb) == _strip(bank_plan) and _strip(rs) == _strip(src_plan))
                    if (K, world, R, anchors) in MUST_AGREE and not all(agree):
                        bad.append(f"{what}: a rank's kernel form differs from the single process's at a required geometry: {agree}")
                i1 = agree[rank]
                left_out += 0 if i1 else 1
                outs = {}
                for name, sh in shards:
                    outs[name] = sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R, anchors=anchors)
                torch.cuda.synchronize()
                for name, _ in shards[1:]:      # the same bits on the same transport
                    if not torch.equal(outs[name], outs["python"]):
                        bad.append(f"{what} {name}: != the python shard")
                if i1 and not torch.equal(outs["python"], loc(comp)):
                    bad.append(f"{what}: I1, pivotal_attention(window=, anchors=)")
                if not anchors:      # I4: the windowed pass itself
                    if not torch.equal(shards[1][1].pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R),
                                       outs["native"]):
                        bad.append(f"{what}: I4, anchors=() != the windowed pass")
                # ---- I3, form-independent
                member_lists = [_members(sets[i]) for i in range(f0, f0 + Kl)]
                rank_plans = (None, None) if cover else _rank_forms(ops, sharded, K, world, rank, R, anchors, S, H, Dh, inject, dtype)
                worst, n_eq = _i3(ops, outs["python"], q, k, v, K, f0, Kl, member_lists, rank_plans, S, H, Dh, scale, inject,
                                  dtype, what, bad, bound_only=cover)
                print(f"{what}: worst excess over the attention bound {worst:.3e}; {n_eq}/{Kl} frames equal their own call; "
                      f"I1 {'checked' if i1 else 'left out'}")
                # ---- the block call and the propagation behind it: the halo slot and the first chunk
                blocks = {}
                for name, sh in shards[:3]:      # (the halo of the torch.distributed transport: tests/test_sharded_gpu.py)
                    ext = sh.ext_alloc(S, D, dtype, piv.device)
                    _nan_fill(ext)
                    ext[0][o:].copy_(piv[f0:f0 + Kl])
                    pe, ie, ke, reqs = sh.pivotal_block(loc(q), loc(k), loc(v), H, scale, inject, ext, inv_norm=True, window=R,
                                                        anchors=anchors)
                    first, _rest = sh.propagate_all(tgt_all, res_all, pe, ie, ke, w, n, halo_reqs=reqs)
                    torch.cuda.synchronize()
                    ke4 = ke.view(3, Kl + o, S, D)
                    blocks[name] = (ke4, first)
                    if not torch.equal(ke4[:, o:].reshape(3 * Kl, S, D), outs["python"]):
                        bad.append(f"{what} {name}: pivotal_block(window=, anchors=) != pivotal_attention")
                    if not (torch.equal(pe[o:], piv[f0:f0 + Kl]) and torch.equal(ie[o:], inv[f0:f0 + Kl])):
                        bad.append(f"{what} {name}: local pivots / inverse norms")
                    if rank > 0 and not (torch.equal(pe[0], piv[f0 - 1]) and torch.equal(ie[0], inv[f0 - 1])):
                        bad.append(f"{what} {name}: halo slot (pivots / inverse norms)")
                    if rank > 0 and not torch.equal(ke4[:, 0], blocks["python"][0][:, 0]):
                        bad.append(f"{what} {name}: halo slot != the python shard's")
                    if not torch.equal(first, blocks["python"][1]):
                        bad.append(f"{what} {name}: first chunk != the python shard's")
                if all(agree):      # every rank holds the single process's bits: the halo slot and the chunk against it
                    ke4, first = blocks["python"]
                    ref = ops.propagate_chunks(tgt[f0], piv, inv, comp, None if f0 == 0 else w, n, 1, f0, f0 == 0, res[f0],
                                               torch.float32 if f0 else dtype)
                    if rank > 0 and not torch.equal(ke4[:, 0], comp.view(3, K, S, D)[:, f0 - 1]):
                        bad.append(f"{what}: halo slot != the single process's frame {f0 - 1}")
                    if not torch.equal(first, ref):
                        bad.append(f"{what}: first chunk of the propagation")
            if ci == 0:      # I4: anchors that already lie inside every window add nothing
                R, a = (K - 1) // 2, ((K - 1) // 2,)
                assert all((m >> a[0]) & 1 for m in ops.bank_frame_sets(K, R, ()))
                for name, sh in shards[:2]:
                    if not torch.equal(sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R, anchors=a),
                                       sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R)):
                        bad.append(f"K{K} W{world} {name} rank {rank}: I4, an anchor inside every window changes the result")
        print(f"K{K} W{world} rank {rank}: I1 left out for {left_out} of {pairs} (case, configuration) pairs")
        shards[1][1].close()
        shards[2][1].close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001  (reported once, through the shared dict; nothing is retried)
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,K", [(2, 5), (3, 7)], ids=["K5-W2", "K7-W3"])
@pytest.mark.parametrize("part", [0, 1, 2], ids=["S64", "S320", "d80-f16"])
def test_anchored_shard(world, K, part):
    """K = 5 over 2 ranks (3, 2) and K = 7 over 3 ranks (3, 2, 2): anchor 0 (rank 0 owns it and sends it to every peer; rank 0's
    sets are ranges, the others' are not), anchors in every rank, radius 0, every 3rd keyframe at radius 2, no anchors (the
    windowed pass), a covering radius (the bank pass).  Several cases inside ONE spawn per world."""
    cases = [CASES[0:4], CASES[4:8], CASES[8:]][part]
    configs = [(R, a) for R, a in CONFIGS if isinstance(a, int) or all(x < K for x in a)]
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), K, configs, cases, ret), nprocs=world, join=True)
    assert dict(ret) == {r: [] for r in range(world)}, dict(ret)


def _big_worker(rank, world, port, ret):
    """K = 66 > 64 over 3 ranks, R = 2, anchors {0, 33}: no single-GPU frame-set call holds this bank; every rank's extended bank
    has 25 / 27 / 26 frames.  I3 on every local keyframe; native == python bit for bit."""
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        K, R, anchors, dtype = 66, 2, (0, 33), torch.bfloat16
        comm = gloo_comm(rank, world)
        py, nat = sharded.FrameShard(K, comm=comm), sharded.NativeShard(K, comm)
        Kl, f0 = py.Kl, py.kf0
        pl = sharded.frame_set_halo_plan(K, world, rank, R, anchors)
        member_lists = [[pl.U[j] for j in _members(m)] for m in pl.sets]
        assert all(fr == sorted(set(range(max(0, i - R), min(K - 1, i + R) + 1)) | set(anchors))
                   for i, fr in zip(range(f0, f0 + Kl), member_lists))
        bad = []
        for S, H, Dh, inject in ((64, 2, 40, False), (64, 2, 40, True), (320, 2, 64, True)):
            D, scale = H * Dh, Dh ** -0.5
            g = torch.Generator().manual_seed(S + Dh + inject)
            q, k, v = (torch.randn(3 * K, S, D, generator=g).to(dtype).cuda() for _ in range(3))
            loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)      # noqa: E731
            outs = [sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R, anchors=anchors).clone()
                    for sh in (py, nat)]
            torch.cuda.synchronize()
            what = f"K66 S{S} Dh{Dh} inject={inject} rank {rank}"
            if not torch.equal(*outs):
                bad.append(f"{what}: native != python")
            rank_plans = _rank_forms(ops, sharded, K, world, rank, R, anchors, S, H, Dh, inject, dtype)
            worst, n_eq = _i3(ops, outs[0], q, k, v, K, f0, Kl, member_lists, rank_plans, S, H, Dh, scale, inject, dtype, what,
                              bad)
            print(f"{what}: worst excess over the attention bound {worst:.3e}; {n_eq}/{Kl} frames equal their own call")
        nat.close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_more_than_64_keyframes():
    ret = mp.Manager().dict()
    mp.spawn(_big_worker, args=(3, _free_port(), ret), nprocs=3, join=True)
    assert dict(ret) == {0: [], 1: [], 2: []}, dict(ret)


def _split_worker(rank, world, port, ret):
    """attn_split=True on an anchored shard: the result is held to the ORACLE's attention bound on every frame's members (not to
    the bit-stable call); the native executor and the Python form issue the same launches: the same bits."""
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = False
        K, R, anchors = 7, 2, (0,)
        comm = gloo_comm(rank, world)
        py, nat = sharded.FrameShard(K, comm=comm, attn_split=True), sharded.NativeShard(K, comm, attn_split=True)
        Kl, f0 = py.Kl, py.kf0
        sets = ops.bank_frame_sets(K, R, anchors)
        bad = []
        for S, H, Dh, inject in ((320, 2, 40, False), (320, 2, 64, True), (64, 2, 40, True)):
            D, scale = H * Dh, Dh ** -0.5
            g = torch.Generator().manual_seed(S + Dh)
            q, k, v = (torch.randn(3 * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
            loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)      # noqa: E731
            outs = [sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R, anchors=anchors).clone()
                    for sh in (py, nat)]
            torch.cuda.synchronize()
            what = f"attn_split S{S} Dh{Dh} inject={inject} rank {rank}"
            if not torch.equal(*outs):
                bad.append(f"{what}: native != python")
            worst, _ = _i3(ops, outs[0], q, k, v, K, f0, Kl, [_members(sets[i]) for i in range(f0, f0 + Kl)], None, S, H, Dh,
                           scale, inject, torch.bfloat16, what, bad, bound_only=True)
            print(f"{what}: worst excess over the attention bound {worst:.3e}")
        nat.close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_attn_split_on_an_anchored_shard():
    ret = mp.Manager().dict()
    mp.spawn(_split_worker, args=(3, _free_port(), ret), nprocs=3, join=True)
    assert dict(ret) == {0: [], 1: [], 2: []}, dict(ret)


def _planted_worker(rank, world, port, ret):
    """K = 7 over 3 ranks, R = 1, anchor 0.  Query (frame 6, token 5) of the last rank (window {5, 6}, members {0, 5, 6}) finds
    its own vector times 12 as a key in frame 0 -- the anchor: it arrives from rank 0 and lies outside the window -- and in
    frame 5; the two member keys tie, so the output is the mean of their values (-1).  The same key with value 100 sits in
    frames 2 and 3, members of neither.  Misplaced anchor rows in the receive buffer, or masks off by the q_frame0 shift, read
    another frame's rows: any trace of 100, or a missing member, fails."""
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        K, R, S, H, Dh = 7, 1, 64, 2, 40
        D, scale = H * Dh, Dh ** -0.5
        g = torch.Generator().manual_seed(7)
        q, k, v = (torch.randn(3, K, S, D, generator=g).bfloat16() for _ in range(3))
        for b in (1, 2):
            for f, tok, val in ((0, 7, 3.0), (5, 9, -5.0), (2, 11, 100.0), (3, 13, 100.0)):
                k[b, f, tok] = (q[b, 6, 5].float() * 12.0).bfloat16()
                v[b, f, tok] = val
        q, k, v = (t.reshape(3 * K, S, D).cuda() for t in (q, k, v))
        comm = gloo_comm(rank, world)
        bad = []
        for name, sh in (("python", sharded.FrameShard(K, comm=comm)), ("native", sharded.NativeShard(K, comm))):
            loc = lambda t: t.view(3, K, S, D)[:, sh.kf0:sh.kf0 + sh.Kl].reshape(3 * sh.Kl, S, D)      # noqa: E731
            out = sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, False, window=R, anchors=(0,)).view(3, sh.Kl, S, D)
            torch.cuda.synchronize()
            if rank == 2:
                assert sh.kf0 + 1 == 6
                got = out[1:, 1, 5].float()
                print(f"{name}: planted query reads {got.min().item():.4f} .. {got.max().item():.4f} (want -1)")
                if not bool(((got + 1.0).abs() < 0.05).all()):
                    bad.append(f"{name}: planted keys: {got.min().item()} .. {got.max().item()}, want -1")
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_planted_keys_in_the_anchor():
    ret = mp.Manager().dict()
    mp.spawn(_planted_worker, args=(3, _free_port(), ret), nprocs=3, join=True)
    assert dict(ret) == {0: [], 1: [], 2: []}, dict(ret)


# ------------------------------------------------------------------------------------------------------ the pack kernel
def _pack_want(slabs, masks):
    frames = [f for m in masks for f in _members(m)]
    return frames, (torch.stack([torch.stack([s[f] for s in slabs]) for f in frames]) if frames else None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ns", [3, 4, 6])
def test_frame_set_halo_pack(dtype, ns):
    """`ops.frame_set_halo_pack` against torch indexing: strided slab views (frame stride != S * ld, ld > D), an empty peer, a
    full peer, a frame sent to three peers, a non-contiguous mask."""
    from tokenflow_amd import ops
    Kl, S, D = 3, 3, 8
    g = torch.Generator().manual_seed(3 + ns)
    buf = torch.randn(6, Kl + 1, S + 2, 3 * D, generator=g).to(dtype).cuda()
    slabs = [buf[i, :Kl, 1:1 + S, D * (i % 3):D * (i % 3) + D] for i in range(ns)]
    assert slabs[0].stride(0) != S * slabs[0].stride(1) and slabs[0].stride(1) > D
    for masks in ([0b000, 0b111, 0b101], [0b010, 0b010, 0b011, 0b110], [0b100], [0b111] * 5, [0, 0]):
        got = ops.frame_set_halo_pack(slabs, masks)
        frames, want = _pack_want(slabs, masks)
        assert got.shape == (len(frames), ns, S, D), masks
        assert want is None or torch.equal(got, want), masks
    out = torch.full((3, ns, S, D), 7.0, dtype=dtype, device="cuda")      # into a given buffer
    assert ops.frame_set_halo_pack(slabs, [0b001, 0b110], out=out) is out and torch.equal(out, _pack_want(slabs, [1, 6])[1])


def test_frame_set_halo_pack_64_frames_and_refusals():
    from tokenflow_amd import _lib, ops
    Kl, S, D = 64, 1, 8
    g = torch.Generator().manual_seed(5)
    slabs = [torch.randn(Kl, S, D, generator=g).bfloat16().cuda() for _ in range(4)]
    for masks in ([1 << 63], [(1 << 64) - 1], [1 << 63, (1 << 64) - 1, 0, 1]):
        got = ops.frame_set_halo_pack(slabs, masks)
        assert torch.equal(got, _pack_want(slabs, masks)[1]), masks
    # rows of more 16-byte pieces than one workgroup holds: several workgroups per row (ny = 141 for 36000 pieces: every thread
    # copies at most one piece, none strides -- tests/test_grid_stride_gpu.py has the rows whose workgroups do)
    big = [torch.randn(5, 300, 320, generator=g).bfloat16().cuda() for _ in range(3)]
    masks = [0b10110, 0b00001, 0, 0b11111]
    assert torch.equal(ops.frame_set_halo_pack(big, masks), _pack_want(big, masks)[1])
    small = [t[:3] for t in slabs]
    with pytest.raises(ValueError):
        ops.frame_set_halo_pack(small, [0b1000])      # a bit at or above Kl
    with pytest.raises(_lib.TokenflowHipError, match="tf_frame_set_halo_pack"):
        ops.frame_set_halo_pack([t.float() for t in small], [0b1])      # fp32
    mis = torch.zeros(3 * 1 * 16 + 8, dtype=torch.bfloat16, device="cuda")[4:4 + 48].view(3, 1, 16)      # 8 bytes off
    with pytest.raises(_lib.TokenflowHipError, match="aligned"):
        ops.frame_set_halo_pack([mis], [0b1])


# ------------------------------------------------------------------------------------------------------ the part entry point
@pytest.mark.parametrize("S,H,Dh,inject,dtype", CASES, ids=[f"S{c[0]}-H{c[1]}-Dh{c[2]}-{'inj' if c[3] else 'no'}-{c[4]}"
                                                            .replace("torch.", "") for c in CASES])
def test_part_entry_point(S, H, Dh, inject, dtype):
    from tokenflow_amd import ops
    K, D, scale = 7, H * Dh, Dh ** -0.5
    g = torch.Generator().manual_seed(S + Dh)
    q, k, v = (torch.randn(3 * K, S, D, generator=g).to(dtype).cuda() for _ in range(3))
    q4, k4, v4 = (t.view(3, K, S, D) for t in (q, k, v))
    kb, vb, b0 = (k4[0:1], v4[1:3], (0, 0, 1, 0)) if inject else (k4[1:3], v4[1:3], (0, 1, 1, 0))
    # the two parts == the whole frame-set call
    sets = ops.bank_frame_sets(K, 1, (0, 6))
    plans = (ops.attn_frame_sets_plan(K, sets, S, H, Dh, inject, dtype=dtype, no_split=True),
             ops.attn_frame_sets_part_plan(K, K, 0, sets, S, H, Dh, inject, dtype=dtype, no_split=True),
             ops.attn_plan(K, K, S, H, Dh, inject, dtype=dtype, part="source", no_split=True))
    assert same_form(*plans), plans
    assert any(t.endswith(",set") or t.endswith(",set]") for t in plans[1]), plans[1]
    comp = _composition(ops, q, k, v, K, H, scale, inject, sets)
    assert torch.equal(comp, ops.ext_attn_frame_sets(q, k, v, H, scale, inject, sets, no_split=True))
    # part "all" is the frame-set call itself
    out = torch.empty_like(q4)
    ops.ext_attn_frame_sets_views(q4, k4, v4, out, H, scale, inject, sets, "all", no_split=True)
    assert torch.equal(out.view(3 * K, S, D), comp)
    # all-range sets: the windowed part, in bits and tokens
    windows = ops.bank_windows(K, 2)
    ranges = [((1 << n) - 1) << lo for lo, n in windows]
    assert (ops.attn_frame_sets_part_plan(K, K, 0, ranges, S, H, Dh, inject, dtype=dtype, no_split=True)
            == ops.attn_windows_part_plan(K, K, 0, windows, S, H, Dh, inject, dtype=dtype, no_split=True))
    a, b = torch.zeros_like(q4), torch.zeros_like(q4)
    ops.ext_attn_frame_sets_views(q4, kb, vb, a, H, scale, inject, ranges, "bank", branch0=b0, no_split=True)
    ops.ext_attn_windows_views(q4, kb, vb, b, H, scale, inject, windows, "bank", branch0=b0, no_split=True)
    assert torch.equal(a, b) and not a[1:].eq(0).all() and a[0].eq(0).all()
    # full sets: the strided bank-only call; a sub-range of query frames with q_frame0
    a, b = torch.zeros(3, 2, S, D, dtype=dtype, device="cuda"), torch.zeros(3, 2, S, D, dtype=dtype, device="cuda")
    ops.ext_attn_frame_sets_views(q4[:, 3:5], kb, vb, a, H, scale, inject, [(1 << K) - 1] * 2, "bank", branch0=b0, q_frame0=3,
                                  no_split=True)
    ops.ext_attn_views(q4[:, 3:5], kb, vb, b, H, scale, inject, "bank", branch0=b0, q_frame0=3, no_split=True)
    assert torch.equal(a, b)
    assert (ops.attn_frame_sets_part_plan(K, 2, 3, [(1 << K) - 1] * 2, S, H, Dh, inject, dtype=dtype, no_split=True)
            == ops.attn_plan(K, 2, S, H, Dh, inject, dtype=dtype, part="bank", no_split=True))
    # ... and with sets: frames 3, 4 of the whole call (the form does not depend on Kq at these shapes: asserted)
    ops.ext_attn_frame_sets_views(q4[:, 3:5], kb, vb, a, H, scale, inject, sets[3:5], "bank", branch0=b0, q_frame0=3,
                                  no_split=True)
    sub = ops.attn_frame_sets_part_plan(K, 2, 3, sets[3:5], S, H, Dh, inject, dtype=dtype, no_split=True)
    assert _strip(sub) == _strip(plans[1]), (sub, plans[1])
    assert torch.equal(a[1:], comp.view(3, K, S, D)[1:, 3:5])
    with pytest.raises(ValueError, match="set-free"):      # the source part flag is refused
        ops.ext_attn_frame_sets_views(q4, k4, v4, out, H, scale, inject, sets, "source")


@pytest.mark.parametrize("S,H,Dh,inject", [(64, 2, 40, True), (320, 2, 64, False)])
def test_world_one(S, H, Dh, inject):
    """I4 in-process: a world of one is `ops.ext_attn_frame_sets(no_split=True)` bit for bit; a covering radius is `ops.ext_attn`
    whatever the anchors; rank 1 of a 3-rank loopback world runs the whole anchored schedule on one GPU (its source branch needs
    nothing from the exchange)."""
    from tokenflow_amd import ops, sharded
    from tokenflow_amd.comm import HipComm
    K, R, anchors = 6, 1, (0, 5)
    D, scale = H * Dh, Dh ** -0.5
    g = torch.Generator().manual_seed(S + Dh)
    q, k, v = (torch.randn(3 * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
    piv = torch.randn(K, S, D, generator=g).bfloat16().cuda()
    want = ops.ext_attn_frame_sets(q, k, v, H, scale, inject, ops.bank_frame_sets(K, R, anchors), no_split=True)
    whole = ops.ext_attn(q, k, v, H, scale, inject, no_split=True)
    for sh in (sharded.NativeShard(K, None), sharded.NativeShard(K, HipComm.loopback(0, 1)), sharded.FrameShard(K)):
        ext = sh.ext_alloc(S, D, torch.bfloat16, q.device)
        ext[0].copy_(piv)
        _pe, ie, ke, reqs = sh.pivotal_block(q, k, v, H, scale, inject, ext, inv_norm=True, window=R, anchors=anchors)
        torch.cuda.synchronize()
        assert reqs == [] and torch.equal(ke, want) and torch.equal(ie, ops.pivot_inv_norm(piv))
        assert torch.equal(sh.pivotal_attention(q, k, v, H, scale, inject, window=R, anchors=anchors), want)
        assert torch.equal(sh.pivotal_attention(q, k, v, H, scale, inject, window=K - 1, anchors=anchors), whole)
        with pytest.raises(ValueError):
            sh.pivotal_attention(q, k, v, H, scale, inject, anchors=anchors)
    sh = sharded.NativeShard(K, HipComm.loopback(1, 3))
    loc = lambda t: t.view(3, K, S, D)[:, 2:4].reshape(6, S, D)      # noqa: E731
    got = sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R, anchors=anchors)
    torch.cuda.synchronize()
    assert torch.equal(got.view(3, 2, S, D)[0], want.view(3, K, S, D)[0, 2:4])
    with pytest.raises(ValueError):
        sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R, anchors=(6,))
    sh.close()
