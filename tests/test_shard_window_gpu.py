"""Sliding-window keyframe bank on a frame shard on an MI355X: `FrameShard` / `NativeShard` with window=R on processes sharing
cuda:0, exchanges through the library's host-transport entry points carried by gloo (tests/gloo_transport.py).

  G1  a rank's windowed pass in the bit-stable mode equals ONE process issuing the same two calls on the full tensors
      (`ops.ext_attn_windows_views(part="bank")` with `ops.bank_windows(K, R)` + the source-only call), bit for bit.
  G2  ... and `ops.ext_attn_windows(no_split=True)` bit for bit wherever the plans name the same kernel form -- asserted for
      every shape used here -- and the oracle on every frame's window within the attention bound.
  G3  a covering radius is today's "bank" pass, world 1 the windowed single-GPU call.
The neighbour halo of the propagation is checked by one `propagate_all` of the rank's chunks behind the pass."""
import datetime
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.nn_families import spread_pivots
from tests.test_sharded_gpu import _free_port

pytestmark = pytest.mark.gpu

TIMEOUT = datetime.timedelta(seconds=60)      # a rank that fails early ends the test instead of hanging its peer

# (S, H, Dh, inject, dtype): S = 64 the fused small-problem path, S = 320 the streaming path (above 256 tokens, ragged)
CASES = [(S, H, Dh, inject, torch.bfloat16) for S in (64, 320) for H, Dh in ((2, 40), (2, 64)) for inject in (False, True)]
CASES += [(320, 1, 80, False, torch.bfloat16), (320, 1, 80, True, torch.bfloat16), (320, 2, 40, True, torch.float16)]


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


def _nan_fill(ext):
    for t in ext:
        if t.element_size() == 2:
            t.view(torch.int16).fill_(0x7fc0 if t.dtype == torch.bfloat16 else 0x7e00)
        else:
            t.view(torch.int32).fill_(0x7fc00000)


def _strip(plan):
    return [re.sub(r"qw=\d,", "", t.replace(",win", "")) for t in plan if t != "vt_pack"]


def same_form(full, bank, src):
    """The windowed call and its two parts name the same kernel forms: the bank launch is the call's first launch; the source
    launch is the call's SOURCE launch, or -- where the call computes the source branch inside its one ALL / fused launch -- the
    SOURCE form of that launch (fused launches agree in KW and PREC, whatever their query waves)."""
    full, bank, src = _strip(full), _strip(bank), _strip(src)
    if len(bank) != 1 or len(src) != 1 or bank[0] != full[0]:
        return False
    if len(full) == 2:
        return full[1] == src[0]
    return len(full) == 1 and (src[0] == full[0].replace("ALL", "SOURCE"))


def _composition(ops, q, k, v, K, H, scale, inject, R):
    """ONE process, the same two calls on the full tensors (bit-stable mode)."""
    _, S, D = q.shape
    q4, k4, v4 = (t.view(3, K, S, D) for t in (q, k, v))
    out = torch.empty_like(q4)
    ops.ext_attn_views(q4, k4, v4, out, H, scale, inject, "source", no_split=True)
    if inject:
        ops.ext_attn_windows_views(q4, k4[0:1], v4[1:3], out, H, scale, True, ops.bank_windows(K, R), "bank",
                                   branch0=(0, 0, 1, 0), no_split=True)
    else:
        ops.ext_attn_windows_views(q4, k4[1:3], v4[1:3], out, H, scale, False, ops.bank_windows(K, R), "bank",
                                   branch0=(0, 1, 1, 0), no_split=True)
    return out.view(3 * K, S, D)


def _win(t, K, f0, f1):
    return t.view(3, K, *t.shape[1:])[:, f0:f1].reshape(3 * (f1 - f0), *t.shape[1:])


def _worker(rank, world, port, K, radii, cases, ret):
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tests.test_kernels_gpu import attn_bound, attn_ref
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        bad, n = [], 2
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
            for R in radii:
                what = f"K{K} W{world} R{R} S{S} H{H} Dh{Dh} inject={inject} {dtype} rank {rank}"
                cover = R >= K - 1
                windows = ops.bank_windows(K, R)
                # ---- single process, computed once per (case, radius), never written again
                if cover:      # G3: today's pass
                    comp = full = ops.ext_attn(q, k, v, H, scale, inject, no_split=True)
                else:
                    comp = _composition(ops, q, k, v, K, H, scale, inject, R)
                    full = ops.ext_attn_windows(q, k, v, H, scale, inject, windows, no_split=True)
                    plans = (ops.attn_windows_plan(K, windows, S, H, Dh, inject, dtype=dtype, no_split=True),
                             ops.attn_windows_part_plan(K, K, 0, windows, S, H, Dh, inject, dtype=dtype, no_split=True),
                             ops.attn_plan(K, K, S, H, Dh, inject, dtype=dtype, part="source", no_split=True))
                    if not same_form(*plans):      # the shapes are chosen so that the forms agree at every one of them
                        bad.append(f"{what}: the plans name different kernel forms {plans}")
                    if not torch.equal(comp, full):
                        bad.append(f"{what}: G2, the two parts != ext_attn_windows(no_split=True)")
                # ---- the oracle on every local frame's window, within the attention bound
                worst = float("-inf")
                for i in range(f0, f0 + Kl):
                    lo, m = windows[i]
                    r, ra, _ = attn_ref(*(_win(t, K, lo, lo + m).float().cpu() for t in (q, k, v)), H, scale, inject,
                                        need_sigma=False)
                    pick = lambda t: t.view(3, m, S, D)[:, i - lo]      # noqa: E731
                    err = (_win(comp, K, i, i + 1).view(3, S, D).float().cpu() - pick(r)).abs()
                    worst = max(worst, float((err - attn_bound(pick(r), pick(ra), dtype=dtype)).max()))
                print(f"{what}: worst excess over the attention bound {worst:.3e}")
                if worst > 0:
                    bad.append(f"{what}: exceeds the oracle's attention bound by {worst:.3e}")
                ref = {c: ops.propagate_chunks(tgt[c], piv, inv, comp, None if c == 0 else w, n, 1, c, c == 0, res[c],
                                               torch.float32 if c else dtype) for c in (f0,)}
                for name, sh in shards:
                    att = sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R)
                    torch.cuda.synchronize()
                    if not torch.equal(att, loc(comp)):
                        bad.append(f"{what} {name}: G1, pivotal_attention(window=)")
                    if name == "dist":      # (the halo of this transport is covered by tests/test_sharded_gpu.py)
                        continue
                    ext = sh.ext_alloc(S, D, dtype, piv.device)
                    _nan_fill(ext)
                    ext[0][o:].copy_(piv[f0:f0 + Kl])
                    pe, ie, ke, reqs = sh.pivotal_block(loc(q), loc(k), loc(v), H, scale, inject, ext, inv_norm=True, window=R)
                    first, _rest = sh.propagate_all(tgt_all, res_all, pe, ie, ke, w, n, halo_reqs=reqs)
                    torch.cuda.synchronize()
                    ke4 = ke.view(3, Kl + o, S, D)
                    if not torch.equal(ke4[:, o:].reshape(3 * Kl, S, D), loc(comp)):
                        bad.append(f"{what} {name}: G1, pivotal_block(window=)")
                    if not (torch.equal(pe[o:], piv[f0:f0 + Kl]) and torch.equal(ie[o:], inv[f0:f0 + Kl])):
                        bad.append(f"{what} {name}: local pivots / inverse norms")
                    if rank > 0 and not (torch.equal(pe[0], piv[f0 - 1]) and torch.equal(ie[0], inv[f0 - 1])
                                         and torch.equal(ke4[:, 0], comp.view(3, K, S, D)[:, f0 - 1])):
                        bad.append(f"{what} {name}: halo slot")
                    if not torch.equal(first, ref[f0]):
                        bad.append(f"{what} {name}: first chunk of the propagation")
        shards[1][1].close()
        shards[2][1].close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001  (reported once, through the shared dict; nothing is retried)
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,K,radii", [(2, 5, (1,)), (3, 7, (1, 2, 3, 6))], ids=["K5-W2", "K7-W3"])
@pytest.mark.parametrize("part", [0, 1, 2], ids=["S64", "S320", "d80-f16"])
def test_windowed_shard(world, K, radii, part):
    """K = 5 over 2 ranks (3, 2), R = 1: one-sided halos, clipped windows.  K = 7 over 3 ranks (3, 2, 2): R = 1 plain neighbour
    halos, R = 2 two-sided halos on the middle rank, R = 3 a halo that spans two ranks and a local frame that goes to two
    peers, R = 6 covers the bank.  Several cases inside ONE spawn per world."""
    cases = [CASES[0:4], CASES[4:8], CASES[8:]][part]
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), K, radii, cases, ret), nprocs=world, join=True)
    assert dict(ret) == {r: [] for r in range(world)}, dict(ret)


def _split_worker(rank, world, port, ret):
    """attn_split=True on a windowed shard: a rank's small grid may split the windows over extra workgroups and merge, so the
    result is held to the ORACLE's attention bound on every frame's window (not to the bit-stable call); the native executor
    and the Python form issue the same launches: the same bits."""
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tests.test_kernels_gpu import attn_bound, attn_ref
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = False
        K, R = 7, 2
        comm = gloo_comm(rank, world)
        py, nat = sharded.FrameShard(K, comm=comm, attn_split=True), sharded.NativeShard(K, comm, attn_split=True)
        Kl, f0 = py.Kl, py.kf0
        bad = []
        for S, H, Dh, inject in ((320, 2, 40, False), (320, 2, 64, True), (64, 2, 40, True)):
            D, scale = H * Dh, Dh ** -0.5
            g = torch.Generator().manual_seed(S + Dh)
            q, k, v = (torch.randn(3 * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
            loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)      # noqa: E731
            outs = [sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R).clone() for sh in (py, nat)]
            torch.cuda.synchronize()
            what = f"attn_split S{S} Dh{Dh} inject={inject} rank {rank}"
            if not torch.equal(*outs):
                bad.append(f"{what}: native != python")
            worst = float("-inf")
            for i in range(f0, f0 + Kl):
                lo, m = ops.bank_windows(K, R)[i]
                r, ra, _ = attn_ref(*(_win(t, K, lo, lo + m).float().cpu() for t in (q, k, v)), H, scale, inject,
                                    need_sigma=False)
                pick = lambda t: t.view(3, m, S, D)[:, i - lo]      # noqa: E731
                err = (outs[0].view(3, Kl, S, D)[:, i - f0].float().cpu() - pick(r)).abs()
                worst = max(worst, float((err - attn_bound(pick(r), pick(ra))).max()))
            print(f"{what}: worst excess over the attention bound {worst:.3e}")
            if worst > 0:
                bad.append(f"{what}: exceeds the oracle's attention bound by {worst:.3e}")
        nat.close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_attn_split_on_a_windowed_shard():
    ret = mp.Manager().dict()
    mp.spawn(_split_worker, args=(3, _free_port(), ret), nprocs=3, join=True)
    assert dict(ret) == {0: [], 1: [], 2: []}, dict(ret)


def _planted_worker(rank, world, port, ret):
    """One bank key per window edge with a dominant score: query (frame 3, token 5) of the middle rank (frames 3, 4 of 7 over
    3 ranks, R = 2: window [1, 5]) finds its own vector times 12 as a key in frame 1 (arrives from rank 0), in frame 5 (from
    rank 2) and in frame 0 and 6, just outside.  The two inside keys tie, so the output is the mean of their values (-1); a
    value of 100 sits on the outside keys."""
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        K, R, S, H, Dh = 7, 2, 64, 2, 40
        D, scale = H * Dh, Dh ** -0.5
        g = torch.Generator().manual_seed(7)
        q, k, v = (torch.randn(3, K, S, D, generator=g).bfloat16() for _ in range(3))
        for b in (1, 2):
            for f, tok, val in ((1, 7, 3.0), (5, 9, -5.0), (0, 11, 100.0), (6, 13, 100.0)):
                k[b, f, tok] = (q[b, 3, 5].float() * 12.0).bfloat16()
                v[b, f, tok] = val
        q, k, v = (t.reshape(3 * K, S, D).cuda() for t in (q, k, v))
        comm = gloo_comm(rank, world)
        bad = []
        for name, sh in (("python", sharded.FrameShard(K, comm=comm)), ("native", sharded.NativeShard(K, comm))):
            loc = lambda t: t.view(3, K, S, D)[:, sh.kf0:sh.kf0 + sh.Kl].reshape(3 * sh.Kl, S, D)      # noqa: E731
            out = sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, False, window=R).view(3, sh.Kl, S, D)
            torch.cuda.synchronize()
            if rank == 1:
                got = out[1:, 0, 5].float()
                print(f"{name}: planted query reads {got.min().item():.4f} .. {got.max().item():.4f} (want -1)")
                if not bool(((got + 1.0).abs() < 0.05).all()):
                    bad.append(f"{name}: planted keys: {got.min().item()} .. {got.max().item()}, want -1")
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_planted_keys_at_the_window_edges():
    ret = mp.Manager().dict()
    mp.spawn(_planted_worker, args=(3, _free_port(), ret), nprocs=3, join=True)
    assert dict(ret) == {0: [], 1: [], 2: []}, dict(ret)


@pytest.mark.parametrize("strided", [False, True])
def test_halo_pack(strided):
    """`ops.window_halo_pack` against torch indexing: dense slabs and column slabs of a fused-QKV buffer (row stride 3D), a
    frame in two segments, an empty side, more than one workgroup."""
    from tokenflow_amd import ops
    Kl, S, D = 3, 72, 80
    g = torch.Generator().manual_seed(3)
    if strided:
        qkv = torch.randn(3, Kl, S, 3 * D, generator=g).bfloat16().cuda()
        k3, v3 = qkv[..., D:2 * D], qkv[..., 2 * D:]
    else:
        k3, v3 = (torch.randn(3, Kl, S, D, generator=g).bfloat16().cuda() for _ in range(2))
    for slabs in ([k3[1], k3[2], v3[1], v3[2]], [k3[0], v3[1], v3[2]]):
        for segs in ([(0, 3), (0, 3), (2, 1)], [(0, 0), (0, 3), (1, 2)], [(1, 1), (0, 0), (0, 0)], [(0, 0), (0, 0)]):
            got = ops.window_halo_pack(slabs, segs)
            frames = [f for f0, n in segs for f in range(f0, f0 + n)]
            want = torch.stack([torch.stack([s[f] for s in slabs]) for f in frames]) if frames else got
            assert got.shape == (len(frames), len(slabs), S, D) and torch.equal(got, want), (strided, segs)
    with pytest.raises(ValueError):
        ops.window_halo_pack([k3[0]], [(2, 2)])
    # more 16-byte pieces than 2048 workgroups of 256 threads hold (10 MB): the grid-stride path
    big = torch.randn(2, 2, 1024, 320, generator=g).bfloat16().cuda()
    slabs, segs = [big[0], big[1], big[1], big[0]], [(1, 1), (0, 2), (0, 1)]
    got = ops.window_halo_pack(slabs, segs)
    want = torch.stack([torch.stack([s[f] for s in slabs]) for f in (1, 0, 1, 0)])
    assert got.numel() * 2 // 16 > 2048 * 256 and torch.equal(got, want)


@pytest.mark.parametrize("S,H,Dh,inject", [(64, 2, 40, True), (320, 2, 64, False)])
def test_world_one_and_loopback(S, H, Dh, inject):
    """G3 in-process: a world of one (no communicator, a loopback communicator of one rank, `FrameShard` without a process
    group) is `ops.ext_attn_windows(no_split=True)` bit for bit; a covering radius is `ops.ext_attn`.  Rank 1 of a 3-rank
    loopback world runs the whole windowed schedule on one GPU: its source branch, which needs nothing from the exchange,
    equals the single-process one."""
    from tokenflow_amd import ops, sharded
    from tokenflow_amd.comm import HipComm
    K, R = 6, 1
    D, scale = H * Dh, Dh ** -0.5
    g = torch.Generator().manual_seed(S + Dh)
    q, k, v = (torch.randn(3 * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
    piv = torch.randn(K, S, D, generator=g).bfloat16().cuda()
    want = ops.ext_attn_windows(q, k, v, H, scale, inject, ops.bank_windows(K, R), no_split=True)
    whole = ops.ext_attn(q, k, v, H, scale, inject, no_split=True)
    for sh in (sharded.NativeShard(K, None), sharded.NativeShard(K, HipComm.loopback(0, 1)), sharded.FrameShard(K)):
        ext = sh.ext_alloc(S, D, torch.bfloat16, q.device)
        ext[0].copy_(piv)
        _pe, ie, ke, reqs = sh.pivotal_block(q, k, v, H, scale, inject, ext, inv_norm=True, window=R)
        torch.cuda.synchronize()
        assert reqs == [] and torch.equal(ke, want) and torch.equal(ie, ops.pivot_inv_norm(piv))
        assert torch.equal(sh.pivotal_attention(q, k, v, H, scale, inject, window=R), want)
        assert torch.equal(sh.pivotal_attention(q, k, v, H, scale, inject, window=K - 1), whole)
    sh = sharded.NativeShard(K, HipComm.loopback(1, 3))
    loc = lambda t: t.view(3, K, S, D)[:, 2:4].reshape(6, S, D)      # noqa: E731
    got = sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=R)
    torch.cuda.synchronize()
    assert torch.equal(got.view(3, 2, S, D)[0], want.view(3, K, S, D)[0, 2:4])
    with pytest.raises(ValueError):
        sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, inject, window=-1)
    sh.close()


def _hooks_worker(rank, world, port, K, ret):
    """`register_frame_shard` + `register_bank_window(pipe, 1, shard=True)` on the small fake pipeline with the REAL kernels
    under autocast: the pivotal pass of a decoder block equals the unsharded windowed hook pass on the rank's keyframes (G2:
    S = 192, Dh = 40, the fused form on both sides)."""
    _init(rank, world, port)
    try:
        import tokenflow_utils as tfu
        from tests import fake_diffusers as fd
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        S, h, dims = 192, 2, (80, 160, 320)
        D = dims[0]
        win = ops.bank_windows(K, 1)      # the precondition of the bit-equality: the fused form on both sides
        plans = (ops.attn_windows_plan(K, win, S, h, D // h, True, no_split=True),
                 ops.attn_windows_part_plan(K, K, 0, win, S, h, D // h, True, no_split=True),
                 ops.attn_plan(K, K, S, h, D // h, True, part="source", no_split=True))
        assert same_form(*plans) and all(p[0].startswith("fused") for p in plans), plans

        def pipe(registered, **kw):
            torch.manual_seed(0)
            p = fd.FakePipeline(dims=dims, heads=h, cross_dim=32).eval().cuda().bfloat16()
            tfu.register_extended_attention_pnp(p, [1])
            tfu.set_tokenflow(p.unet)
            tfu.register_time(p, 1)
            if registered is not None:
                tfu.register_frame_shard(p, registered)
            tfu.register_bank_window(p, 1, **kw)
            tfu.register_pivotal(p, True)
            return p, p.unet.up_blocks[3].attentions[1].transformer_blocks[0]
        g = torch.Generator().manual_seed(1)
        x = torch.randn(3, K, S, D, generator=g).cuda().bfloat16()
        enc = torch.randn(3, K, 7, 32, generator=g).cuda().bfloat16()
        bad = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            _, blk = pipe(None)
            want = blk(x.reshape(3 * K, S, D), encoder_hidden_states=enc.reshape(3 * K, 7, 32)).view(3, K, S, D).clone()
            comm = gloo_comm(rank, world)
            for name, sh in (("python", sharded.FrameShard(K, comm=comm)), ("native", sharded.NativeShard(K, comm))):
                lo, hi = sh.kf0, sh.kf0 + sh.Kl
                xl, el = x[:, lo:hi].reshape(3 * sh.Kl, S, D), enc[:, lo:hi].reshape(3 * sh.Kl, 7, 32)
                _, blk = pipe(sh, shard=True)
                got = blk(xl, encoder_hidden_states=el).view(3, sh.Kl, S, D)
                torch.cuda.synchronize()
                if not torch.equal(got, want[:, lo:hi]):
                    bad.append(f"{name}: block output of the windowed shard")
                _, blk = pipe(sh)      # without the opt-in the old error stays
                try:
                    blk(xl, encoder_hidden_states=el)
                    bad.append(f"{name}: no error without shard=True")
                except ValueError as e:
                    if "on a registered frame shard is not supported" not in str(e):
                        bad.append(f"{name}: {e}")
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_hooks_two_ranks_windowed_shard():
    ret = mp.Manager().dict()
    mp.spawn(_hooks_worker, args=(2, _free_port(), 4, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)
