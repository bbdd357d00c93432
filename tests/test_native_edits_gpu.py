"""The native rank executor for multi-edit batches on an MI355X: `NativeEditShard` (ONE tf_rank_pivotal_edits call per block,
csrc/rank_exec.hip) on processes sharing cuda:0, exchanges through the library's host-transport entry points carried by gloo
(tests/gloo_transport.py) -- tests/test_sharded_gpu.py::_native_worker crossed with tests/test_shard_edits_gpu.py::_worker.

Identities under test.  Native against the Python `FrameShard` on the same transport: every buffer either fills, bit for bit,
in every form.  In the one-pass form both also equal the single-process `ops.ext_attn_edits(..., no_split=True,
multi_v=False, inject_mask=m)` slices and the `ops.propagate_chunks_edits` references bit for bit.  With attn_split=True a
rank's small grid takes other launch plans: every edit is held to the ORACLE's attention bound with its own flag."""
import datetime
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.nn_families import spread_pivots
from tests.test_sharded_gpu import _free_port

pytestmark = pytest.mark.gpu

TIMEOUT = datetime.timedelta(seconds=60)      # a rank that fails early ends the test instead of hanging its peer


def _nan_fill(ext):
    for t in ext:
        if t.dtype == torch.bfloat16:
            t.view(torch.int16).fill_(0x7fc0)
        else:
            t.view(torch.int32).fill_(0x7fc00000)


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


def _data(K, E, mask, S, h, d, n):
    B, D = 1 + 2 * E, h * d
    g = torch.Generator().manual_seed(E * 16 + mask)
    q, k, v = (torch.randn(B * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
    piv = spread_pivots(K, S, D, torch.bfloat16, g)[0].cuda()      # row norms differ: a misplaced inv_norm shows
    tgt = [(piv[c].float()[torch.randperm(S, generator=g).cuda()].repeat(n, 1)
            + 0.1 * torch.randn(n * S, D, generator=g).cuda()).bfloat16() for c in range(K)]
    res = [torch.randn(B * n, S, D, generator=g).bfloat16().cuda() for _ in range(K)]
    s = torch.arange(0, n)
    w = torch.sigmoid(torch.abs(s + n - n // 2) / (torch.abs(s - n // 2) + torch.abs(s + n - n // 2))).cuda()
    return q, k, v, piv, tgt, res, w


def _worker(rank, world, port, K, h, mode, E, mask, S, d, split, ret):
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = not split
        n = 2
        B, D = 1 + 2 * E, h * d
        q, k, v, piv, tgt, res, w = _data(K, E, mask, S, h, d, n)
        bad = []
        # ---- single process, bit-stable mode, four-bank form off: computed once, never written again
        full = ops.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, no_split=True, multi_v=False, inject_mask=mask)
        inv = ops.pivot_inv_norm(piv)
        # ---- this rank: the native form and the Python form on the same transport
        comm, halo_comm = gloo_comm(rank, world), gloo_comm(rank, world)
        sh = sharded.NativeEditShard(K, comm, halo_comm, attn_split=split)
        py = sharded.FrameShard(K, comm=comm, attn_split=split)
        Kl, f0, o = sh.Kl, sh.kf0, 1
        ref = {c: ops.propagate_chunks_edits(tgt[c], piv, inv, full, None if c == 0 else w, n, 1, c, c == 0, res[c],
                                             torch.float32 if c else torch.bfloat16, E) for c in range(f0, f0 + Kl)}
        loc = lambda t: t.view(B, K, S, D)[:, f0:f0 + Kl].reshape(B * Kl, S, D)
        tgt_all = torch.cat([tgt[f0 + j] for j in range(Kl)])
        res_all = torch.stack([res[f0 + j].view(B, n, S, D) for j in range(Kl)], dim=1).reshape(B * Kl * n, S, D)
        outs = []
        for shard, name in ((sh, "native"), (py, "python")):
            ext = shard.ext_alloc(S, D, torch.bfloat16, piv.device, n_edits=E)
            _nan_fill(ext)
            ext[0][o:].copy_(piv[f0:f0 + Kl])
            pe, ie, ke, reqs = shard.pivotal_block(loc(q), loc(k), loc(v), h, d ** -0.5, False, ext, mode=mode,
                                                   inv_norm=True, n_edits=E, inject_mask=mask)
            first, rest = shard.propagate_all(tgt_all, res_all, pe, ie, ke, w, n, halo_reqs=reqs, n_edits=E)
            torch.cuda.synchronize()
            ke4 = ke.view(B, Kl + o, S, D)
            got = ke4[:, o:].reshape(B * Kl, S, D)
            outs.append((pe.clone(), ie.clone(), ke4.clone(), first.clone(), None if rest is None else rest.clone()))
            if rank > 0 and not (torch.equal(pe[0], piv[f0 - 1]) and torch.equal(ie[0], inv[f0 - 1])):
                bad.append(f"{name}: halo slot of the pivots / inverse norms")
            if not (torch.equal(pe[o:], piv[f0:f0 + Kl]) and torch.equal(ie[o:], inv[f0:f0 + Kl])):
                bad.append(f"{name}: local pivots / inverse norms")
            if not split:      # one-pass form: the single-process results bit for bit
                if not torch.equal(got, loc(full)):
                    bad.append(f"{name}: attention slots")
                if rank > 0 and not torch.equal(ke4[:, 0], full.view(B, K, S, D)[:, f0 - 1]):
                    bad.append(f"{name}: halo slot of the attention output")
                if not torch.equal(first, ref[f0]):
                    bad.append(f"{name}: deferred first chunk")
                for j in range(1, Kl):
                    if not torch.equal(rest.view(B, Kl - 1, n, S, D)[:, j - 1].reshape(B * n, S, D), ref[f0 + j]):
                        bad.append(f"{name}: chunk {f0 + j}")
            elif shard is sh:  # every edit against the oracle on [source | uncond_e | cond_e] with ITS flag
                from tests.test_kernels_gpu import attn_bound, attn_ref
                worst = 0.0
                for e in range(E):
                    sl = [0, 1 + 2 * e, 2 + 2 * e]
                    q3, k3, v3 = (t.view(B, K, S, D)[sl].reshape(3 * K, S, D).float().cpu() for t in (q, k, v))
                    r, r_abs, _ = attn_ref(q3, k3, v3, h, d ** -0.5, bool((mask >> e) & 1), need_sigma=False)
                    pick = lambda x: x.view(3, K, S, D)[:, f0:f0 + Kl]
                    err = (got.view(B, Kl, S, D)[sl].float().cpu() - pick(r)).abs()
                    worst = max(worst, float((err - attn_bound(pick(r), pick(r_abs))).max()))
                print(f"rank {rank}: attn_split, worst excess over the attention bound {worst:.3e}")
                if worst > 0:
                    bad.append(f"attention exceeds the oracle bound by {worst:.3e}")
        # ---- native and Python: the same bits in every buffer they fill (the unset halo slot of rank 0 excluded)
        lo = 0 if rank > 0 else o
        (pe_n, ie_n, ke_n, first_n, rest_n), (pe_p, ie_p, ke_p, first_p, rest_p) = outs
        for what, a, b in (("pivots", pe_n[lo:], pe_p[lo:]), ("inverse norms", ie_n[lo:], ie_p[lo:]),
                           ("attention output", ke_n[:, lo:], ke_p[:, lo:]), ("first chunk", first_n, first_p)):
            if not torch.equal(a, b):
                bad.append(f"native != python: {what}")
        if (rest_n is None) != (rest_p is None) or (rest_n is not None and not torch.equal(rest_n, rest_p)):
            bad.append("native != python: rest")
        # ---- the attention alone (TF_RANK_NO_HALO: what the hook path calls from attn1), strided q/k/v slabs of one buffer
        qkv = torch.cat([loc(q), loc(k), loc(v)], dim=-1)
        qs, ks, vs = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        a_n = sh.pivotal_attention(qs, ks, vs, h, d ** -0.5, False, mode=mode, n_edits=E, inject_mask=mask)
        a_p = py.pivotal_attention(qs, ks, vs, h, d ** -0.5, False, mode=mode, n_edits=E, inject_mask=mask)
        torch.cuda.synchronize()
        if not torch.equal(a_n, a_p):
            bad.append("native != python: pivotal_attention on strided slabs")
        if not split and not torch.equal(a_n, loc(full)):
            bad.append("pivotal_attention on strided slabs")
        sh.close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001  (reported once, through the shared dict; nothing is retried)
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,K,h,mode,E,mask,S,d,split", [
    (2, 4, 2, "heads", 2, 0b11, 320, 40, False),       # uniform injection, streaming launches, slot 0 alone on the wire
    (2, 5, 2, "heads", 3, 0b101, 320, 40, False),      # uneven runs (3 + 2), a mixed mask: compact q / k on the wire
    (2, 4, 2, "bank", 2, 0b00, 320, 40, False),        # no source slot: b0 = 1
    (2, 5, 2, "bank", 3, 0b010, 320, 40, False),       # the compact-q staging region
    (2, 4, 2, "heads", 2, 0b01, 64, 160, False),       # the fused regime: the bank sets in one launch
    (2, 4, 2, "heads", 3, 0b101, 320, 40, True),       # attn_split=True: against the oracle bound
    (2, 2, 2, "heads", 8, 0xA5, 64, 40, False),        # 19 halo messages, the 48-slab pack kernels
    (8, 8, 8, "heads", 2, 0b10, 192, 40, False),       # one keyframe per rank
    (8, 25, 5, "bank", 2, 0b01, 192, 40, False)])      # runs 4,3,3,3,3,3,3,3; the heads do not divide
def test_native_edit_executor(world, K, h, mode, E, mask, S, d, split):
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), K, h, mode, E, mask, S, d, split, ret), nprocs=world, join=True)
    assert dict(ret) == {r: [] for r in range(world)}, dict(ret)


def _one_edit_worker(rank, world, port, ret):
    """n_edits = 1 through `NativeEditShard` is `NativeShard`: the same call, the same bits."""
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        K, h, S, d, n = 5, 2, 192, 40, 2
        D = h * d
        q, k, v, piv, tgt, res, w = _data(K, 1, 0, S, h, d, n)
        comm = gloo_comm(rank, world)
        one, edit = sharded.NativeShard(K, comm), sharded.NativeEditShard(K, comm)
        Kl, f0, o = one.Kl, one.kf0, 1
        loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)
        bad = []
        for mode, inject in (("heads", True), ("bank", False)):
            outs = []
            for shard in (one, edit):
                ext = shard.ext_alloc(S, D, torch.bfloat16, piv.device)
                _nan_fill(ext)
                ext[0][o:].copy_(piv[f0:f0 + Kl])
                kw = {} if shard is one else dict(n_edits=1)
                pe, ie, ke, reqs = shard.pivotal_block(loc(q), loc(k), loc(v), h, d ** -0.5, inject, ext, mode=mode,
                                                       inv_norm=True, **kw)
                for r in reqs:
                    r.wait()
                att = shard.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, inject, mode=mode, **kw)
                torch.cuda.synchronize()
                outs.append((pe.clone(), ie.clone(), ke.clone(), att.clone()))
            lo = 0 if rank > 0 else o
            (pe_a, ie_a, ke_a, att_a), (pe_b, ie_b, ke_b, att_b) = outs
            ke_a, ke_b = ke_a.view(3, Kl + o, S, D), ke_b.view(3, Kl + o, S, D)
            same = (torch.equal(pe_a[lo:], pe_b[lo:]) and torch.equal(ie_a[lo:], ie_b[lo:])
                    and torch.equal(ke_a[:, lo:], ke_b[:, lo:]) and torch.equal(att_a, att_b))
            if not same:
                bad.append(f"{mode}: NativeEditShard(n_edits=1) != NativeShard")
            if not torch.equal(outs[1][3], ops.ext_attn(q, k, v, h, d ** -0.5, inject, no_split=True)
                               .view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)):
                bad.append(f"{mode}: attention")
        one.close()
        edit.close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_one_edit_is_the_native_shard():
    ret = mp.Manager().dict()
    mp.spawn(_one_edit_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)


@pytest.mark.parametrize("E,mask,S,d", [(2, 0b01, 320, 40), (3, 0b101, 64, 160)])
def test_single_rank(E, mask, S, d):
    """World of one (no communicator): the inverse norms, then tf_ext_attn_fwd_edits_masked straight into the state."""
    from tokenflow_amd import ops, sharded
    K, h, n = 4, 2, 2
    D = h * d
    q, k, v, piv, _tgt, _res, _w = _data(K, E, mask, S, h, d, n)
    sh = sharded.NativeEditShard(K, None)
    ext = sh.ext_alloc(S, D, torch.bfloat16, q.device, n_edits=E)
    _nan_fill(ext)
    ext[0].copy_(piv)
    pe, ie, ke, reqs = sh.pivotal_block(q, k, v, h, d ** -0.5, False, ext, inv_norm=True, n_edits=E, inject_mask=mask)
    torch.cuda.synchronize()
    assert reqs == []
    assert torch.equal(ke, ops.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, no_split=True, inject_mask=mask))
    assert torch.equal(ie, ops.pivot_inv_norm(piv))
    with pytest.raises(ValueError):
        sh.pivotal_block(q, k, v, h, d ** -0.5, True, ext, n_edits=E, inject_mask=mask)      # inject beside a mask
    sh.close()


def _hooks_worker(rank, world, port, K, ret):
    """`register_frame_shard(NativeEditShard)` + `register_edits` + `register_edit_schedules` with schedules that disagree at
    the step under test, on the small fake pipeline with the REAL kernels under autocast: one pivotal pass and the chunk passes
    of a decoder block give the block outputs of the same run on `FrameShard`, bit for bit."""
    _init(rank, world, port)
    try:
        import tokenflow_utils as tfu
        from tests import fake_diffusers as fd
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        E, n, S, h, dims = 2, 2, 192, 2, (80, 160, 320)
        B, D = 1 + 2 * E, dims[0]

        def pipe(shard):
            torch.manual_seed(0)
            p = fd.FakePipeline(dims=dims, heads=h, cross_dim=32).eval().cuda().bfloat16()
            tfu.register_extended_attention_pnp(p, [1])
            tfu.set_tokenflow(p.unet)
            tfu.register_time(p, 1)
            tfu.register_edits(p, E)
            tfu.register_edit_schedules(p, qk_schedules=[[1], []])      # edit 0 injects at t = 1, edit 1 never
            tfu.register_frame_shard(p, shard)
            return p, p.unet.up_blocks[3].attentions[1].transformer_blocks[0]
        g = torch.Generator().manual_seed(1)
        x_piv = torch.randn(B, K, S, D, generator=g).cuda().bfloat16()
        enc = torch.randn(B, K, 7, 32, generator=g).cuda().bfloat16()
        enc_n = torch.randn(B * n, 7, 32, generator=g).cuda().bfloat16()
        chunks = []
        for c in range(K):
            perm = torch.randperm(S, generator=g)
            src = x_piv[0, c][perm][None].repeat(n, 1, 1)
            chunks.append(torch.cat([src, torch.randn((B - 1) * n, S, D, generator=g).cuda().bfloat16()]))
        comm = gloo_comm(rank, world)
        native, python = sharded.NativeEditShard(K, comm), sharded.FrameShard(K, comm=comm)
        outs = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for shard in (native, python):
                p, blk = pipe(shard)
                lo, hi = shard.kf0, shard.kf0 + shard.Kl
                tfu.register_pivotal(p, True)
                got = [blk(x_piv[:, lo:hi].reshape(B * shard.Kl, S, D),
                           encoder_hidden_states=enc[:, lo:hi].reshape(B * shard.Kl, 7, 32)).clone()]
                tfu.register_pivotal(p, False)
                for c in range(lo, hi):
                    tfu.register_batch_idx(p, c)
                    got.append(blk(chunks[c], encoder_hidden_states=enc_n).clone())
                torch.cuda.synchronize()
                outs.append(got)
        bad = [f"block output {i}" for i, (a, b) in enumerate(zip(*outs)) if not torch.equal(a, b)]
        if any(bool(torch.isnan(a).any()) for a in outs[0]):
            bad.append("NaN in a block output")
        native.close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_hooks_two_ranks_native_multi_edit():
    ret = mp.Manager().dict()
    mp.spawn(_hooks_worker, args=(2, _free_port(), 4, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)
