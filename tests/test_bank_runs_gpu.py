"""The "bank_runs" exchange pattern of the pivotal pass on an MI355X: `NativeShard` (tf_rank_pivotal, TF_RANK_BANK_RUNS) and
the Python `FrameShard` on processes sharing one GPU, exchanges carried by gloo (tests/gloo_transport.py).

Guarantee under test: equal bit for bit to a single-process `ops.ext_attn_runs` with the same runs, and to
the oracle within the attention bound -- not to the bit-stable single-GPU call.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.nn_families import spread_pivots
from tests.test_sharded_gpu import _attn_oracle_bound, _free_port

pytestmark = pytest.mark.gpu


def _runs_of(K, world, rank):
    counts = [K // world + (1 if r < K % world else 0) for r in range(world)]
    f0, Kl = sum(counts[:rank]), counts[rank]
    return f0, Kl, [(f0, Kl)] + ([(0, f0)] if f0 else []) + ([(f0 + Kl, K - f0 - Kl)] if f0 + Kl < K else [])


def _nan_fill(t):
    t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).fill_(0x7fc0 if t.dtype == torch.bfloat16 else 0x7fc00000)


def _worker(rank, world, port, K, h, inject, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        S, d = 192, 40
        D = h * d
        scale = d ** -0.5
        g = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(3 * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
        piv = spread_pivots(K, S, D, torch.bfloat16, g)[0].cuda()      # row norms differ: a misplaced inv_norm shows
        inv = ops.pivot_inv_norm(piv)
        comm, halo_comm = gloo_comm(rank, world), gloo_comm(rank, world)
        sh = sharded.NativeShard(K, comm, halo_comm)
        py = sharded.FrameShard(K, comm=comm)                 # the Python form on the same transport
        Kl, f0 = sh.Kl, sh.kf0
        o = 1
        msgs = []
        f0_, Kl_, runs = _runs_of(K, world, rank)
        if (f0_, Kl_) != (f0, Kl) or py.bank_runs_of_rank() != runs:
            msgs.append(f"runs {py.bank_runs_of_rank()} != {runs}")
        loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)   # noqa: E731
        # single-process reference: the same runs over the full tensors (one-pass runs: the shards' default)
        one = ops.ext_attn_runs(loc(q).contiguous(), k, v, h, scale, inject, runs, q_frame0=f0, no_split=True)
        o_ref, o_bound = _attn_oracle_bound(q, k, v, h, d, inject)
        if not bool(((one.float().cpu() - loc(o_ref)).abs() <= loc(o_bound)).all()):
            msgs.append("single-process ext_attn_runs outside the oracle bound")
        if rank > 0:      # what the left neighbour sends: the last keyframe of ITS run set
            fl, Kll, runs_l = _runs_of(K, world, rank - 1)
            ql = q.view(3, K, S, D)[:, fl:fl + Kll].reshape(3 * Kll, S, D).contiguous()
            left = ops.ext_attn_runs(ql, k, v, h, scale, inject, runs_l, q_frame0=fl, no_split=True).view(3, Kll, S, D)[:, -1]
        outs = []
        for shard in (sh, py):
            ext = shard.ext_alloc(S, D, torch.bfloat16, piv.device)
            for block in range(2):     # the second block finds every buffer of the first one NaN-filled
                for t in ext:
                    _nan_fill(t)
                for b in shard._bufs.values():                 # send / receive buffers of the Python host
                    _nan_fill(b)
                for b in getattr(shard, "_nws", {}).values():  # the native executor's workspace: exchange buffers, V^T image,
                    b.fill_(0xFF)                              # norm table, slot counts, partial results
                ext[0][o:].copy_(piv[f0:f0 + Kl])
                if shard is py:    # the native executor computes the inverse norms inside its pack launch (TF_RANK_INV_NORM)
                    ops.pivot_inv_norm(ext[0][o:], out=ext[1][o:])
                pe, ie, ke, reqs = shard.pivotal_block(loc(q), loc(k), loc(v), h, scale, inject, ext, mode="bank_runs",
                                                       inv_norm=shard is sh)
                shard.halo_wait(reqs)
                torch.cuda.synchronize()
                dist.barrier()
            ke4 = ke.view(3, Kl + o, S, D)
            got = ke4[:, o:].reshape(3 * Kl, S, D)
            name = "native" if shard is sh else "python"
            if not torch.equal(got, one):
                msgs.append(f"{name}: differs from single-process ext_attn_runs ({float((got.float() - one.float()).abs().max()):.3e})")
            if not bool(((got.float().cpu() - loc(o_ref)).abs() <= loc(o_bound)).all()):
                msgs.append(f"{name}: outside the oracle bound")
            if not (torch.equal(pe[o:], piv[f0:f0 + Kl]) and torch.equal(ie[o:], inv[f0:f0 + Kl])):
                msgs.append(f"{name}: local pivots / inverse norms")
            if rank > 0:           # the halo slot holds the left neighbour's last keyframe
                if not (torch.equal(pe[0], piv[f0 - 1]) and torch.equal(ie[0], inv[f0 - 1]) and torch.equal(ke4[:, 0], left)):
                    msgs.append(f"{name}: halo slot")
            outs.append((pe.clone(), ie.clone(), ke.clone()))
        # the attention alone (TF_RANK_NO_HALO), strided q/k/v slabs of one fused projection buffer
        qkv = torch.cat([loc(q), loc(k), loc(v)], dim=-1)
        qs, ks, vs = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        a_n = sh.pivotal_attention(qs, ks, vs, h, scale, inject, mode="bank_runs")
        a_p = py.pivotal_attention(qs, ks, vs, h, scale, inject, mode="bank_runs")
        torch.cuda.synchronize()
        if not (torch.equal(a_n, one) and torch.equal(a_p, one)):
            msgs.append("pivotal_attention on strided slabs")
        # native and Python forms: the same bits in every buffer they fill (the unset halo slot of rank 0 excluded)
        lo = 0 if rank > 0 else o
        (pe_n, ie_n, ke_n), (pe_p, ie_p, ke_p) = outs
        if not (torch.equal(pe_n[lo:], pe_p[lo:]) and torch.equal(ie_n[lo:], ie_p[lo:])
                and torch.equal(ke_n.view(3, Kl + o, S, D)[:, lo:], ke_p.view(3, Kl + o, S, D)[:, lo:])):
            msgs.append("native != python")
        sh.close()
        ret[rank] = "; ".join(msgs)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,K,h,inject", [
    (2, 4, 2, False), (2, 4, 2, True), (2, 5, 2, False), (2, 5, 2, True),
    (8, 8, 8, True), (8, 25, 5, False)])
def test_bank_runs_native_python_and_single_process_agree(world, K, h, inject):
    port = _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, K, h, inject, ret), nprocs=world, join=True)
    assert dict(ret) == {r: "" for r in range(world)}


def test_world1_ignores_the_mode_and_loopback_completes():
    """World of one: plain attention whatever the mode.  The loopback transport at 'rank 3 of 8' with the wire model on:
    every launch, size check and stream hand-over of the bank_runs schedule runs; the source branch never leaves the rank
    and is exact whatever the transport delivers."""
    from tokenflow_amd import ops, sharded
    from tokenflow_amd.comm import HipComm
    K, S, h, d = 8, 256, 8, 40
    D = h * d
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(3 * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
    sh = sharded.NativeShard(K, None)
    ext = sh.ext_alloc(S, D, torch.bfloat16, q.device)
    for inject in (False, True):
        pe, ie, ke, reqs = sh.pivotal_block(q, k, v, h, d ** -0.5, inject, ext, mode="bank_runs")
        assert reqs == [] and torch.equal(ke, ops.ext_attn(q, k, v, h, d ** -0.5, inject, no_split=True))
        py = sharded.FrameShard(K)
        assert torch.equal(py.pivotal_attention(q, k, v, h, d ** -0.5, inject, mode="bank_runs"),
                           ops.ext_attn(q, k, v, h, d ** -0.5, inject, no_split=True))
    sh.close()
    comm = HipComm.loopback(3, 8, wire=(25.0, 50.0))
    sh = sharded.NativeShard(K, comm, attn_split=True)
    assert (sh.Kl, sh.kf0) == (1, 3) and sh.bank_runs_of_rank() == [(3, 1), (0, 3), (4, 4)]
    ext = sh.ext_alloc(S, D, torch.bfloat16, q.device)
    ext[0][1:].normal_()
    ops.pivot_inv_norm(ext[0][1:], out=ext[1][1:])
    ql, kl, vl = (t.view(3, K, S, D)[:, 3:4].reshape(3, S, D) for t in (q, k, v))
    for inject in (False, True):
        pe, ie, ke, reqs = sh.pivotal_block(ql, kl, vl, h, d ** -0.5, inject, ext, mode="bank_runs")
        for r in reqs:
            r.wait()
        torch.cuda.synchronize()
        want = ops.ext_attn(ql, kl, vl, h, d ** -0.5, inject, part="source", no_split=True, fused=False)
        assert torch.equal(ke.view(3, 2, S, D)[0, 1], want[0])
    sh.close()
    comm.close()
