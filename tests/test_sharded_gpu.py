"""Frame-sharded path with the REAL HIP ops: 2 ranks sharing cuda:0 over gloo (RCCL refuses two
ranks on one device; the collectives are backend-agnostic torch.distributed calls).  Each rank's
sharded results in FrameShard's default one-pass form must equal the single-GPU results IN THE BIT-STABLE MODE
(TF_ATTN_NO_SPLIT on both sides: kernel choice and key split are then functions of the shape alone) bit for bit --
same kernels, partitioned work.  The single-GPU DEFAULT mode may pick another key split for large grids of small
frames (cfg2 level 2: KW = 1 instead of the rank's KW = 4); against that the sharded results agree within the
attention's parity bound (test_shard_vs_default_and_bit_stable_single_gpu_call)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.nn_families import spread_pivots

pytestmark = pytest.mark.gpu


def _attn_oracle_bound(q, k, v, h, d, inject):
    """(oracle output, its parity bound) of the attention on device tensors (tests/test_kernels_gpu.py: attn_bound):
    what the split / fused forms of a sharded rank are held to -- the ORACLE, not another HIP launch."""
    from tests.test_kernels_gpu import attn_bound, attn_ref
    ref, ref_abs, _ = attn_ref(q.float().cpu(), k.float().cpu(), v.float().cpu(), h, d ** -0.5, inject, need_sigma=False)
    return ref, attn_bound(ref, ref_abs)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, K, inject, mode, no_split, ret, backend="gloo"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    hip_comm = None
    if backend == "nccl":        # RCCL: one GPU per rank
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    elif backend == "hip":       # exchanges through the C ABI (tf_comm_*); gloo only hands the unique id around
        torch.cuda.set_device(rank)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from tokenflow_amd.comm import HipComm
        uid = [HipComm.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        hip_comm = HipComm(uid[0], rank, world)
    else:                        # gloo: the ranks share cuda:0
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True      # the single-GPU reference in the bit-stable mode (TF_ATTN_NO_SPLIT): the claim under test
                                 # is "rank one-pass form == single GPU in that mode"; the default single-GPU mode
                                 # may split small grids (this toy size) or pick KW = 1 on large grids of small
                                 # frames (cfg2 level 2).  The sharded side follows FrameShard's own default

        n, S, h, d = 2, 320, 2, 40
        D = h * d
        h_ = h
        g = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(3 * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
        piv = spread_pivots(K, S, D, torch.bfloat16, g)[0].cuda()      # row norms differ: a misplaced inv_norm shows
        tgt = [(piv[c].float()[torch.randperm(S, generator=g).cuda()].repeat(n, 1)
                + 0.1 * torch.randn(n * S, D, generator=g).cuda()).bfloat16() for c in range(K)]
        res = [torch.randn(3 * n, S, D, generator=g).bfloat16().cuda() for _ in range(K)]
        s = torch.arange(0, n)
        w = torch.sigmoid(torch.abs(s + n - n // 2) / (torch.abs(s - n // 2) + torch.abs(s + n - n // 2))).cuda()
        # single-GPU reference
        full = ops.ext_attn(q, k, v, h, d ** -0.5, inject)
        inv = ops.pivot_inv_norm(piv)
        one = sharded.FrameShard.__new__(sharded.FrameShard)
        one.group, one.world, one.rank, one.K, one.Kl, one.kf0 = None, 1, 0, K, K, 0
        ref = [one.propagate(c, tgt[c], res[c], piv, inv, full, w, n) for c in range(K)]
        # sharded
        sh = sharded.FrameShard(K, comm=hip_comm) if no_split else sharded.FrameShard(K, comm=hip_comm, attn_split=True)
        assert sh.attn_split == (not no_split)
        Kl, f0 = sh.Kl, sh.kf0
        loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)
        out = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, inject, mode=mode)
        if no_split:     # same arithmetic per (query, head) whoever computes it
            ok = torch.equal(out, loc(full))
            slack = 0.0
        else:            # small grids take other kernels (key split inside the workgroup, merged): against the ORACLE,
            o_ref, o_bound = _attn_oracle_bound(q, k, v, h, d, inject)      # with the parity bound of the attention tests
            ok = bool(((out.float().cpu() - loc(o_ref)).abs() <= loc(o_bound)).all())
            # the propagation gathers rows of two attention outputs that are each within the bound of the oracle
            slack = 2.0 * float(o_bound.max())
        pe, ie, ke = sh.exchange_halo(piv[f0:f0 + Kl], inv[f0:f0 + Kl], out)

        def same(y, r):
            if no_split:
                return torch.equal(y, r)
            # same indices; gathered / blended rows of attention outputs within the bound, one fp32 -> 16-bit rounding
            return bool(((y.float() - r.float()).abs() <= 2.0 ** -8 * r.float().abs() + slack).all())
        for j in range(Kl):
            ok = ok and same(sh.propagate(j, tgt[f0 + j], res[f0 + j], pe, ie, ke, w, n), ref[f0 + j])
        # all local chunks in one call; halo in two halves with the first chunk deferred behind it
        tgt_all = torch.cat([tgt[f0 + j] for j in range(Kl)])
        res_all = torch.stack([res[f0 + j].view(3, n, S, D) for j in range(Kl)], dim=1).reshape(3 * Kl * n, S, D)
        want = torch.stack([ref[f0 + j].float().view(3, n, S, D) for j in range(Kl)], dim=1).reshape(3 * Kl * n, S, D)
        ok = ok and same(sh.propagate_all(tgt_all, res_all, pe, ie, ke, w, n), want)
        h = sh.halo_start(piv[f0:f0 + Kl], inv[f0:f0 + Kl])
        pe2, ie2, ke2, reqs = sh.halo_finish(h, out, wait=False)
        first, rest = sh.propagate_all(tgt_all, res_all, pe2, ie2, ke2, w, n, halo_reqs=reqs)
        ok = ok and same(first, ref[f0])
        if Kl > 1:
            ok = ok and same(rest, want.view(3, Kl, n, S, D)[:, 1:].reshape(3 * (Kl - 1) * n, S, D))
        # in-place form of the two-pass order (what bench.py runs at N > 1): producers write into the halo-extended
        # buffers, one grouped neighbour exchange per block, the propagation waits for it
        ext = sh.ext_alloc(S, D, torch.bfloat16, piv.device)
        o = 1 if world > 1 else 0
        ext[0][o:].copy_(piv[f0:f0 + Kl])
        ops.pivot_inv_norm(ext[0][o:], out=ext[1][o:])
        pe3, ie3, ke3, reqs = sh.pivotal_block(loc(q), loc(k), loc(v), h_, d ** -0.5, inject, ext, mode=mode)
        first, rest = sh.propagate_all(tgt_all, res_all, pe3, ie3, ke3, w, n, halo_reqs=reqs)
        ok = ok and same(first, ref[f0])
        if Kl > 1:
            ok = ok and same(rest, want.view(3, Kl, n, S, D)[:, 1:].reshape(3 * (Kl - 1) * n, S, D))
        got3 = ke3.view(3, Kl + o, S, D)[:, o:].reshape(3 * Kl, S, D)
        ok = ok and (torch.equal(got3, out) if no_split else same(got3, out))
        torch.cuda.synchronize()
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("K,mode,inject,no_split", [
    (4, "heads", False, True), (4, "heads", True, True), (4, "bank", False, True), (4, "bank", True, True),
    (5, "heads", True, True), (5, "heads", False, True), (5, "bank", False, True),
    # the split forms (oracle-bounded, not bit-equal): one case per exchange pattern and run shape -- every case is a
    # two-process spawn, and the full matrix was a minute of the GPU suite
    (4, "heads", False, False), (5, "heads", True, False), (4, "bank", True, False)])
def test_sharded_real_kernels_two_ranks(K, mode, inject, no_split):
    """K = 5: uneven runs (3 + 2 keyframes).  no_split = FrameShard's DEFAULT: one-pass attention, no environment
    switch -> bit-identical to the single-GPU run; attn_split=True: small grids split the bank over workgroups ->
    equal within the output rounding."""
    port = _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, port, K, inject, mode, no_split, ret), nprocs=2, join=True)
    assert dict(ret) == {0: True, 1: True}


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL refuses two ranks on one device)")
@pytest.mark.parametrize("backend", ["nccl", "hip"])
@pytest.mark.parametrize("K,mode,inject", [(4, "heads", False), (4, "heads", True), (5, "heads", True), (4, "bank", True),
                                           (5, "bank", False)])
def test_sharded_real_kernels_two_gpus_rccl(K, mode, inject, backend):
    """The same comparison with one GPU per rank over RCCL (xGMI): the all-to-alls of the head re-sharding, the bank
    all-gather and the grouped point-to-point halo on the real backend with a world of two -- through
    torch.distributed ("nccl") and through the library's own C-ABI exchange entry points ("hip")."""
    port = _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, port, K, inject, mode, True, ret, backend), nprocs=2, join=True)
    assert dict(ret) == {0: True, 1: True}


def _rccl_worker(rank, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        K, S, h, d = 3, 320, 2, 40
        g = torch.Generator().manual_seed(3)
        q, k, v = (torch.randn(3 * K, S, h * d, generator=g).bfloat16().cuda() for _ in range(3))
        sh = sharded.FrameShard(K)
        ok = True
        for inject in (False, True):
            full = ops.ext_attn(q, k, v, h, d ** -0.5, inject)
            out = sh._pivotal_heads(q, k, v, h, d ** -0.5, inject)      # the all-to-alls run through RCCL
            ok = ok and torch.equal(out, full)
            out = sh._pivotal_bank(q, k, v, h, d ** -0.5, inject)       # pack + all-gather through RCCL + one call
            ok = ok and torch.equal(out, full)
        pe, ie, ke = sh.exchange_halo(q[:K], torch.ones(K, S, device="cuda"), full)
        ok = ok and pe is q[:K] or pe.data_ptr() == q.data_ptr()
        torch.cuda.synchronize()
        ret[0] = bool(ok)
    finally:
        dist.destroy_process_group()


def test_head_exchange_through_rccl_single_rank():
    """The same torch.distributed calls the multi-GPU run makes (all_to_all_single with async_op, default splits),
    on the real backend: RCCL ("nccl") with a world of one GPU -- all the pool offers.  Catches API-level
    mistakes that the gloo tests cannot (argument forms, device tensors, stream ordering)."""
    port = _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_rccl_worker, args=(port, ret), nprocs=1, join=True)
    assert dict(ret) == {0: True}


# ---------------------------------------------------------------------------------------------------------------
# The C-ABI exchange steps (tf_comm_*, include/tokenflow_hip.h) through tokenflow_amd.comm: RCCL bound by dlopen.

def test_c_abi_comm_single_rank():
    """World of one on the real backend: every entry point runs (communicator, all-gather, row all-to-all, grouped
    send/recv with itself) and moves the bytes it should."""
    from tokenflow_amd import comm
    c = comm.HipComm(comm.HipComm.unique_id(), 0, 1)
    try:
        g = torch.Generator(device="cuda").manual_seed(3)
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            a = torch.randn(5, 64, 40, generator=g, device="cuda").to(dt)
            bank = torch.empty_like(a)
            assert torch.equal(c.allgather(a, bank), a)
            r = torch.empty_like(a)
            assert torch.equal(c.all_to_all_rows(a, r, [5], [5]), a)
            r2 = torch.empty_like(a)
            assert torch.equal(c.all_to_all_rows(a, r2), a)                 # equal parts
        s1, s2 = torch.randn(64, 320, generator=g, device="cuda").bfloat16(), torch.randn(64, generator=g, device="cuda").bfloat16()
        d1, d2 = torch.zeros_like(s1), torch.zeros_like(s2)
        c.sendrecv([s1, s2], 0, [d1, d2], 0)
        c.sendrecv([s1], -1, [d1], -1)                                       # both directions skipped: no-op
        torch.cuda.synchronize()
        assert torch.equal(d1, s1) and torch.equal(d2, s2)
        with pytest.raises(ValueError):
            c.all_to_all_rows(s1, torch.empty(3, 320, device="cuda", dtype=torch.bfloat16), [64], [2])
    finally:
        c.close()


def _comm_worker(rank, world, path, ret):
    import time
    from tokenflow_amd import comm
    torch.cuda.set_device(rank)
    if rank == 0:
        uid = comm.HipComm.unique_id()
        with open(path + ".tmp", "wb") as f:
            f.write(uid)
        os.replace(path + ".tmp", path)
    else:
        while not os.path.exists(path):
            time.sleep(0.01)
        uid = open(path, "rb").read()
    c = comm.HipComm(uid, rank, world)
    try:
        dev = torch.device("cuda", rank)
        S, D = 64, 80
        mine = torch.full((2, S, D), float(rank + 1), device=dev).bfloat16()
        bank = torch.empty(world * 2, S, D, device=dev, dtype=torch.bfloat16)
        c.allgather(mine, bank)
        ok = all(bool((bank[2 * r:2 * r + 2] == r + 1).all()) for r in range(world))
        # uneven rows: rank r sends (p + 1) rows to peer p, so it receives (r + 1) rows from everybody
        send_rows = [p + 1 for p in range(world)]
        recv_rows = [rank + 1] * world
        send = torch.cat([torch.full((p + 1, D), 10.0 * rank + p, device=dev) for p in range(world)]).bfloat16()
        recv = torch.empty(sum(recv_rows), D, device=dev, dtype=torch.bfloat16)
        c.all_to_all_rows(send, recv, send_rows, recv_rows)
        off = 0
        for p in range(world):
            ok = ok and bool((recv[off:off + rank + 1] == 10.0 * p + rank).all())
            off += rank + 1
        # halo: last keyframe to rank + 1, the left neighbour's from rank - 1
        halo = torch.zeros(S, D, device=dev, dtype=torch.bfloat16)
        c.sendrecv([mine[-1]], rank + 1 if rank + 1 < world else -1, [halo], rank - 1 if rank > 0 else -1)
        torch.cuda.synchronize()
        ok = ok and bool((halo == (rank if rank > 0 else 0)).all())
        ret[rank] = ok
    finally:
        c.close()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL refuses two ranks on one device)")
def test_c_abi_comm_two_gpus(tmp_path):
    ret = mp.get_context("spawn").Manager().dict()
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    mp.spawn(_comm_worker, args=(2, str(tmp_path / "uid"), ret), nprocs=2, join=True)
    assert ret[0] and ret[1]


def test_frame_shard_over_c_abi_comm_single_rank():
    """FrameShard on the C-ABI exchange entry points with a world of one (all the pool offers): the head re-sharding's
    two all-to-alls run through RCCL on the side stream, ordered against the compute stream with events.
    (Capturing these RCCL calls into a HIP graph was tried here and crashes inside hipStreamEndCapture with the RCCL
    2.26.6 of this PyTorch build, so no per-rank graph over the collectives is offered.)"""
    from tokenflow_amd import comm, ops, sharded
    c = comm.HipComm(comm.HipComm.unique_id(), 0, 1)
    old = ops.NO_SPLIT
    ops.NO_SPLIT = True
    try:
        K, S, h, d = 3, 320, 2, 40
        g = torch.Generator(device="cuda").manual_seed(5)
        q, k, v = (torch.randn(3 * K, S, h * d, generator=g, device="cuda").bfloat16() for _ in range(3))
        sh = sharded.FrameShard(K, comm=c)
        assert sh.world == 1 and sh.Kl == K
        for inject in (False, True):
            full = ops.ext_attn(q, k, v, h, d ** -0.5, inject)
            for _ in range(3):                                      # buffers are reused call after call
                out = sh._pivotal_heads(q, k, v, h, d ** -0.5, inject)
            torch.cuda.synchronize()
            assert torch.equal(out, full)
    finally:
        ops.NO_SPLIT = old
        c.close()


def _native_worker(rank, world, port, K, h, inject, mode, split, ret):
    """`NativeShard` (one tf_rank_pivotal call per block) on `world` processes sharing cuda:0, exchanges through the
    library's host-transport entry points carried by gloo (tests/gloo_transport.py)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        n, S, d = 2, 192, 40
        D = h * d
        g = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(3 * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
        piv = spread_pivots(K, S, D, torch.bfloat16, g)[0].cuda()      # row norms differ: a misplaced inv_norm shows
        tgt = [(piv[c].float()[torch.randperm(S, generator=g).cuda()].repeat(n, 1)
                + 0.1 * torch.randn(n * S, D, generator=g).cuda()).bfloat16() for c in range(K)]
        res = [torch.randn(3 * n, S, D, generator=g).bfloat16().cuda() for _ in range(K)]
        s = torch.arange(0, n)
        w = torch.sigmoid(torch.abs(s + n - n // 2) / (torch.abs(s - n // 2) + torch.abs(s + n - n // 2))).cuda()
        full = ops.ext_attn(q, k, v, h, d ** -0.5, inject)
        inv = ops.pivot_inv_norm(piv)
        one = sharded.FrameShard.__new__(sharded.FrameShard)
        one.group, one.world, one.rank, one.K, one.Kl, one.kf0 = None, 1, 0, K, K, 0
        ref = [one.propagate(c, tgt[c], res[c], piv, inv, full, w, n) for c in range(K)]

        comm, halo_comm = gloo_comm(rank, world), gloo_comm(rank, world)
        sh = sharded.NativeShard(K, comm, halo_comm, attn_split=split)
        py = sharded.FrameShard(K, comm=comm, attn_split=split)          # the Python form on the same transport
        Kl, f0 = sh.Kl, sh.kf0
        o = 1 if world > 1 else 0
        loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)
        tgt_all = torch.cat([tgt[f0 + j] for j in range(Kl)])
        res_all = torch.stack([res[f0 + j].view(3, n, S, D) for j in range(Kl)], dim=1).reshape(3 * Kl * n, S, D)
        want = torch.stack([ref[f0 + j].float().view(3, n, S, D) for j in range(Kl)], dim=1).reshape(3 * Kl * n, S, D)
        ok = True
        outs = []
        for shard in (sh, py):
            ext = shard.ext_alloc(S, D, torch.bfloat16, piv.device)
            for t in ext:
                t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).fill_(0x7fc0 if t.dtype == torch.bfloat16 else 0x7fc00000)  # NaN
            ext[0][o:].copy_(piv[f0:f0 + Kl])
            if shard is py:        # the native executor computes the inverse norms inside its pack launch (TF_RANK_INV_NORM)
                ops.pivot_inv_norm(ext[0][o:], out=ext[1][o:])
            pe, ie, ke, reqs = shard.pivotal_block(loc(q), loc(k), loc(v), h, d ** -0.5, inject, ext, mode=mode,
                                                   inv_norm=shard is sh)
            first, rest = shard.propagate_all(tgt_all, res_all, pe, ie, ke, w, n, halo_reqs=reqs)
            torch.cuda.synchronize()
            got = ke.view(3, Kl + o, S, D)[:, o:].reshape(3 * Kl, S, D)
            outs.append((got.clone(), pe.clone(), ie.clone(), ke.clone(), first.clone()))
            if not split:          # one-pass attention: the single-GPU result bit for bit
                ok = ok and torch.equal(got, loc(full)) and torch.equal(first, ref[f0])
                if Kl > 1:
                    ok = ok and torch.equal(rest, want.view(3, Kl, n, S, D)[:, 1:].reshape(3 * (Kl - 1) * n, S, D))
            else:                  # against the oracle with the attention tests' bound (not against another HIP launch)
                o_ref, o_bound = _attn_oracle_bound(q, k, v, h, d, inject)
                ok = ok and bool(((got.float().cpu() - loc(o_ref)).abs() <= loc(o_bound)).all())
            if rank > 0:           # the halo slot holds the left neighbour's last keyframe
                ok = ok and torch.equal(pe[0], piv[f0 - 1]) and torch.equal(ie[0], inv[f0 - 1])
                if not split:
                    ok = ok and torch.equal(ke.view(3, Kl + o, S, D)[:, 0], full.view(3, K, S, D)[:, f0 - 1])
        # the attention alone (TF_RANK_NO_HALO: what the hook path calls from attn1), strided q/k/v slabs of one buffer
        qkv = torch.cat([loc(q), loc(k), loc(v)], dim=-1)
        qs, ks, vs = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        a_n = sh.pivotal_attention(qs, ks, vs, h, d ** -0.5, inject, mode=mode)
        a_p = py.pivotal_attention(qs, ks, vs, h, d ** -0.5, inject, mode=mode)
        torch.cuda.synchronize()
        ok = ok and torch.equal(a_n, a_p) and (split or torch.equal(a_n, loc(full)))
        # native and Python forms: the same bits in every buffer they fill (the unset halo slot of rank 0 excluded)
        lo = 0 if rank > 0 else o
        (got_n, pe_n, ie_n, ke_n, first_n), (got_p, pe_p, ie_p, ke_p, first_p) = outs
        ok = ok and torch.equal(got_n, got_p) and torch.equal(first_n, first_p)
        ok = ok and torch.equal(pe_n[lo:], pe_p[lo:]) and torch.equal(ie_n[lo:], ie_p[lo:])
        ok = ok and torch.equal(ke_n.view(3, Kl + o, S, D)[:, lo:], ke_p.view(3, Kl + o, S, D)[:, lo:])
        sh.close()
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,K,h,mode,inject,split", [
    (2, 4, 2, "heads", False, False), (2, 4, 2, "heads", True, False), (2, 5, 2, "heads", True, False),
    (2, 5, 2, "bank", False, False), (2, 4, 2, "bank", True, False), (2, 4, 2, "heads", False, True),
    (8, 8, 8, "heads", False, False), (8, 8, 8, "heads", True, False), (8, 8, 8, "bank", True, False),
    (8, 25, 5, "bank", False, False), (8, 8, 8, None, False, True)])
def test_native_rank_executor(world, K, h, mode, inject, split):
    """tf_rank_pivotal (csrc/rank_exec.hip) through `NativeShard`: the whole pivotal pass of a block -- pack, both
    exchanges, source and bank attention, unpack, neighbour halo -- issued by one library call, on 2 and on 8
    processes sharing one GPU (BASELINE configs 3 and 5 at their own rank geometry: one keyframe per rank; runs of
    4,3,3,3,3,3,3,3 with 5 heads -> bank form).  Equal to the single-GPU result bit for bit in the one-pass form, and to
    the Python `FrameShard` on the same transport bit for bit in every form."""
    port = _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_native_worker, args=(world, port, K, h, inject, mode, split, ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}


def test_native_rank_executor_single_rank_and_loopback():
    """World of one (no communicator: plain attention into the extended buffer) and the wire-less loopback transport
    at 'rank 3 of 8' (results meaningless by construction; every launch, size check and stream hand-over runs)."""
    from tokenflow_amd import ops, sharded
    from tokenflow_amd.comm import HipComm
    K, S, h, d = 8, 256, 8, 40
    D = h * d
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(3 * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
    sh = sharded.NativeShard(K, None)
    ext = sh.ext_alloc(S, D, torch.bfloat16, q.device)
    for inject in (False, True):
        pe, ie, ke, reqs = sh.pivotal_block(q, k, v, h, d ** -0.5, inject, ext)
        assert reqs == [] and torch.equal(ke, ops.ext_attn(q, k, v, h, d ** -0.5, inject, no_split=True))
    sh.close()
    for mode in ("heads", "bank"):
        comm = HipComm.loopback(3, 8)
        sh = sharded.NativeShard(K, comm, attn_split=True)
        assert (sh.Kl, sh.kf0) == (1, 3)
        ext = sh.ext_alloc(S, D, torch.bfloat16, q.device)
        ext[0][1:].normal_()
        ops.pivot_inv_norm(ext[0][1:], out=ext[1][1:])
        ql, kl, vl = (t.view(3, K, S, D)[:, 3:4].reshape(3, S, D) for t in (q, k, v))
        for inject in (False, True):
            pe, ie, ke, reqs = sh.pivotal_block(ql, kl, vl, h, d ** -0.5, inject, ext, mode=mode)
            for r in reqs:
                r.wait()
        torch.cuda.synchronize()
        # the source branch never leaves the rank: exact whatever the transport
        want = ops.ext_attn(ql, kl, vl, h, d ** -0.5, False, part="source", no_split=True)
        assert torch.equal(ke.view(3, 2, S, D)[0, 1], want[0])
        sh.close()
        comm.close()


def test_loopback_transport_copies_switch():
    """tf_comm_init_loopback stands in for the wire with same-size local copies; tf_comm_loopback_copies(0) leaves the
    calls in place and moves nothing (the rank-step measurement with the stand-in copies excluded)."""
    from tokenflow_amd.comm import HipComm
    send = torch.arange(8 * 64, device="cuda", dtype=torch.float32).view(8, 64).bfloat16()
    for copies in (True, False):
        comm = HipComm.loopback(3, 8, copies=copies)
        recv = torch.zeros_like(send)
        comm.all_to_all_rows(send, recv)
        bank = torch.zeros(8, 64, device="cuda", dtype=torch.bfloat16)
        comm.allgather(send[:1], bank)
        got = [torch.zeros(64, device="cuda", dtype=torch.bfloat16)]
        comm.sendrecv([send[0]], 4, got, 2)
        torch.cuda.synchronize()
        moved = bool(recv.any()) or bool(bank.any()) or bool(got[0].any())
        assert moved == copies
        if copies:
            assert torch.equal(recv, send) and torch.equal(bank, send[:1].expand(8, 64)) and torch.equal(got[0], send[0])
        comm.close()


def test_loopback_wire_model_holds_the_stream():
    """tf_comm_loopback_wire (ABI 7): every exchange of a loopback communicator holds its stream for
    latency + bytes on the busiest link / bandwidth -- the executed stand-in for the wire of tools/rank_step_microbench.py
    --wire-model.  Data movement is unchanged; the model switches off again with (0, 0)."""
    from tokenflow_amd import _lib
    from tokenflow_amd.comm import HipComm
    send = torch.arange(8 * 4096, device="cuda", dtype=torch.float32).view(8, 4096).bfloat16()   # 8 KB per peer

    def timed(comm):
        recv = torch.zeros_like(send)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        comm.all_to_all_rows(send, recv)          # warm-up (module load of the hold kernel)
        torch.cuda.synchronize()
        e0.record()
        comm.all_to_all_rows(send, recv)
        e1.record()
        torch.cuda.synchronize()
        assert torch.equal(recv, send)
        return e0.elapsed_time(e1) * 1e3          # us

    comm = HipComm.loopback(3, 8, wire=(2000.0, 0.008))    # 2 ms latency + 8 KB on a link at 8 MB/s = 1 ms more
    t_wire = timed(comm)
    assert 2900.0 <= t_wire <= 10000.0, t_wire      # the hold is a LOWER bound; the upper one only catches a runaway
    _lib.check(_lib.load().tf_comm_loopback_wire(comm._h, 0.0, 0.0), "tf_comm_loopback_wire")
    assert timed(comm) < 2000.0
    # neighbour exchange: one link out, one link in -> max(sent, received) bytes
    _lib.check(_lib.load().tf_comm_loopback_wire(comm._h, 1000.0, 0.0), "tf_comm_loopback_wire")
    got = [torch.zeros(4096, device="cuda", dtype=torch.bfloat16)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    comm.sendrecv([send[0]], 4, got, 2)
    e1.record()
    torch.cuda.synchronize()
    assert torch.equal(got[0], send[0]) and 900.0 <= e0.elapsed_time(e1) * 1e3 <= 8000.0
    comm.close()
    plain = HipComm.loopback(0, 1)
    plain.close()


def _hooks_gpu_worker(rank, world, port, K, inject, native, ret):
    """The drop-in hooks sharded over ranks (register_frame_shard) with the REAL kernels under autocast: each rank's
    block outputs equal the one-process hooks' bit for bit."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import tokenflow_utils as tfu
        from tests import fake_diffusers as fd
        from tokenflow_amd import hooks, ops, sharded
        ops.NO_SPLIT = True      # the one-process reference of this toy size in its one-pass form (see _worker)
        n, S, D, h = 2, 192, 320, 8

        def make():
            torch.manual_seed(0)
            blk = fd.BasicTransformerBlock(D, h, cross_dim=32).eval()
            holder = torch.nn.Module()
            holder.unet = torch.nn.Module()
            holder.unet.blk = blk
            holder.cuda().bfloat16()
            blk.attn1.forward = hooks._make_sa_forward(blk.attn1, pnp=True)
            hooks._set_schedule(blk.attn1, [5])
            blk.attn1.t = 5 if inject else 7
            tfu.set_tokenflow(holder)
            return holder, blk
        g = torch.Generator().manual_seed(1)
        x_piv = torch.randn(3, K, S, D, generator=g).cuda().bfloat16()
        enc = torch.randn(3, K, 7, 32, generator=g).cuda().bfloat16()
        enc_n = torch.randn(3 * n, 7, 32, generator=g).cuda().bfloat16()
        chunks = []
        for c in range(K):
            perm = torch.randperm(S, generator=g)
            src = x_piv[0, c][perm][None].repeat(n, 1, 1)
            chunks.append(torch.cat([src, torch.randn(2 * n, S, D, generator=g).cuda().bfloat16()]))
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            holder, blk = make()
            tfu.register_pivotal(holder, True)
            piv_out = blk(x_piv.reshape(3 * K, S, D), encoder_hidden_states=enc.reshape(3 * K, 7, 32)).view(3, K, S, D)
            tfu.register_pivotal(holder, False)
            want = []
            for c in range(K):
                tfu.register_batch_idx(holder, c)
                want.append(blk(chunks[c], encoder_hidden_states=enc_n))
            if native:
                from tests.gloo_transport import gloo_comm
                sh = sharded.NativeShard(K, gloo_comm(rank, world))
            else:
                sh = sharded.FrameShard(K)
            holder, blk = make()
            tfu.register_frame_shard(holder, sh)
            lo, hi = sh.kf0, sh.kf0 + sh.Kl
            tfu.register_pivotal(holder, True)
            got_p = blk(x_piv[:, lo:hi].reshape(3 * sh.Kl, S, D),
                        encoder_hidden_states=enc[:, lo:hi].reshape(3 * sh.Kl, 7, 32)).view(3, sh.Kl, S, D)
            ok = torch.equal(got_p, piv_out[:, lo:hi])
            tfu.register_pivotal(holder, False)
            for c in range(lo, hi):
                tfu.register_batch_idx(holder, c)
                ok = ok and torch.equal(blk(chunks[c], encoder_hidden_states=enc_n), want[c])
        torch.cuda.synchronize()
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("K,inject,native", [(4, False, False), (5, True, False), (4, True, True)])
def test_hooks_sharded_real_kernels_two_ranks(K, inject, native):
    """`register_frame_shard` through the real kernels: 2 ranks sharing one GPU run the hook layer on their own
    keyframes and chunks (fused norm, fused QKV slabs read in place by the exchange, extended attention over the
    bank of all keyframes, propagation from the halo-extended caches); outputs equal the one-process hooks' bit for
    bit.  native: the same on `NativeShard` (its Python-level methods on the library's host transport)."""
    port = _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_hooks_gpu_worker, args=(2, port, K, inject, native, ret), nprocs=2, join=True)
    assert dict(ret) == {0: True, 1: True}


@pytest.mark.parametrize("K,S,h,d", [(8, 256, 8, 160), (8, 64, 8, 160), (8, 1024, 8, 80)])
@pytest.mark.parametrize("inject", [False, True])
def test_shard_vs_default_and_bit_stable_single_gpu_call(K, S, h, d, inject):
    """What "bit-identical to one GPU" means, pinned at the cfg2 level-2 / level-3 / level-1 shapes: a
    world-1 FrameShard (default: one-pass form) and a W = 8 rank's bank problems (q_frame subset through the same
    entry point) equal the single-GPU call with no_split=True bit for bit; against the single-GPU call in its DEFAULT
    mode (which may take KW = 1 on this large grid) they agree within the attention parity bound of the oracle."""
    from tokenflow_amd import ops, sharded
    D = h * d
    g = torch.Generator(device="cuda").manual_seed(7)
    q, k, v = (torch.randn(3 * K, S, D, generator=g, device="cuda").bfloat16() for _ in range(3))
    stable = ops.ext_attn(q, k, v, h, d ** -0.5, inject, no_split=True)
    default = ops.ext_attn(q, k, v, h, d ** -0.5, inject)
    sh = sharded.FrameShard(K)
    assert sh.world == 1 and not sh.attn_split
    assert torch.equal(sh.pivotal_attention(q, k, v, h, d ** -0.5, inject), stable)
    # one keyframe's queries against the whole bank, as a rank of 8 computes them (small grid)
    f = 3
    qf = q.view(3, K, S, D)[:, f:f + 1].reshape(3, S, D).contiguous()
    part = ops.ext_attn(qf, k, v, h, d ** -0.5, inject, q_frame0=f, no_split=True)
    assert torch.equal(part, stable.view(3, K, S, D)[:, f])
    ref, bound = _attn_oracle_bound(q, k, v, h, d, inject)
    for got in (stable, default):
        assert bool(((got.float().cpu() - ref).abs() <= bound).all())
