"""The "bank_runs" exchange pattern for multi-edit batches on an MI355X: `NativeEditShard(edit_runs=True)`
(tf_rank_pivotal_edits, TF_RANK_BANK_EDIT_RUNS) and the Python `FrameShard(edit_runs=True)` on processes sharing one GPU,
exchanges carried by gloo (tests/gloo_transport.py) -- tests/test_bank_runs_gpu.py crossed with tests/test_native_edits_gpu.py.

Guarantee under test: both fill every buffer with the same bits; both equal, bit for bit, the single-process
`ops.ext_attn_runs_edits` with the rank's runs, and every edit the oracle on [source | uncond_e | cond_e] with its own flag
within the attention bound -- not the bit-stable one-call form.
"""
import datetime
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.nn_families import spread_pivots
from tests.test_bank_runs_gpu import _runs_of
from tests.test_sharded_gpu import _free_port

pytestmark = pytest.mark.gpu

TIMEOUT = datetime.timedelta(seconds=60)      # a rank that fails early ends the test instead of hanging its peer


def _nan_fill(t):
    t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).fill_(0x7fc0 if t.dtype == torch.bfloat16 else 0x7fc00000)


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


def _worker(rank, world, port, K, h, S, d, E, masks, ret):
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tests.test_kernels_gpu import attn_bound, attn_ref
        from tokenflow_amd import ops, sharded
        B, D = 1 + 2 * E, h * d
        scale = d ** -0.5
        g = torch.Generator().manual_seed(7 + K + S)
        q, k, v = (torch.randn(B * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
        piv = spread_pivots(K, S, D, torch.bfloat16, g)[0].cuda()      # row norms differ: a misplaced inv_norm shows
        inv = ops.pivot_inv_norm(piv)
        comm, halo_comm = gloo_comm(rank, world), gloo_comm(rank, world)
        sh = sharded.NativeEditShard(K, comm, halo_comm, edit_runs=True)
        py = sharded.FrameShard(K, comm=comm, edit_runs=True)      # the Python form on the same transport
        Kl, f0, o = sh.Kl, sh.kf0, 1
        f0_, Kl_, runs = _runs_of(K, world, rank)
        msgs = []
        if (f0_, Kl_) != (f0, Kl) or py.bank_runs_of_rank() != runs:
            msgs.append(f"runs {py.bank_runs_of_rank()} != {runs}")
        loc = lambda t: t.view(B, K, S, D)[:, f0:f0 + Kl].reshape(B * Kl, S, D)   # noqa: E731
        # the oracle per edit and injection state, on the rows of this rank's frames
        refs = {}
        for e in range(E):
            sl = [0, 1 + 2 * e, 2 + 2 * e]
            q3, k3, v3 = (t.view(B, K, S, D)[sl].reshape(3 * K, S, D).float().cpu() for t in (q, k, v))
            for inj in sorted({bool((m >> e) & 1) for m in masks}):
                r, r_abs, _ = attn_ref(q3, k3, v3, h, scale, inj, need_sigma=False)
                pick = lambda x: x.view(3, K, S, D)[:, f0:f0 + Kl]   # noqa: E731
                refs[e, inj] = (pick(r), attn_bound(pick(r), pick(r_abs)))
        for mask in masks:
            # single-process reference: the same runs over the full tensors (one-pass runs: the shards' default)
            one = ops.ext_attn_runs_edits(loc(q).contiguous(), k, v, h, scale, E, mask, runs, q_frame0=f0, no_split=True)
            if rank > 0:      # what the left neighbour sends: the last keyframe of ITS run set
                fl, Kll, runs_l = _runs_of(K, world, rank - 1)
                ql = q.view(B, K, S, D)[:, fl:fl + Kll].reshape(B * Kll, S, D).contiguous()
                left = ops.ext_attn_runs_edits(ql, k, v, h, scale, E, mask, runs_l, q_frame0=fl,
                                               no_split=True).view(B, Kll, S, D)[:, -1]
            outs = []
            for shard in (sh, py):
                name = f"mask {mask:#b} " + ("native" if shard is sh else "python")
                ext = shard.ext_alloc(S, D, torch.bfloat16, piv.device, n_edits=E)
                for t in ext:
                    _nan_fill(t)
                for b in shard._bufs.values():                  # send / receive buffers of the Python host
                    _nan_fill(b)
                for b in getattr(shard, "_news", {}).values():  # the native executor's workspace: exchange buffers, V^T image,
                    b.fill_(0xFF)                               # norm table, slot counts, partial results
                ext[0][o:].copy_(piv[f0:f0 + Kl])
                pe, ie, ke, reqs = shard.pivotal_block(loc(q), loc(k), loc(v), h, scale, False, ext, mode="bank_runs",
                                                       inv_norm=True, n_edits=E, inject_mask=mask)
                shard.halo_wait(reqs)
                torch.cuda.synchronize()
                dist.barrier()
                ke4 = ke.view(B, Kl + o, S, D)
                got = ke4[:, o:].reshape(B * Kl, S, D)
                if not torch.equal(got, one):
                    msgs.append(f"{name}: differs from single-process ext_attn_runs_edits "
                                f"({float((got.float() - one.float()).abs().max()):.3e})")
                for e in range(E):
                    r, bound = refs[e, bool((mask >> e) & 1)]
                    err = (got.view(B, Kl, S, D)[[0, 1 + 2 * e, 2 + 2 * e]].float().cpu() - r).abs()
                    if not bool((err <= bound).all()):
                        msgs.append(f"{name}: edit {e} outside the oracle bound by {float((err - bound).max()):.3e}")
                if not (torch.equal(pe[o:], piv[f0:f0 + Kl]) and torch.equal(ie[o:], inv[f0:f0 + Kl])):
                    msgs.append(f"{name}: local pivots / inverse norms")
                if rank > 0 and not (torch.equal(pe[0], piv[f0 - 1]) and torch.equal(ie[0], inv[f0 - 1])
                                     and torch.equal(ke4[:, 0], left)):
                    msgs.append(f"{name}: halo slot")
                outs.append((pe.clone(), ie.clone(), ke4.clone()))
            # the attention alone (TF_RANK_NO_HALO: what the hook path calls from attn1), strided q/k/v slabs of one buffer
            qkv = torch.cat([loc(q), loc(k), loc(v)], dim=-1)
            qs, ks, vs = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
            a_n = sh.pivotal_attention(qs, ks, vs, h, scale, False, mode="bank_runs", n_edits=E, inject_mask=mask)
            a_p = py.pivotal_attention(qs, ks, vs, h, scale, False, mode="bank_runs", n_edits=E, inject_mask=mask)
            torch.cuda.synchronize()
            if not (torch.equal(a_n, one) and torch.equal(a_p, one)):
                msgs.append(f"mask {mask:#b}: pivotal_attention on strided slabs")
            lo = 0 if rank > 0 else o       # (the unset halo slot of rank 0 excluded)
            (pe_n, ie_n, ke_n), (pe_p, ie_p, ke_p) = outs
            if not (torch.equal(pe_n[lo:], pe_p[lo:]) and torch.equal(ie_n[lo:], ie_p[lo:])
                    and torch.equal(ke_n[:, lo:], ke_p[:, lo:])):
                msgs.append(f"mask {mask:#b}: native != python")
        if rank == 0:      # without the opt-in the explicit mode keeps raising, on both classes
            plain = sharded.NativeEditShard(K, comm)
            for shard in (plain, sharded.FrameShard(K, comm=comm)):
                try:
                    shard.pivotal_attention(loc(q), loc(k), loc(v), h, scale, False, mode="bank_runs", n_edits=E, inject_mask=0)
                    msgs.append("bank_runs with several edits ran without the opt-in")
                except ValueError as e:
                    if "edit_runs" not in str(e):
                        msgs.append(f"refusal text: {e}")
            plain.close()
        sh.close()
        ret[rank] = msgs
    except Exception as e:      # noqa: BLE001  (reported once, through the shared dict; nothing is retried)
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,K,h,S,d", [
    (2, 5, 2, 192, 40),        # uneven runs (3 + 2), the one-tile kernels
    (2, 5, 5, 320, 64),        # five heads, DUAL and ALL run launches at head dim 64
    (8, 8, 2, 192, 40)])       # one keyframe per rank: three runs on the inner ranks
def test_native_python_and_single_process_agree(world, K, h, S, d):
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), K, h, S, d, 2, (0b00, 0b11, 0b01), ret), nprocs=world, join=True)
    assert dict(ret) == {r: [] for r in range(world)}, dict(ret)


def _hooks_worker(rank, world, port, K, ret):
    """`register_frame_shard` + `register_edits` + `register_edit_schedules` with schedules that disagree at the step under
    test, on the small fake pipeline with the REAL kernels under autocast, the shards' `auto_mode` answering "bank_runs" (the
    answer is planted: the toy frames are shorter than its threshold): `NativeEditShard` and `FrameShard` with the opt-in give
    the same block outputs bit for bit, and `ops.ext_attn_runs_edits_views` saw the mixed mask."""
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
        native = sharded.NativeEditShard(K, comm, bank_runs=True, edit_runs=True)
        python = sharded.FrameShard(K, comm=comm, bank_runs=True, edit_runs=True)
        seen = []
        views = ops.ext_attn_runs_edits_views
        ops.ext_attn_runs_edits_views = lambda *a, **kw: (seen.append(a[6]), views(*a, **kw))[1]
        outs = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for shard in (native, python):
                shard.auto_mode = lambda heads, S_, n_edits=1: "bank_runs"
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
        ops.ext_attn_runs_edits_views = views
        bad = [f"block output {i}" for i, (a, b) in enumerate(zip(*outs)) if not torch.equal(a, b)]
        if any(bool(torch.isnan(a).any()) for a in outs[0]):
            bad.append("NaN in a block output")
        if seen != [0b01]:
            bad.append(f"masks at the Python shard's run form: {seen}")
        native.close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_hooks_two_ranks_schedules_that_disagree():
    ret = mp.Manager().dict()
    mp.spawn(_hooks_worker, args=(2, _free_port(), 4, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)
