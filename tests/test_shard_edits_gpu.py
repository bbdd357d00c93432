"""Multi-edit batches on a frame shard with the REAL HIP ops: 2 ranks sharing cuda:0 over gloo (the pattern and sizes of
tests/test_sharded_gpu.py::test_sharded_real_kernels_two_ranks).

Identity under test, in FrameShard's default one-pass form: a rank's slices for edit e equal, bit for bit, the
single-process `ops.ext_attn_edits(..., no_split=True, multi_v=False, inject_mask=m)` slices -- and with them the sharded
single-edit pass on [source | uncond_e | cond_e], which test_sharded_gpu.py holds to the single-edit call -- for the
attention, `pivotal_block`'s in-place state and `propagate_all` with the deferred halo.  With attn_split=True the small
grid of a rank takes other launch plans: held to the ORACLE's attention bound, every edit with its own flag."""
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


def _worker(rank, world, port, K, mode, E, mask, S, d, no_split, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
    try:
        from tokenflow_amd import ops, sharded
        n, h = 2, 2
        B, D = 1 + 2 * E, h * d
        g = torch.Generator().manual_seed(E * 16 + mask)
        q, k, v = (torch.randn(B * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
        piv = spread_pivots(K, S, D, torch.bfloat16, g)[0].cuda()      # row norms differ: a misplaced inv_norm shows
        tgt = [(piv[c].float()[torch.randperm(S, generator=g).cuda()].repeat(n, 1)
                + 0.1 * torch.randn(n * S, D, generator=g).cuda()).bfloat16() for c in range(K)]
        res = [torch.randn(B * n, S, D, generator=g).bfloat16().cuda() for _ in range(K)]
        s = torch.arange(0, n)
        w = torch.sigmoid(torch.abs(s + n - n // 2) / (torch.abs(s - n // 2) + torch.abs(s + n - n // 2))).cuda()
        bad = []
        # ---- single process, bit-stable mode, four-bank form off
        full = ops.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, no_split=True, multi_v=False, inject_mask=mask)
        inv = ops.pivot_inv_norm(piv)
        ref = [ops.propagate_chunks_edits(tgt[c], piv, inv, full, None if c == 0 else w, n, 1, c, c == 0, res[c],
                                          torch.float32 if c else torch.bfloat16, E) for c in range(K)]
        # ---- this rank
        sh = sharded.FrameShard(K) if no_split else sharded.FrameShard(K, attn_split=True)
        Kl, f0 = sh.Kl, sh.kf0
        loc = lambda t: t.view(B, K, S, D)[:, f0:f0 + Kl].reshape(B * Kl, S, D)
        out = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, False, mode=mode, n_edits=E, inject_mask=mask)
        if not no_split:
            from tests.test_kernels_gpu import attn_bound, attn_ref
            worst = 0.0
            for e in range(E):       # every edit against the oracle on [source | uncond_e | cond_e] with ITS flag
                sl = [0, 1 + 2 * e, 2 + 2 * e]
                q3, k3, v3 = (t.view(B, K, S, D)[sl].reshape(3 * K, S, D).float().cpu() for t in (q, k, v))
                r, r_abs, _ = attn_ref(q3, k3, v3, h, d ** -0.5, bool((mask >> e) & 1), need_sigma=False)
                pick = lambda x: x.view(3, K, S, D)[:, f0:f0 + Kl]
                err = (out.view(B, Kl, S, D)[sl].float().cpu() - pick(r)).abs()
                worst = max(worst, float((err - attn_bound(pick(r), pick(r_abs))).max()))
            print(f"rank {rank}: attn_split, worst excess over the attention bound {worst:.3e}")
            if worst > 0:
                bad.append(f"attention exceeds the oracle bound by {worst:.3e}")
            torch.cuda.synchronize()
            ret[rank] = bad
            return
        if not torch.equal(out, loc(full)):
            bad.append("attention")
        # ---- in-place two-pass form: state written by the attention, one grouped exchange, first chunk deferred
        o = 1
        ext = sh.ext_alloc(S, D, torch.bfloat16, piv.device, n_edits=E)
        ext[0][o:].copy_(piv[f0:f0 + Kl])
        pe, ie, ke, reqs = sh.pivotal_block(loc(q), loc(k), loc(v), h, d ** -0.5, False, ext, mode=mode, inv_norm=True,
                                            n_edits=E, inject_mask=mask)
        if not torch.equal(ke.view(B, Kl + o, S, D)[:, o:].reshape(B * Kl, S, D), loc(full)):
            bad.append("pivotal_block state")
        tgt_all = torch.cat([tgt[f0 + j] for j in range(Kl)])
        res_all = torch.stack([res[f0 + j].view(B, n, S, D) for j in range(Kl)], dim=1).reshape(B * Kl * n, S, D)
        first, rest = sh.propagate_all(tgt_all, res_all, pe, ie, ke, w, n, halo_reqs=reqs, n_edits=E)
        if not torch.equal(first, ref[f0]):
            bad.append("deferred first chunk")
        for j in range(1, Kl):
            if not torch.equal(rest.view(B, Kl - 1, n, S, D)[:, j - 1].reshape(B * n, S, D), ref[f0 + j]):
                bad.append(f"chunk {f0 + j}")
        if rank > 0 and not torch.equal(ke.view(B, Kl + o, S, D)[:, 0], full.view(B, K, S, D)[:, f0 - 1]):
            bad.append("halo slot")
        torch.cuda.synchronize()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001  (reported once, through the shared dict; nothing is retried)
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("K,mode,E,mask,S,d,no_split", [
    (4, "heads", 2, 0b11, 320, 40, True),
    (5, "heads", 3, 0b101, 320, 40, True),      # uneven runs (3 + 2 keyframes), a mixed mask: compact q / k on the wire
    (4, "bank", 2, 0b00, 320, 40, True),
    (5, "bank", 3, 0b010, 320, 40, True),
    (4, "heads", 2, 0b01, 64, 160, True),       # the fused regime: the bank part of both edits in ONE launch
    (4, "heads", 3, 0b101, 320, 40, False)])    # attn_split=True: against the oracle bound
def test_two_ranks_real_kernels(K, mode, E, mask, S, d, no_split):
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), K, mode, E, mask, S, d, no_split, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)
