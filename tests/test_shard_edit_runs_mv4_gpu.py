"""The four-bank run launches on a frame shard (`edit_runs_multi_v=True` on top of `edit_runs=True`): 2 ranks on one MI355X,
exchanges carried by gloo (tests/gloo_transport.py), as tests/test_shard_edit_runs_gpu.py runs them.

Guarantee under test: `FrameShard(edit_runs=True, edit_runs_multi_v=True)` and `NativeEditShard` with the same opt-in (the
executor hands TF_ATTN_RUN_MULTI_V to the local run, the remote runs and the merge) fill the attention output with the same
bits, which are those of the single-process `ops.ext_attn_runs_edits(..., multi_v=True)` over the rank's runs, and every edit
equals the oracle on [source | uncond_e | cond_e] within the attention bound.  Without the opt-in the bits are those of the
flag-less call.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.nn_families import spread_pivots
from tests.test_bank_runs_gpu import _runs_of
from tests.test_shard_edit_runs_gpu import TIMEOUT, _nan_fill
from tests.test_sharded_gpu import _free_port

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, K, h, S, d, E, masks, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("TOKENFLOW_SHARD_EDIT_RUNS_MULTI_V", None)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
    try:
        from tests.gloo_transport import gloo_comm
        from tests.test_kernels_gpu import attn_bound, attn_ref
        from tokenflow_amd import ops, sharded
        B, D = 1 + 2 * E, h * d
        scale = d ** -0.5
        g = torch.Generator().manual_seed(11 + K + S)
        q, k, v = (torch.randn(B * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
        piv = spread_pivots(K, S, D, torch.bfloat16, g)[0].cuda()      # row norms differ: a misplaced inv_norm shows
        comm, halo_comm = gloo_comm(rank, world), gloo_comm(rank, world)
        shards = {
            ("native", True): sharded.NativeEditShard(K, comm, halo_comm, edit_runs=True, edit_runs_multi_v=True),
            ("python", True): sharded.FrameShard(K, comm=comm, edit_runs=True, edit_runs_multi_v=True),
            ("native", False): sharded.NativeEditShard(K, comm, halo_comm, edit_runs=True),
            ("python", False): sharded.FrameShard(K, comm=comm, edit_runs=True),
        }
        f0, Kl, runs = _runs_of(K, world, rank)
        o = 1
        msgs = []
        loc = lambda t: t.view(B, K, S, D)[:, f0:f0 + Kl].reshape(B * Kl, S, D)   # noqa: E731
        refs = {}
        for e in range(E):
            sl = [0, 1 + 2 * e, 2 + 2 * e]
            q3, k3, v3 = (t.view(B, K, S, D)[sl].reshape(3 * K, S, D).float().cpu() for t in (q, k, v))
            for inj in sorted({bool((m >> e) & 1) for m in masks}):
                r, r_abs, _ = attn_ref(q3, k3, v3, h, scale, inj, need_sigma=False)
                pick = lambda x: x.view(3, K, S, D)[:, f0:f0 + Kl]   # noqa: E731
                refs[e, inj] = (pick(r), attn_bound(pick(r), pick(r_abs)))
        for mask in masks:
            one = {mv: ops.ext_attn_runs_edits(loc(q).contiguous(), k, v, h, scale, E, mask, runs, q_frame0=f0, no_split=True,
                                               multi_v=mv) for mv in (True, False)}
            n_inj = bin(mask).count("1")
            if (n_inj >= 2) == torch.equal(one[True], one[False]):
                msgs.append(f"mask {mask:#b}: the flag {'changed nothing' if n_inj >= 2 else 'changed a call with no pair'}")
            for (name, mv), shard in shards.items():
                what = f"mask {mask:#b} {name} multi_v={mv}"
                ext = shard.ext_alloc(S, D, torch.bfloat16, piv.device, n_edits=E)
                for t in ext:
                    _nan_fill(t)
                for b in getattr(shard, "_news", {}).values():   # the native executor's workspace, partial results included
                    b.fill_(0xFF)
                ext[0][o:].copy_(piv[f0:f0 + Kl])
                pe, ie, ke, reqs = shard.pivotal_block(loc(q), loc(k), loc(v), h, scale, False, ext, mode="bank_runs",
                                                       inv_norm=True, n_edits=E, inject_mask=mask)
                shard.halo_wait(reqs)
                torch.cuda.synchronize()
                dist.barrier()
                got = ke.view(B, Kl + o, S, D)[:, o:].reshape(B * Kl, S, D)
                if not torch.equal(got, one[mv]):
                    msgs.append(f"{what}: differs from single-process ext_attn_runs_edits "
                                f"({float((got.float() - one[mv].float()).abs().max()):.3e})")
                for e in range(E):
                    r, bound = refs[e, bool((mask >> e) & 1)]
                    err = (got.view(B, Kl, S, D)[[0, 1 + 2 * e, 2 + 2 * e]].float().cpu() - r).abs()
                    if not bool((err <= bound).all()):
                        msgs.append(f"{what}: edit {e} outside the oracle bound by {float((err - bound).max()):.3e}")
                # the attention alone (TF_RANK_NO_HALO: what the hook path calls from attn1)
                a = shard.pivotal_attention(loc(q), loc(k), loc(v), h, scale, False, mode="bank_runs", n_edits=E,
                                            inject_mask=mask)
                torch.cuda.synchronize()
                if not torch.equal(a, one[mv]):
                    msgs.append(f"{what}: pivotal_attention")
        for (name, mv), shard in shards.items():
            if name == "native":
                shard.close()
        ret[rank] = msgs
    except Exception as e:      # noqa: BLE001  (reported once, through the shared dict; nothing is retried)
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("K,h,S,d,E,masks", [
    (5, 2, 256, 40, 2, (0b11, 0b01)),          # uneven runs (3 + 2); all / mixed
    (5, 2, 256, 64, 3, (0b111, 0b101)),        # a pair beside an odd edit; a pair around an edit that does not inject
    (5, 5, 320, 64, 2, (0b11,))])              # five heads: the case in which the heads do not divide over the ranks
def test_native_python_and_single_process_agree(K, h, S, d, E, masks):
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), K, h, S, d, E, masks, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)
