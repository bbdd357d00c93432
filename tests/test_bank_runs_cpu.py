"""The "bank_runs" exchange pattern of the pivotal pass on 2 and on 8 CPU processes (gloo): the host logic of
tokenflow_amd/sharded.py -- what is packed, which runs a rank computes and in which slot order -- with an oracle-backed
stand-in for the run and merge ops (per-run scores in torch, log-sum-exp merge in slot order).

The merge re-associates sums, so the yardstick is the oracle on the full tensors within the attention tolerance of
tests/test_oracle_golden.py (2e-6), not bit identity with the one-call form.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import tokenflow_oracle as orc
from tests.fake_ops import FakeOps
from tests.test_sharded_cpu import GlooComm, _data, _free_port

ATTN_TOL = 2e-6      # tests/test_oracle_golden.py: the attention tolerance between two fp32 evaluation orders


class RunsFakeOps(FakeOps):
    """FakeOps + the run form on the CPU.  A run call sees ONLY the views it is handed (its own frames, the branches the
    call may read); everything else of the bank is NaN while it computes, as FakeOps.ext_attn poisons what `part` may not
    read: a run that looked outside its frames or at a slab that was never sent would poison its result."""

    def head_pack(self, slabs, W, out=None):
        self.calls.append(("head_pack", len(slabs)))
        return super().head_pack(slabs, W, out=out)

    def ext_attn_runs_views(self, q, kv_runs, out, heads, scale, inject, runs, K, branch0=(0, 0), q_frame0=0,
                            streams=None, fold_scale=None, no_split=False, hints=0, order=None):
        self.calls.append(("ext_attn_runs", tuple(runs), bool(inject)))
        assert sorted(f for f0, n in runs for f in range(f0, f0 + n)) == list(range(K)), "runs must partition the bank"
        assert runs[0][0] <= q_frame0 and q_frame0 + q.shape[1] <= runs[0][0] + runs[0][1], "run 0 holds the query frames"
        Kq, S, D = q.shape[1:]
        d = D // heads
        qd = torch.full((3, Kq, S, D), float("nan"))
        qd[branch0[0]:branch0[0] + q.shape[0]] = self._r(q)
        parts = []      # per run: (O [2, Kq, heads, S, d], l [2, Kq, heads, S], m [2, Kq, heads, S])
        for r in (range(len(runs)) if order is None else order):
            f0, n = runs[r]
            kv, vv, kb0, vb0 = kv_runs[r]
            assert kv.shape[1] == n and vv.shape[1] == n
            kd = torch.full((3, K, S, D), float("nan"))
            vd = torch.full((3, K, S, D), float("nan"))
            kd[kb0:kb0 + kv.shape[0], f0:f0 + n] = self._r(kv)
            vd[vb0:vb0 + vv.shape[0], f0:f0 + n] = self._r(vv)
            O = torch.empty(2, Kq, heads, S, d)
            l = torch.empty(2, Kq, heads, S)
            m = torch.empty(2, Kq, heads, S)
            for b in (1, 2):
                bq = 0 if inject else b
                keys = kd[bq, f0:f0 + n].reshape(n * S, heads, d)
                vals = vd[b, f0:f0 + n].reshape(n * S, heads, d)
                for f in range(Kq):
                    s = torch.einsum("qhc,khc->hqk", qd[bq, f].view(S, heads, d), keys) * scale
                    m[b - 1, f] = s.amax(-1)
                    p = torch.exp(s - m[b - 1, f][..., None])
                    l[b - 1, f] = p.sum(-1)
                    O[b - 1, f] = torch.einsum("hqk,khc->hqc", p, vals)
            parts.append((r, O, l, m))
            if r == 0:      # the source branch of the query frames: final, from the local run
                for f in range(Kq):
                    fb = q_frame0 + f
                    s = torch.einsum("qhc,khc->hqk", qd[0, f].view(S, heads, d), kd[0, fb].view(S, heads, d)) * scale
                    o = torch.einsum("hqk,khc->hqc", torch.softmax(s, -1), vd[0, fb].view(S, heads, d))
                    out[0 - branch0[1], f] = self._r(o.permute(1, 0, 2).reshape(S, D)).to(out.dtype)
        parts.sort(key=lambda t: t[0])      # the merge reduces in SLOT order, whatever the issue order
        M = torch.stack([p[3] for p in parts]).amax(0)
        num = torch.zeros_like(parts[0][1])
        den = torch.zeros_like(parts[0][2])
        for _, O, l, m in parts:
            w = torch.exp(m - M)
            num += O * w[..., None]
            den += l * w
        res = (num / den[..., None]).permute(0, 1, 3, 2, 4).reshape(2, Kq, S, D)
        for b in (1, 2):
            out[b - branch0[1]] = self._r(res[b - 1]).to(out.dtype)
        return out


def _worker(rank, world, port, K, S, h, d, inject, use_comm, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tokenflow_amd import sharded
        fake = RunsFakeOps()
        sharded.ops = fake
        q, k, v, piv, *_ = _data(K, 1, S, h, d, seed=3)
        D = h * d
        ref = orc.ext_attn_core(q, k, v, h, d ** -0.5, inject)
        sh = sharded.FrameShard(K, comm=GlooComm() if use_comm else None)
        Kl, f0 = sh.Kl, sh.kf0
        loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)   # noqa: E731
        runs = sh.bank_runs_of_rank()
        msgs = []
        # the rank's runs: local first, then left, then right; they partition the bank
        want_runs = [(f0, Kl)] + ([(0, f0)] if f0 else []) + ([(f0 + Kl, K - f0 - Kl)] if f0 + Kl < K else [])
        if runs != want_runs:
            msgs.append(f"runs {runs} != {want_runs}")
        out = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, inject, mode="bank_runs")
        err = float((out - loc(ref)).abs().max())
        if not err <= ATTN_TOL:
            msgs.append(f"pivotal_attention: max abs err {err:.3e} (NaN = a run read outside its frames / slabs)")
        packs = [c[1] for c in fake.calls if c[0] == "head_pack"]
        if packs != [3 if inject else 4]:
            msgs.append(f"packed slabs {packs}")
        if [c for c in fake.calls if c[0] == "ext_attn_runs"] != [("ext_attn_runs", tuple(want_runs), inject)]:
            msgs.append(f"calls {fake.calls}")
        if any(c[0] == "ext_attn" for c in fake.calls):
            msgs.append("the one-call attention ran in bank_runs mode")
        # the in-place form: output into the halo-extended buffer, halo slot from the left neighbour
        ext = sh.ext_alloc(S, D, q.dtype, q.device)
        o = 1 if world > 1 else 0
        ext[0][o:].copy_(piv[f0:f0 + Kl])
        ext[2].fill_(float("nan"))
        pe, ie, ke, reqs = sh.pivotal_block(loc(q), loc(k), loc(v), h, d ** -0.5, inject, ext, mode="bank_runs", inv_norm=True)
        sh.halo_wait(reqs)
        ke4 = ke.view(3, Kl + o, S, D)
        err = float((ke4[:, o:].reshape(3 * Kl, S, D) - loc(ref)).abs().max())
        if not err <= ATTN_TOL:
            msgs.append(f"pivotal_block: max abs err {err:.3e}")
        if rank > 0:
            left = ref.view(3, K, S, D)[:, f0 - 1]
            if not (torch.equal(pe[0], piv[f0 - 1]) and float((ke4[:, 0] - left).abs().max()) <= ATTN_TOL):
                msgs.append("halo slot")
        # opt-in auto_mode through mode=None: this toy S is below the threshold -> today's answer runs
        sh2 = sharded.FrameShard(K, comm=GlooComm() if use_comm else None, bank_runs=True)
        fake.calls.clear()
        sh2.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, inject)
        if any(c[0] == "ext_attn_runs" for c in fake.calls):
            msgs.append("auto_mode took bank_runs below BANK_RUNS_MIN_S")
        ret[rank] = "; ".join(msgs)
    finally:
        dist.destroy_process_group()


def _spawn(world, K, S, h, d, inject, use_comm=False):
    port = _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, K, S, h, d, inject, use_comm, ret), nprocs=world, join=True)
    assert dict(ret) == {r: "" for r in range(world)}


@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("K", [4, 5])
def test_world2_even_and_uneven(K, inject):
    _spawn(2, K, 12, 2, 8, inject)


@pytest.mark.parametrize("inject", [False, True])
def test_world2_over_comm_interface(inject):
    _spawn(2, 5, 12, 3, 8, inject, use_comm=True)


@pytest.mark.parametrize("K,h", [(8, 8), (25, 5)])
@pytest.mark.parametrize("inject", [False, True])
def test_world8_baseline_geometries(K, h, inject):
    """BASELINE configs 3 (K = 8: one keyframe per rank) and 5 (K = 25: runs of 4,3,3,3,3,3,3,3; 5 heads do not divide
    over 8 ranks) at their rank geometry, toy token counts."""
    _spawn(8, K, 6, h, 8, inject)


def _shard(world, bank_runs, monkeypatch=None, env=None):
    from tokenflow_amd import sharded
    if monkeypatch is not None:
        if env is None:
            monkeypatch.delenv("TOKENFLOW_SHARD_BANK_RUNS", raising=False)
        else:
            monkeypatch.setenv("TOKENFLOW_SHARD_BANK_RUNS", env)
    sh = sharded.FrameShard(max(world, 1), bank_runs=bank_runs)
    sh.world = world       # auto_mode reads nothing else
    return sh


def test_auto_mode_defaults_unchanged(monkeypatch):
    """Without the opt-in the answers are today's, at every level and head count."""
    for world in (2, 8):
        sh = _shard(world, None, monkeypatch)
        assert not sh.bank_runs
        for heads in (5, 8, 10, 16, 20):
            for S in (16, 64, 256, 1024, 4096, 9216):
                want = "bank" if (heads % world or S <= 64) else "heads"
                assert sh.auto_mode(heads, S) == want, (world, heads, S)


@pytest.mark.parametrize("how", ["arg", "env"])
def test_auto_mode_opt_in(monkeypatch, how):
    from tokenflow_amd import sharded
    sh = _shard(8, True, monkeypatch) if how == "arg" else _shard(8, None, monkeypatch, env="1")
    assert sh.bank_runs and sharded.FrameShard.BANK_RUNS_MIN_S == 1024
    for heads in (5, 10, 20):                       # cfg5: the heads never divide over 8 ranks
        assert sh.auto_mode(heads, 4096) == "bank_runs" and sh.auto_mode(heads, 1024) == "bank_runs"
        assert sh.auto_mode(heads, 256) == "bank" and sh.auto_mode(heads, 64) == "bank"
    for S in (64, 256, 1024, 4096):                 # where the heads divide, the heads form stays (mid block: bank)
        assert sh.auto_mode(8, S) == ("bank" if S <= 64 else "heads")
    assert not _shard(8, False, monkeypatch, env="1").bank_runs     # the argument wins over the environment
