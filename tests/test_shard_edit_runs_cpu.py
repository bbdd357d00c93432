"""The "bank_runs" exchange pattern for multi-edit batches (`FrameShard(K, edit_runs=True)`) on 2 and on 8 CPU processes
(gloo): the host logic of tokenflow_amd/sharded.py with the oracle-backed ops of tests/shard_edit_runs_ops.py.

The merge re-associates sums, so the yardstick of the attention is the single-process oracle per edit within the attention
tolerance between two fp32 evaluation orders (tests/test_oracle_golden.py, 2e-6), as in tests/test_bank_runs_cpu.py; NaN = a
run read outside its frames, a slab that was never sent, or another edit's slot."""
import datetime
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_bank_runs_cpu import ATTN_TOL
from tests.test_shard_edits_cpu import _data
from tests.test_sharded_cpu import GlooComm, _free_port

TIMEOUT = datetime.timedelta(seconds=60)      # a rank that fails early ends the test instead of hanging its peer
CASES = [(2, 0b00), (2, 0b11), (2, 0b01), (3, 0b000), (3, 0b111), (3, 0b101), (3, 0b010)]


def _worker(rank, world, port, K, h, use_comm, cases, ret, S=12):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
    try:
        from tests.shard_edit_runs_ops import ShardEditRunsFakeOps
        from tokenflow_amd import sharded
        fake = ShardEditRunsFakeOps()
        sharded.ops = fake
        n, d = 2, 8
        D = h * d
        sh = sharded.FrameShard(K, comm=GlooComm() if use_comm else None, edit_runs=True)
        Kl, f0, o = sh.Kl, sh.kf0, 1 if world > 1 else 0
        want_runs = [(f0, Kl)] + ([(0, f0)] if f0 else []) + ([(f0 + Kl, K - f0 - Kl)] if f0 + Kl < K else [])
        bad = []
        for E, mask in cases:
            B = 1 + 2 * E
            q, k, v, piv, *_ = _data(E, K, n, S, h, d, seed=E * 8 + mask)
            full = fake.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, inject_mask=mask)     # the oracle, per edit
            loc = lambda t: t.view(B, K, S, D)[:, f0:f0 + Kl].reshape(B * Kl, S, D)      # noqa: E731
            n_non = E - bin(mask).count("1")
            ns = (1 if mask else 0) + 2 * n_non + 2 * E
            gathers = []
            gather = sh._gather_slabs
            sh._gather_slabs = lambda slabs, tag: (gathers.append(len(slabs)), gather(slabs, tag))[1]
            try:
                fake.calls.clear()
                out = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, False, mode="bank_runs", n_edits=E,
                                           inject_mask=mask)
            finally:
                sh._gather_slabs = gather
            for e in range(E):
                sl = [0, 1 + 2 * e, 2 + 2 * e]
                err = float((out.view(B, Kl, S, D)[sl] - loc(full).view(B, Kl, S, D)[sl]).abs().max())
                if not err <= ATTN_TOL:
                    bad.append(f"E{E} mask {mask:#b} edit {e}: max abs err {err:.3e}")
            packs = [c for c in fake.calls if c[0] == "head_pack"]
            if packs != [("head_pack", ns, 1)] or gathers != [ns]:
                bad.append(f"E{E} mask {mask:#b}: packs {packs}, gathers {gathers}, want ONE of {ns} slabs each")
            runs_calls = [c for c in fake.calls if c[0] == "ext_attn_runs_edits"]
            if runs_calls != [("ext_attn_runs_edits", tuple(want_runs), E, mask, (False,) + (True,) * (len(want_runs) - 1), False)]:
                bad.append(f"E{E} mask {mask:#b}: run calls {runs_calls}")
            if any(c[0] in ("ext_attn", "ext_attn_edits", "ext_attn_edits_views", "ext_attn_runs") for c in fake.calls):
                bad.append(f"E{E} mask {mask:#b}: another attention form ran: {fake.calls}")
            # the in-place form: output into the halo-extended state, halo slot from the left neighbour
            ext = sh.ext_alloc(S, D, q.dtype, q.device, n_edits=E)
            ext[0][o:].copy_(piv[f0:f0 + Kl])
            ext[2].fill_(float("nan"))
            pe, ie, ke, reqs = sh.pivotal_block(loc(q), loc(k), loc(v), h, d ** -0.5, False, ext, mode="bank_runs",
                                                inv_norm=True, n_edits=E, inject_mask=mask)
            sh.halo_wait(reqs)
            ke4 = ke.view(B, Kl + o, S, D)
            if not float((ke4[:, o:].reshape(B * Kl, S, D) - loc(full)).abs().max()) <= ATTN_TOL:
                bad.append(f"E{E} mask {mask:#b}: pivotal_block state")
            if rank > 0 and not (torch.equal(pe[0], piv[f0 - 1]) and
                                 float((ke4[:, 0] - full.view(B, K, S, D)[:, f0 - 1]).abs().max()) <= ATTN_TOL):
                bad.append(f"E{E} mask {mask:#b}: halo slot")
        if world == 2:
            # one edit through the keyword is the single-edit bank_runs pass
            q, k, v, *_ = _data(1, K, n, S, h, d, seed=5)
            loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)      # noqa: E731
            a = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, True, mode="bank_runs")
            b = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, True, mode="bank_runs", n_edits=1)
            if not torch.equal(a, b):
                bad.append("n_edits=1")
            # a shard built WITHOUT the opt-in keeps the refusal, and its text names the opt-in
            plain = sharded.FrameShard(K, comm=GlooComm() if use_comm else None, edit_runs=False)
            z = torch.zeros(5 * Kl, S, D)
            try:
                plain.pivotal_attention(z, z, z, h, 1.0, False, mode="bank_runs", n_edits=2)
                bad.append("bank_runs with two edits did not raise without the opt-in")
            except ValueError as e:
                if "bank_runs" not in str(e) or "edit_runs" not in str(e):
                    bad.append(f"refusal text: {e}")
        ret[rank] = bad
        dist.barrier()      # no rank closes its connections while a peer is still receiving
    except Exception as e:      # noqa: BLE001  (reported once, through the shared dict)
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def _spawn(world, *args, S=12):
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port()) + args + (ret, S), nprocs=world, join=True)
    assert dict(ret) == {r: [] for r in range(world)}, dict(ret)


@pytest.mark.parametrize("use_comm", [False, True])
@pytest.mark.parametrize("K", [4, 5])
def test_two_ranks_equal_the_oracle_per_edit(K, use_comm):
    """K = 5: runs of 3 and 2 keyframes (the row forms of the collectives)."""
    _spawn(2, K, 2, use_comm, CASES)


@pytest.mark.parametrize("K,h", [(8, 8), (25, 5)])
def test_world8_baseline_geometries(K, h):
    """One keyframe per rank, and BASELINE config 5's geometry (runs of 4,3,3,3,3,3,3,3; 5 heads do not divide)."""
    _spawn(8, K, h, False, [(2, 0b01)] if K == 25 else [(2, 0b01), (3, 0b101)], S=4)


def _shard(world, bank_runs, edit_runs):
    from tokenflow_amd import sharded
    sh = sharded.FrameShard(max(world, 1), bank_runs=bank_runs, edit_runs=edit_runs)
    sh.world = world       # auto_mode reads nothing else
    return sh


@pytest.mark.parametrize("bank_runs", [False, True])
@pytest.mark.parametrize("edit_runs", [False, True])
def test_auto_mode_under_the_four_opt_in_combinations(monkeypatch, bank_runs, edit_runs):
    monkeypatch.delenv("TOKENFLOW_SHARD_BANK_RUNS", raising=False)
    monkeypatch.delenv("TOKENFLOW_SHARD_EDIT_RUNS", raising=False)
    sh = _shard(8, bank_runs, edit_runs)
    assert (sh.bank_runs, sh.edit_runs) == (bank_runs, edit_runs)
    for heads in (5, 10, 20):                       # cfg5: the heads never divide over 8 ranks
        for S in (64, 256, 1024, 4096):
            one = "bank_runs" if bank_runs and S >= 1024 else "bank"
            assert sh.auto_mode(heads, S) == sh.auto_mode(heads, S, 1) == one
            for E in (2, 3):
                assert sh.auto_mode(heads, S, E) == (one if edit_runs else "bank"), (heads, S, E)
    for S in (64, 256, 1024, 4096):                 # where the heads divide, the heads form stays (mid block: bank)
        for E in (1, 2):
            assert sh.auto_mode(8, S, E) == ("bank" if S <= 64 else "heads")


def test_opt_in_from_the_environment(monkeypatch):
    from tokenflow_amd import sharded
    monkeypatch.delenv("TOKENFLOW_SHARD_EDIT_RUNS", raising=False)
    assert not sharded.FrameShard(1).edit_runs
    monkeypatch.setenv("TOKENFLOW_SHARD_EDIT_RUNS", "1")
    assert sharded.FrameShard(1).edit_runs and not sharded.FrameShard(1, edit_runs=False).edit_runs
    monkeypatch.setenv("TOKENFLOW_SHARD_EDIT_RUNS", "0")
    assert not sharded.FrameShard(1).edit_runs and sharded.FrameShard(1, edit_runs=True).edit_runs


def _hooks_worker(rank, world, port, K, E, qk_sched, ret):
    """`register_frame_shard` + `register_edits` + `register_edit_schedules` on a shard with BOTH opt-ins whose `auto_mode`
    answers "bank_runs" (the toy frames are shorter than its threshold: the answer is planted): the pivotal pass on the
    rank's keyframes against the same hooks in one process."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
    try:
        import tokenflow_utils as tfu
        from oracle import golden_cases as gc
        from tests import fake_diffusers as fd
        from tests.shard_edit_runs_ops import ShardEditRunsFakeOps
        from tokenflow_amd import hooks, sharded
        fake = ShardEditRunsFakeOps()
        hooks.ops = fake
        sharded.ops = fake
        cfg = gc.BLOCKS_CFG
        B = 1 + 2 * E

        def pipe():
            torch.manual_seed(cfg["seed"])
            p = fd.FakePipeline(dims=cfg["dims"], heads=cfg["heads"], cross_dim=cfg["cross_dim"]).eval()
            tfu.register_extended_attention_pnp(p, [1])
            tfu.set_tokenflow(p.unet)
            tfu.register_time(p, 1)
            tfu.register_edits(p, E)
            tfu.register_edit_schedules(p, qk_schedules=qk_sched)
            return p
        S = 12
        g = torch.Generator().manual_seed(11)
        bad = []
        for name, lvl, blk_of in (("up3", 0, lambda p: p.unet.up_blocks[3].attentions[1].transformer_blocks[0]),
                                  ("down1", 1, lambda p: p.unet.down_blocks[1].attentions[0].transformer_blocks[0])):
            D = cfg["dims"][lvl]
            x_piv = torch.randn(B, K, S, D, generator=g)
            enc = torch.randn(B, K, 7, cfg["cross_dim"], generator=g)
            with torch.no_grad():
                ref_p = pipe()
                tfu.register_pivotal(ref_p, True)
                piv_out = blk_of(ref_p)(x_piv.reshape(B * K, S, D),
                                        encoder_hidden_states=enc.reshape(B * K, 7, -1)).view(B, K, S, D)
                sh = sharded.FrameShard(K, bank_runs=True, edit_runs=True)
                my_p = pipe()
                tfu.register_frame_shard(my_p, sh)
                lo, hi = sh.kf0, sh.kf0 + sh.Kl
                tfu.register_pivotal(my_p, True)
                sh.auto_mode = lambda heads, S_, n_edits=1: "bank_runs"
                fake.calls.clear()
                got_p = blk_of(my_p)(x_piv[:, lo:hi].reshape(B * sh.Kl, S, D),
                                     encoder_hidden_states=enc[:, lo:hi].reshape(B * sh.Kl, 7, -1)).view(B, sh.Kl, S, D)
                err = float((got_p - piv_out[:, lo:hi]).abs().max())
                if not err <= 1e-4:      # a block output: the attention's 2e-6 through the block's projections and norms
                    bad.append(f"{name}: pivotal pass, max abs err {err:.3e}")
                masks = {c[3] for c in fake.calls if c[0] == "ext_attn_runs_edits"}
                if masks != {sum(1 << e for e, sc in enumerate(qk_sched) if sc) if name == "up3" else 0}:
                    bad.append(f"{name}: injection masks {masks} at the shard")
                if any(c[0] == "ext_attn_edits_views" for c in fake.calls):
                    bad.append(f"{name}: the one-call part form ran")
        ret[rank] = bad
        dist.barrier()      # no rank closes its connections while a peer is still receiving
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("K,E,qk_sched", [(5, 3, [[1], [], [1]])])
def test_hooks_two_ranks_multi_edit_bank_runs(K, E, qk_sched):
    ret = mp.Manager().dict()
    mp.spawn(_hooks_worker, args=(2, _free_port(), K, E, qk_sched, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)
