"""Multi-edit batches on a frame shard, on 2 and on 8 CPU processes (gloo): the exchange logic of tokenflow_amd/sharded.py
with the oracle-backed ops of tests/shard_edit_ops.py standing in for the HIP ops.

Every rank's attention, halo-extended state and propagation must equal the single-process multi-edit results bit for bit
(work is partitioned, not re-associated), with the collectives and the launches of a block at the single-edit count: ONE
pack of 2 * (any_inject + 2 * n_non_injecting) + 2E slabs, two all-to-alls or one gather, ONE unpack into 2E destinations,
ONE search per propagation call."""
import datetime
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import tokenflow_oracle as orc
from tests.test_sharded_cpu import GlooComm, _free_port

TIMEOUT = datetime.timedelta(seconds=60)      # a rank that fails early ends the test instead of hanging its peer
CASES = [(2, 0b00), (2, 0b11), (2, 0b01), (3, 0b000), (3, 0b111), (3, 0b001), (3, 0b101)]


def _data(E, K, n, S, h, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, D = 1 + 2 * E, h * d
    q, k, v = (torch.randn(B * K, S, D, generator=g) for _ in range(3))
    piv = torch.randn(K, S, D, generator=g)
    kf_out = torch.randn(B * K, S, D, generator=g)
    tgt = torch.randn(K, n * S, D, generator=g)            # per chunk
    res = torch.randn(K, B * n, S, D, generator=g)
    return q, k, v, piv, kf_out, tgt, res


def _slab_count(E, mask):
    n_non = E - bin(mask).count("1")
    return 2 * ((1 if mask else 0) + 2 * n_non) + 2 * E


def _check_case(sharded, fake, sh, world, E, mask, mode, K, n, S, h, d):
    """One (E, mask, mode) on this rank against the single-process results; returns a list of failure texts."""
    bad = []
    B, D = 1 + 2 * E, h * d
    q, k, v, piv, kf_out, tgt, res = _data(E, K, n, S, h, d, seed=E * 8 + mask)
    full_attn = fake.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, inject_mask=mask)
    inv = fake.pivot_inv_norm(piv)
    w = orc.blend_weights(n, 1)
    full_prop = [fake.propagate_chunks_edits(tgt[c], piv, inv, kf_out, None if c == 0 else w, n, 1, c, c == 0, res[c],
                                             torch.float32, E) for c in range(K)]
    Kl, f0, o = sh.Kl, sh.kf0, 1 if world > 1 else 0
    loc = lambda t: t.view(B, K, S, D)[:, f0:f0 + Kl].reshape(B * Kl, S, D)
    counts = {"a2a": 0, "gather": 0}
    a2a, gather = sh._a2a, sh._gather_slabs
    sh._a2a = lambda *a, **kw: (counts.__setitem__("a2a", counts["a2a"] + 1), a2a(*a, **kw))[1]
    sh._gather_slabs = lambda *a, **kw: (counts.__setitem__("gather", counts["gather"] + 1), gather(*a, **kw))[1]
    try:
        fake.calls.clear()
        out = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, False, mode=mode, n_edits=E, inject_mask=mask)
        if not torch.equal(out, loc(full_attn)):
            bad.append("attention")
        eff = mode or sh.auto_mode(h, S, E)
        packs = [c for c in fake.calls if c[0] == "head_pack"]
        unpacks = [c for c in fake.calls if c[0] == "head_unpack"]
        parts = [c[4] for c in fake.calls if c[0] == "ext_attn_edits_views"]
        if eff == "heads":
            want = ([("head_pack", _slab_count(E, mask), world)], [("head_unpack", 2 * E)], ["source", "bank"], 2, 0)
        else:       # exactly the compact k slots and the 2E value slabs travel
            want = ([("head_pack", _slab_count(E, mask) // 2 + E, 1)], [], ["bank", "source"], 0, 1)
        if (packs, unpacks, parts, counts["a2a"], counts["gather"]) != want:
            bad.append(f"launches {(packs, unpacks, parts, counts)} != {want}")
        if any(c[0] in ("ext_attn", "ext_attn_edits") for c in fake.calls):
            bad.append("a single-edit or one-process attention call in a sharded multi-edit pass")
        # ---- halo + propagation, chunk by chunk and all chunks in one call
        piv_e, inv_e, kfo_e = sh.exchange_halo(piv[f0:f0 + Kl], inv[f0:f0 + Kl], loc(kf_out), n_edits=E)
        for j in range(Kl):
            fake.calls.clear()
            y = sh.propagate(j, tgt[f0 + j], res[f0 + j], piv_e, inv_e, kfo_e, w, n, n_edits=E)
            if not torch.equal(y, full_prop[f0 + j]) or [c[0] for c in fake.calls] != ["propagate_chunks_edits"]:
                bad.append(f"propagate {j}")
        tgt_all = torch.cat([tgt[f0 + j] for j in range(Kl)])
        res_all = torch.stack([res[f0 + j].view(B, n, S, D) for j in range(Kl)], dim=1).reshape(B * Kl * n, S, D)
        want_all = torch.stack([full_prop[f0 + j].view(B, n, S, D) for j in range(Kl)], dim=1).reshape(B * Kl * n, S, D)
        fake.calls.clear()
        got = sh.propagate_all(tgt_all, res_all, piv_e, inv_e, kfo_e, w, n, n_edits=E)
        if not torch.equal(got, want_all) or [c[0] for c in fake.calls] != ["propagate_chunks_edits"]:
            bad.append("propagate_all")       # ONE multi-edit call = one search, one gather over all branches
        # ---- the in-place two-pass form: the attention writes the halo-extended state, ONE grouped exchange carries the
        #      last keyframe of all B branches, the first chunk is deferred behind it
        ext = sh.ext_alloc(S, D, q.dtype, q.device, n_edits=E)
        if ext[2].shape != (B, Kl + o, S, D):
            bad.append("ext_alloc")
        ext[0][o:].copy_(piv[f0:f0 + Kl])
        pe, ie, ke, reqs = sh.pivotal_block(loc(q), loc(k), loc(v), h, d ** -0.5, False, ext, mode=mode, inv_norm=True,
                                            n_edits=E, inject_mask=mask)
        ke4 = ke.view(B, Kl + o, S, D)
        if not torch.equal(ke4[:, o:].reshape(B * Kl, S, D), loc(full_attn)):
            bad.append("pivotal_block state")
        sh.halo_wait(reqs)
        if sh.rank > 0 and not (torch.equal(ke4[:, 0], full_attn.view(B, K, S, D)[:, f0 - 1]) and
                                torch.equal(pe[0], piv[f0 - 1]) and torch.equal(ie[0], inv[f0 - 1])):
            bad.append("halo slot of pivotal_block")
        h0 = sh.halo_start(piv[f0:f0 + Kl], inv[f0:f0 + Kl], n_edits=E)
        pe, ie, ke, reqs = sh.halo_finish(h0, loc(kf_out), wait=False, n_edits=E)
        fake.calls.clear()
        first, rest = sh.propagate_all(tgt_all, res_all, pe, ie, ke, w, n, halo_reqs=reqs, n_edits=E)
        if not torch.equal(first, full_prop[f0]):
            bad.append("deferred first chunk")
        if Kl > 1 and not torch.equal(rest, want_all.view(B, Kl, n, S, D)[:, 1:].reshape(B * (Kl - 1) * n, S, D)):
            bad.append("chunks behind the first")
        if [c[0] for c in fake.calls] != ["propagate_chunks_edits"] * (2 if Kl > 1 else 1):
            bad.append(f"deferred form calls {fake.calls}")
    finally:
        sh._a2a, sh._gather_slabs = a2a, gather
    return [f"E{E} mask {mask:#b} {mode}: {b}" for b in bad]


def _single_edit_trace(sharded, fake, sh, world, K, n, S, h, d, mode, inject):
    """n_edits = 1 issues exactly the single-edit ops: the call trace with the keyword equals the trace without it."""
    from tests.test_sharded_cpu import _data as data1
    q, k, v, piv, kf_out, tgt, res = data1(K, n, S, h, d)
    D, Kl, f0, o = h * d, sh.Kl, sh.kf0, 1 if world > 1 else 0
    loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)
    inv, w = fake.pivot_inv_norm(piv), orc.blend_weights(n, 1)
    tgt_all = torch.cat([tgt[f0 + j] for j in range(Kl)])
    res_all = torch.stack([res[f0 + j].view(3, n, S, D) for j in range(Kl)], dim=1).reshape(3 * Kl * n, S, D)
    traces, outs = [], []
    for kw in ({}, {"n_edits": 1}):
        fake.calls.clear()
        out = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, inject, mode=mode,
                                   **({"n_edits": 1, "inject_mask": None} if kw else {}))
        pe, ie, ke = sh.exchange_halo(piv[f0:f0 + Kl], inv[f0:f0 + Kl], loc(kf_out), **kw)
        y = sh.propagate(0, tgt[f0], res[f0], pe, ie, ke, w, n, **kw)
        got = sh.propagate_all(tgt_all, res_all, pe, ie, ke, w, n, **kw)
        ext = sh.ext_alloc(S, D, q.dtype, q.device, **kw)
        ext[0][o:].copy_(piv[f0:f0 + Kl])
        blk = sh.pivotal_block(loc(q), loc(k), loc(v), h, d ** -0.5, inject, ext, mode=mode, inv_norm=True, **kw)
        sh.halo_wait(blk[3])
        traces.append(list(fake.calls))
        outs.append((out, y, got, blk[2].view(3, Kl + o, S, D)[:, o:].clone()))      # (slot 0 stays unset on rank 0)
    same = traces[0] == traces[1] and all(torch.equal(a, b) for a, b in zip(*outs))
    names = [c[0] for c in traces[0]]
    return same and "ext_attn" in names and not any(x.endswith("_edits") or x.endswith("edits_views") for x in names)


def _worker(rank, world, port, K, h, use_comm, cases, modes, ret, S=12):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
    try:
        from tests.shard_edit_ops import ShardEditFakeOps
        from tokenflow_amd import sharded
        fake = ShardEditFakeOps()
        sharded.ops = fake
        n, d = 2, 8
        sh = sharded.FrameShard(K, comm=GlooComm() if use_comm else None)
        bad = []
        for mode in modes:
            for E, mask in cases:
                bad += _check_case(sharded, fake, sh, world, E, mask, mode, K, n, S, h, d)
        if world == 2:
            for mode in ("heads", "bank"):
                for inject in (False, True):
                    if not _single_edit_trace(sharded, fake, sh, world, K, n, S, h, d, mode, inject):
                        bad.append(f"n_edits=1 trace, {mode}, inject {inject}")
            # "bank_runs" has no multi-edit form: explicit mode raises, the opt-in of auto_mode falls back to "bank"
            q = torch.zeros(5 * sh.Kl, S, h * d)
            try:
                sh.pivotal_attention(q, q, q, h, 1.0, False, mode="bank_runs", n_edits=2)
                bad.append("bank_runs with two edits did not raise")
            except ValueError as e:
                if "bank_runs" not in str(e):
                    bad.append(f"bank_runs message: {e}")
            runs = sharded.FrameShard(K, comm=GlooComm() if use_comm else None, bank_runs=True)
            if (runs.auto_mode(3, 4096), runs.auto_mode(3, 4096, 2), runs.auto_mode(3, 4096, 1)) != \
                    ("bank_runs", "bank", "bank_runs"):
                bad.append("auto_mode under the bank_runs opt-in")
            try:
                sh.pivotal_attention(q, q, q, h, 1.0, True, mode="bank", n_edits=2, inject_mask=0b01)
                bad.append("inject=True beside a mask did not raise")
            except ValueError:
                pass
        ret[rank] = bad
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
def test_two_ranks_equal_single_process(K, use_comm):
    """K = 5: runs of 3 and 2 keyframes (the row forms of the collectives)."""
    _spawn(2, K, 2, use_comm, CASES, ("heads", "bank"))


def test_world8_cfg5_geometry():
    """BASELINE config 5 at its rank geometry, toy token count: 25 keyframes in runs of 4,3,3,3,3,3,3,3; 5 heads do not divide
    over the ranks, so `auto_mode` answers "bank"."""
    _spawn(8, 25, 5, False, [(2, 0b01)], (None,), S=4)


def _hooks_worker(rank, world, port, K, E, qk_sched, mode, ret):
    """`register_frame_shard` + `register_edits` + `register_edit_schedules` on two ranks against the same hooks in one
    process, on the small fake pipeline: pivotal pass on the rank's keyframes, chunk passes of its chunks."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
    try:
        import tokenflow_utils as tfu
        from oracle import golden_cases as gc
        from tests import fake_diffusers as fd
        from tests.shard_edit_ops import ShardEditFakeOps
        from tokenflow_amd import hooks, sharded
        fake = ShardEditFakeOps()
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
        n, S = 2, 12
        g = torch.Generator().manual_seed(11)
        bad = []
        # a decoder block (its attn1 injects: the per-edit mask reaches the shard) and an encoder block (mask 0)
        for name, lvl, blk_of in (("up3", 0, lambda p: p.unet.up_blocks[3].attentions[1].transformer_blocks[0]),
                                  ("down1", 1, lambda p: p.unet.down_blocks[1].attentions[0].transformer_blocks[0])):
            D = cfg["dims"][lvl]
            x_piv = torch.randn(B, K, S, D, generator=g)
            enc = torch.randn(B, K, 7, cfg["cross_dim"], generator=g)
            chunks = [torch.randn(B * n, S, D, generator=g) for _ in range(K)]
            enc_n = torch.randn(B * n, 7, cfg["cross_dim"], generator=g)
            with torch.no_grad():
                ref_p = pipe()
                blk = blk_of(ref_p)
                tfu.register_pivotal(ref_p, True)
                piv_out = blk(x_piv.reshape(B * K, S, D), encoder_hidden_states=enc.reshape(B * K, 7, -1)).view(B, K, S, D)
                tfu.register_pivotal(ref_p, False)
                want = []
                for c in range(K):
                    tfu.register_batch_idx(ref_p, c)
                    want.append(blk(chunks[c], encoder_hidden_states=enc_n))
                sh = sharded.FrameShard(K)
                my_p = pipe()
                tfu.register_frame_shard(my_p, sh)
                blk = blk_of(my_p)
                lo, hi = sh.kf0, sh.kf0 + sh.Kl
                tfu.register_pivotal(my_p, True)
                sh.auto_mode = lambda heads, S_, n_edits=1: mode
                fake.calls.clear()
                got_p = blk(x_piv[:, lo:hi].reshape(B * sh.Kl, S, D),
                            encoder_hidden_states=enc[:, lo:hi].reshape(B * sh.Kl, 7, -1)).view(B, sh.Kl, S, D)
                if not torch.equal(got_p, piv_out[:, lo:hi]):
                    bad.append(f"{name}: pivotal pass")
                masks = {c[3] for c in fake.calls if c[0] == "ext_attn_edits_views"}
                if masks != {sum(1 << e for e, sc in enumerate(qk_sched) if sc) if name == "up3" else 0}:
                    bad.append(f"{name}: injection masks {masks} at the shard")
                tfu.register_pivotal(my_p, False)
                for c in range(lo, hi):
                    tfu.register_batch_idx(my_p, c)
                    if not torch.equal(blk(chunks[c], encoder_hidden_states=enc_n), want[c]):
                        bad.append(f"{name}: chunk {c}")
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("K,E,qk_sched,mode", [(4, 2, [[1], []], "heads"), (5, 3, [[1], [], [1]], "bank")])
def test_hooks_two_ranks_multi_edit(K, E, qk_sched, mode):
    """The hook API with edits AND a frame shard reproduces the single-process multi-edit block outputs bit for bit."""
    ret = mp.Manager().dict()
    mp.spawn(_hooks_worker, args=(2, _free_port(), K, E, qk_sched, mode, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)


def test_a_shard_without_the_capability_still_raises(monkeypatch):
    """A `NativeShard`-like object (supports_edits = False, or a type that never heard of edits) keeps the refusal."""
    import tokenflow_utils as tfu
    from oracle import golden_cases as gc
    from tests import edit_forms as ef
    from tests import fake_diffusers as fd
    from tokenflow_amd import hooks
    monkeypatch.setattr(hooks, "ops", ef.EditFakeOps())
    cfg = gc.BLOCKS_CFG
    torch.manual_seed(cfg["seed"])
    pipe = fd.FakePipeline(dims=cfg["dims"], heads=cfg["heads"], cross_dim=cfg["cross_dim"]).eval()
    tfu.register_extended_attention_pnp(pipe, [])
    tfu.set_tokenflow(pipe.unet)
    tfu.register_time(pipe, 1)
    tfu.register_pivotal(pipe, True)
    tfu.register_edits(pipe, 2)
    blk = pipe.unet.down_blocks[0].attentions[0].transformer_blocks[0]
    x, enc = torch.randn(10, 16, cfg["dims"][0]), torch.randn(10, 7, 32)

    class _Native:
        world, Kl, kf0 = 2, 2, 0
        supports_edits = False
    with torch.no_grad():
        tfu.register_frame_shard(pipe.unet, _Native())
        with pytest.raises(ValueError, match="frame shard"):
            blk(x, encoder_hidden_states=enc)
        with pytest.raises(ValueError, match="frame shard"):
            blk.attn1(x)
        tfu.register_frame_shard(pipe.unet, None)
        blk(x, encoder_hidden_states=enc)


def test_supports_edits_marks_the_capability():
    from tokenflow_amd import sharded
    assert sharded.FrameShard.supports_edits is True and sharded.NativeShard.supports_edits is False
