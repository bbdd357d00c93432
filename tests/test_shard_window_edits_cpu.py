"""Several prompts on a windowed / anchored frame shard without a GPU: real gloo spawns of 2 and 3 ranks with torch stand-ins
for the ops (tests/shard_window_edit_fake_ops.py).  `FrameShard(window_edits=True).pivotal_attention(..., n_edits=E,
inject_mask=m, window=R, anchors=A)` equals the single-process multi-edit window / frame-set attention on the rank's keyframes
-- every edit, over torch.distributed and over a stand-in `comm` -- with exactly ONE pack, ONE row all-to-all and ONE bank call
of the plan's geometry; E = 1 records today's single-edit ops; and the hooks' opt-in matrix: with every keyword the sharded pass
equals the unsharded one, each missing keyword keeps its old message."""
import datetime
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_sharded_cpu import GlooComm, _free_port

TIMEOUT = datetime.timedelta(seconds=60)
EDITS = [(2, 0b00), (2, 0b11), (2, 0b01), (3, 0b101)]


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


def _slabs(E, mask):
    n_non = E - bin(mask).count("1")
    slots = (1 if mask else 0) + 2 * n_non
    return slots + 2 * E, (slots if mask and n_non else 0)


def _worker(rank, world, port, K, radii, ret):
    _init(rank, world, port)
    try:
        from tests.shard_window_edit_fake_ops import ShardWindowEditFakeOps
        from tokenflow_amd import sharded
        torch.set_num_threads(1)      # the ranks share this machine's cores
        fake = ShardWindowEditFakeOps()
        sharded.ops = fake
        S, h, d = 6, 2, 8
        D = h * d
        bad = []
        for use_comm in (False, True):
            sh = sharded.FrameShard(K, comm=GlooComm() if use_comm else None, window_edits=True)
            Kl, f0 = sh.Kl, sh.kf0
            n_a2a = [0]
            a2a = sh._a2a
            sh._a2a = lambda *a, **kw: (n_a2a.__setitem__(0, n_a2a[0] + 1), a2a(*a, **kw))[1]
            for R in (radii[1:3] if use_comm else radii):      # (the stand-in comm: two radii per world)
                for anchors in ((), (0,), (K - 1,), tuple(range(0, K, 3))):
                    for E, mask in EDITS:
                        B = 1 + 2 * E
                        loc = lambda t: t.view(B, K, S, D)[:, f0:f0 + Kl].reshape(B * Kl, S, D)      # noqa: E731
                        g = torch.Generator().manual_seed(10 * K + R + E)
                        q, k, v = (torch.randn(B * K, S, D, generator=g) for _ in range(3))
                        cover = R >= K - 1
                        if cover:
                            full = fake.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, inject_mask=mask)
                        elif anchors:
                            full = fake.ext_attn_frame_sets_edits(q, k, v, h, d ** -0.5, False, E,
                                                                  fake.bank_frame_sets(K, R, anchors), inject_mask=mask)
                        else:
                            full = fake.ext_attn_windows_edits(q, k, v, h, d ** -0.5, False, E, fake.bank_windows(K, R),
                                                               inject_mask=mask)
                        fake.calls.clear()
                        n_a2a[0] = 0
                        out = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, False, n_edits=E, inject_mask=mask,
                                                   window=R, anchors=anchors or None)
                        calls = list(fake.calls)
                        what = f"K{K} W{world} R{R} anchors{anchors} E{E} mask {mask:#b} comm={use_comm} rank {rank}"
                        if not torch.equal(out, loc(full)):      # every edit's data path
                            bad.append(f"{what}: max abs err {float((out - loc(full)).abs().max()):.3e}")
                        packs = [c for c in calls if c[0].endswith("halo_pack")]
                        if cover:      # today's multi-edit bank pass
                            if packs or any(c[0].endswith("_edits_views") and c[0] != "ext_attn_edits_views" for c in calls):
                                bad.append(f"{what}: a covering radius must issue today's pass")
                            continue
                        plan = sharded.frame_set_halo_plan(K, world, rank, R, anchors)
                        masks = tuple(plan.send) if anchors else tuple(((1 << n) - 1) << a for a, n in plan.send)
                        ns, nq = _slabs(E, mask)
                        if packs != [("edit_halo_pack", ns, nq, masks)] or n_a2a[0] != 1:
                            bad.append(f"{what}: packs {packs}, {n_a2a[0]} exchanges")
                        name = "ext_attn_frame_sets_edits_views" if anchors else "ext_attn_windows_edits_views"
                        banks = [c for c in calls if c[0].endswith("_edits_views") and c[0] != "ext_attn_edits_views"]
                        table = tuple(plan.sets) if anchors else tuple(plan.windows)
                        q0 = plan.q_frame0 if anchors else plan.hl
                        if (len(banks) != 1 or banks[0][0] != name or banks[0][2][1] != plan.F
                                or banks[0][3:] != (E, mask, table, "bank", True, q0)):
                            bad.append(f"{what}: bank calls {banks}")
                        src = [c for c in calls if c[0] == "ext_attn_edits_views"]
                        if [c[4] for c in src] != ["source"]:
                            bad.append(f"{what}: source calls {src}")
            # E = 1 records exactly today's single-edit ops, with and without anchors
            g = torch.Generator().manual_seed(3)
            q, k, v = (torch.randn(3 * K, S, D, generator=g) for _ in range(3))
            loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)      # noqa: E731
            for anchors in (None, (0,)):
                for mask in (0, 1):
                    fake.calls.clear()
                    a = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, bool(mask), window=1, anchors=anchors)
                    one = list(fake.calls)
                    fake.calls.clear()
                    b = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, bool(mask), n_edits=1, window=1,
                                             anchors=anchors)
                    if one != list(fake.calls) or not torch.equal(a, b) or any("edit" in c[0] for c in one):
                        bad.append(f"n_edits=1 anchors={anchors} mask={mask}: {one} / {fake.calls}")
            # without the opt-in, and on objects made with __new__, the old refusal
            t5 = torch.zeros(5 * Kl, S, D)
            off = sharded.FrameShard(K, comm=GlooComm() if use_comm else None)
            raw = sharded.FrameShard.__new__(sharded.FrameShard)
            raw.K, raw.Kl, raw.world = K, Kl, world
            for obj in (off, raw):
                for kw in (dict(window=1), dict(window=1, anchors=(0,))):
                    try:
                        obj.pivotal_attention(t5, t5, t5, h, 1.0, False, n_edits=2, inject_mask=0, **kw)
                        bad.append(f"no ValueError without the opt-in for {kw}")
                    except ValueError as e:
                        if "runs one edit" not in str(e):
                            bad.append(str(e))
            for kw in (dict(window=1, n_edits=2, inject_mask=0b100), dict(window=1, n_edits=2, mode="bank"),
                       dict(window=-1, n_edits=2), dict(anchors=(0,), n_edits=2), dict(window=1, anchors=(K,), n_edits=2)):
                try:
                    sh.pivotal_attention(t5, t5, t5, h, d ** -0.5, False, **kw)
                    bad.append(f"no ValueError for {kw}")
                except ValueError:
                    pass
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,K,radii", [(2, 5, (0, 1, 2, 3, 6)), (3, 7, (0, 1, 2, 3, 6))])
def test_windowed_multi_edit_shard_equals_the_single_process_composition(world, K, radii):
    """K = 5 over 2 ranks (3, 2) and K = 7 over 3 (3, 2, 2): uneven shards; anchors owned by the first, the last and a middle
    rank; R = 3 spans two ranks; R = 6 covers the bank."""
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), K, radii, ret), nprocs=world, join=True)
    assert dict(ret) == {r: [] for r in range(world)}, dict(ret)


def _hooks_worker(rank, world, port, K, ret):
    _init(rank, world, port)
    try:
        import tokenflow_utils as tfu
        from tests import fake_diffusers as fd
        from tests.shard_window_edit_fake_ops import ShardWindowEditFakeOps
        from tokenflow_amd import hooks, sharded
        torch.set_num_threads(1)
        fake = ShardWindowEditFakeOps()
        hooks.ops = fake
        sharded.ops = fake
        S, h, dims, E = 6, 2, (16, 32, 64), 2
        D, B = dims[0], 1 + 2 * E
        qk_sched = [[1], []]      # edit 0 injects at step 1, edit 1 never: a mixed mask at the injected blocks

        def pipe(registered, **kw):
            torch.manual_seed(0)
            p = fd.FakePipeline(dims=dims, heads=h, cross_dim=8).eval()
            tfu.register_extended_attention_pnp(p, [1])
            tfu.set_tokenflow(p.unet)
            tfu.register_time(p, 1)
            tfu.register_edits(p, E)
            tfu.register_edit_schedules(p, qk_schedules=qk_sched)
            if registered is not None:
                tfu.register_frame_shard(p, registered)
            tfu.register_bank_window(p, 1, **kw)
            tfu.register_pivotal(p, True)
            return p, p.unet.up_blocks[3].attentions[1].transformer_blocks[0].attn1
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B, K, S, D, generator=g)
        bad = []
        with torch.no_grad():
            sh = sharded.FrameShard(K, window_edits=True)
            lo, hi = sh.kf0, sh.kf0 + sh.Kl
            xl = x[:, lo:hi].reshape(B * sh.Kl, S, D)
            every = dict(shard=True, edits=True, edit_shard=True)
            with_anchors = dict(every, anchors=[0, K - 1], anchor_edits=True, anchor_shard=True)
            for kw, ref_kw, name in ((every, dict(edits=True), "ext_attn_windows_edits_views"),
                                     (with_anchors, dict(edits=True, anchors=[0, K - 1], anchor_edits=True),
                                      "ext_attn_frame_sets_edits_views")):
                _, attn = pipe(None, **ref_kw)
                want = attn(x.reshape(B * K, S, D)).view(B, K, S, D).clone()
                fake.calls.clear()
                _, attn = pipe(sh, **kw)
                got = attn(xl).view(B, sh.Kl, S, D)
                if not torch.equal(got, want[:, lo:hi]):
                    bad.append(f"{name}: max abs err {float((got - want[:, lo:hi]).abs().max()):.3e}")
                banks = [c for c in fake.calls if c[0] == name]
                if len(banks) != 1 or banks[0][3:5] != (E, 0b01):      # the step's per-edit mask reaches the shard
                    bad.append(f"{name}: bank calls {banks}")

            def refused(what, needle, shard_obj=sh, **kw):
                _, a = pipe(shard_obj, **kw)
                try:
                    a(xl)
                    bad.append(f"{what}: no ValueError")
                except ValueError as e:
                    if needle not in str(e):
                        bad.append(f"{what}: {e}")
            one_edit = "a sliding-window bank on a registered frame shard runs one edit"
            refused("without edit_shard=True", one_edit, shard=True, edits=True)
            refused("without edits=True", one_edit, shard=True, edit_shard=True)
            refused("without shard=True", "a sliding-window bank on a registered frame shard is not supported", edits=True,
                    edit_shard=True)
            refused("a shard built without window_edits", one_edit, shard_obj=sharded.FrameShard(K), **every)
            refused("anchors without anchor_edits=True", "anchor keyframes in a multi-edit batch", **dict(with_anchors,
                                                                                                            anchor_edits=False))
            refused("anchors without anchor_shard=True", "anchor keyframes on a registered frame shard are not supported",
                    **dict(with_anchors, anchor_shard=False))

            class NoWindowEdits:      # a shard type that takes window= but never heard of the opt-in: the pinned error
                world, rank, K, Kl, kf0, supports_window, supports_edits = sh.world, sh.rank, sh.K, sh.Kl, sh.kf0, True, True
            refused("a shard type without supports_window_edits", one_edit, shard_obj=NoWindowEdits(), **every)
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_hooks_opt_in_matrix_two_ranks():
    ret = mp.Manager().dict()
    mp.spawn(_hooks_worker, args=(2, _free_port(), 6, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)


def test_register_bank_window_edit_shard_sets_and_clears_state():
    import tokenflow_utils as tfu
    from tests import fake_diffusers as fd
    from tokenflow_amd import hooks
    pipe = fd.FakePipeline(dims=(16, 32, 64), heads=2, cross_dim=8).eval()
    blocks = hooks._hook_blocks(pipe.unet)
    state = lambda: {(getattr(m, "bank_window_shard"), getattr(m, "bank_window_edit_shard"))      # noqa: E731
                     for tb in blocks for m in (tb, tb.attn1)}
    tfu.register_bank_window(pipe, 1, edits=True, shard=True, edit_shard=True)
    assert state() == {(True, True)}
    tfu.register_bank_window(pipe, 1, edits=True, shard=True)      # the keyword is per call
    assert state() == {(True, False)}
    tfu.register_bank_window(pipe, None, edits=True, shard=True, edit_shard=True)      # no window: nothing to open
    assert state() == {(False, False)}
    hooks._set_bank_window(blocks, 1, True, (0,))      # existing callers of the helper keep working
    assert state() == {(False, False)}
