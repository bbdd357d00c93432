"""Anchor keyframes on a windowed frame shard without a GPU: real gloo spawns of 2 and 3 ranks with torch stand-ins for the ops
(tests/shard_frame_set_fake_ops.py).  `FrameShard.pivotal_attention(..., window=R, anchors=A)` equals the single-process
frame-set attention on the rank's keyframes -- over torch.distributed and over a stand-in `comm` -- with exactly one pack and
one bank call of the plan's geometry; anchors=() records today's windowed ops; and the hooks' opt-in
`register_bank_window(..., shard=True, anchor_shard=True)` equals the unsharded anchored pass."""
import datetime
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_sharded_cpu import GlooComm, _free_port

TIMEOUT = datetime.timedelta(seconds=60)


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


def _anchor_sets(K):
    return [(), (0,), (K - 1,), (0, K // 2), tuple(range(0, K, 3))]


def _worker(rank, world, port, K, radii, ret):
    _init(rank, world, port)
    try:
        from tests.shard_frame_set_fake_ops import ShardFrameSetFakeOps
        from tokenflow_amd import sharded
        torch.set_num_threads(1)      # the ranks share this machine's cores
        fake = ShardFrameSetFakeOps()
        sharded.ops = fake
        S, h, d = 6, 2, 8
        D = h * d
        bad = []
        for use_comm in (False, True):
            sh = sharded.FrameShard(K, comm=GlooComm() if use_comm else None)
            Kl, f0 = sh.Kl, sh.kf0
            loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)      # noqa: E731
            for R in (radii[1:3] if use_comm else radii):      # (the stand-in comm: two radii per world)
                for anchors in _anchor_sets(K):
                    inject = (R + len(anchors)) % 2 == 1
                    g = torch.Generator().manual_seed(10 * K + R)
                    q, k, v = (torch.randn(3 * K, S, D, generator=g) for _ in range(3))
                    cover = R >= K - 1
                    full = (fake.ext_attn(q, k, v, h, d ** -0.5, inject) if cover
                            else fake.ext_attn_frame_sets(q, k, v, h, d ** -0.5, inject, fake.bank_frame_sets(K, R, anchors)))
                    fake.calls.clear()
                    out = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, inject, window=R, anchors=anchors)
                    calls = list(fake.calls)
                    what = f"K{K} W{world} R{R} anchors{anchors} inject={inject} comm={use_comm} rank {rank}"
                    if not torch.equal(out, loc(full)):
                        bad.append(f"{what}: max abs err {float((out - loc(full)).abs().max()):.3e}")
                    packs = [c for c in calls if c[0] in ("window_halo_pack", "frame_set_halo_pack")]
                    if cover:
                        if packs:
                            bad.append(f"{what}: a covering radius must issue today's pass")
                        continue
                    if not anchors:      # exactly today's windowed ops
                        fake.calls.clear()
                        sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, inject, window=R)
                        if calls != list(fake.calls) or [c[0] for c in packs] != ["window_halo_pack"]:
                            bad.append(f"{what}: anchors=() recorded {calls}, the windowed pass {fake.calls}")
                        continue
                    plan = sharded.frame_set_halo_plan(K, world, rank, R, anchors)
                    if packs != [("frame_set_halo_pack", 3 if inject else 4, tuple(plan.send))]:
                        bad.append(f"{what}: packs {packs}")
                    banks = [c for c in calls if c[0] in ("ext_attn_frame_sets_views", "ext_attn_windows_views")]
                    if (len(banks) != 1 or banks[0][0] != "ext_attn_frame_sets_views" or banks[0][2][1] != plan.F
                            or banks[0][4:] != (tuple(plan.sets), "bank", plan.q_frame0)):
                        bad.append(f"{what}: bank calls {banks}")
            for kw in (dict(window=1, anchors=(0,), n_edits=2), dict(window=-1, anchors=(0,)), dict(anchors=(0,)),
                       dict(window=1, anchors=(K,)), dict(window=1, anchors=(0,), mode="bank")):
                try:
                    sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, False, **kw)
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
def test_anchored_shard_equals_the_single_process_frame_set_attention(world, K, radii):
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
        from tests.shard_frame_set_fake_ops import ShardFrameSetFakeOps
        from tokenflow_amd import hooks, sharded
        torch.set_num_threads(1)
        fake = ShardFrameSetFakeOps()
        hooks.ops = fake
        sharded.ops = fake
        S, h, dims = 6, 2, (16, 32, 64)
        D = dims[0]

        def pipe(registered, **kw):
            torch.manual_seed(0)
            p = fd.FakePipeline(dims=dims, heads=h, cross_dim=8).eval()
            tfu.register_extended_attention_pnp(p, [1])
            tfu.set_tokenflow(p.unet)
            tfu.register_time(p, 1)
            if registered is not None:
                tfu.register_frame_shard(p, registered)
            tfu.register_bank_window(p, 1, **kw)
            tfu.register_pivotal(p, True)
            return p, p.unet.up_blocks[3].attentions[1].transformer_blocks[0].attn1
        g = torch.Generator().manual_seed(1)
        x = torch.randn(3, K, S, D, generator=g)
        bad = []
        with torch.no_grad():
            sh = sharded.FrameShard(K)
            lo, hi = sh.kf0, sh.kf0 + sh.Kl
            xl = x[:, lo:hi].reshape(3 * sh.Kl, S, D)
            # anchors given as indices and as a stride: both resolve against the shard's WHOLE bank (K = 6: 0, 4; not the 3 local)
            for anchors, resolved in (([0, K - 1], (0, K - 1)), (4, (0, 4))):
                _, attn = pipe(None, anchors=anchors)
                want = attn(x.reshape(3 * K, S, D)).view(3, K, S, D).clone()
                fake.calls.clear()
                _, attn = pipe(sh, shard=True, anchors=anchors, anchor_shard=True)
                got = attn(xl).view(3, sh.Kl, S, D)
                if not torch.equal(got, want[:, lo:hi]):
                    bad.append(f"anchors={anchors}: max abs err {float((got - want[:, lo:hi]).abs().max()):.3e}")
                plan = sharded.frame_set_halo_plan(K, world, rank, 1, resolved)
                banks = [c for c in fake.calls if c[0] == "ext_attn_frame_sets_views"]
                if len(banks) != 1 or banks[0][4:] != (tuple(plan.sets), "bank", plan.q_frame0):
                    bad.append(f"anchors={anchors}: bank calls {banks}, plan {plan}")

            def refused(what, needle, setup, **kw):
                p, a = pipe(sh, **kw)
                setup(p, a)
                try:
                    a(xl)
                    bad.append(f"{what}: no ValueError")
                except ValueError as e:
                    if needle not in str(e):
                        bad.append(f"{what}: {e}")
            nothing = lambda p, a: None      # noqa: E731
            refused("without anchor_shard=True", "anchor keyframes on a registered frame shard are not supported (every rank "
                    "would have to hold the anchors)", nothing, shard=True, anchors=[0])
            refused("without shard=True", "a sliding-window bank on a registered frame shard is not supported", nothing,
                    anchors=[0], anchor_shard=True)
            refused("an index >= shard.K", f"on a frame shard of {K} keyframes", nothing, shard=True, anchors=[0, K],
                    anchor_shard=True)
            refused("segments", "keyframe segments", lambda p, a: setattr(a, "keyframe_segments", (1, 1)), shard=True,
                    anchors=[0], anchor_shard=True)
            refused("edits", "one edit", lambda p, a: setattr(a, "n_edits", 2), shard=True, anchors=[0], anchor_shard=True)
            # an index that fits the whole bank but not the rank's local count passes
            _, attn = pipe(sh, shard=True, anchors=[K - 1], anchor_shard=True)
            attn(xl)

            class NoAnchors:      # a shard type that takes window= but not anchors=: the pinned error
                world, rank, K, Kl, kf0, supports_window = sh.world, sh.rank, sh.K, sh.Kl, sh.kf0, True
            p, a = pipe(sh, shard=True, anchors=[0], anchor_shard=True)
            a.__dict__["_tf_shard"] = NoAnchors()
            try:
                a(xl)
                bad.append("a shard type without anchors=: no ValueError")
            except ValueError as e:
                if "anchor keyframes on a registered frame shard are not supported" not in str(e):
                    bad.append(str(e))
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_hooks_opt_in_two_ranks():
    ret = mp.Manager().dict()
    mp.spawn(_hooks_worker, args=(2, _free_port(), 6, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)


def test_register_bank_window_anchor_shard_sets_and_clears_state():
    import tokenflow_utils as tfu
    from tests import fake_diffusers as fd
    from tokenflow_amd import hooks
    pipe = fd.FakePipeline(dims=(16, 32, 64), heads=2, cross_dim=8).eval()
    blocks = hooks._hook_blocks(pipe.unet)
    state = lambda: {(getattr(m, "bank_window_shard"), getattr(m, "bank_window_anchor_shard"))      # noqa: E731
                     for tb in blocks for m in (tb, tb.attn1)}
    tfu.register_bank_window(pipe, 1, anchors=[0], shard=True, anchor_shard=True)
    assert state() == {(True, True)}
    tfu.register_bank_window(pipe, 1, anchors=[0], shard=True)      # the keyword is per call
    assert state() == {(True, False)}
    tfu.register_bank_window(pipe, None, anchors=[0], shard=True, anchor_shard=True)      # no window: nothing to open
    assert state() == {(False, False)}
