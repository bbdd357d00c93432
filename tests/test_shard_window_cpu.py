"""Sliding-window keyframe bank on a frame shard without a GPU: real gloo spawns of 2 and 3 ranks with torch stand-ins for the
ops (tests/shard_window_fake_ops.py).  `FrameShard.pivotal_attention(..., window=R)` equals the single-process windowed
attention on the rank's keyframes -- over torch.distributed and over a stand-in `comm`, with uneven shards and a radius that
spans two ranks -- and the hooks' opt-in `register_bank_window(..., shard=True)` equals the unsharded windowed pass."""
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


def _worker(rank, world, port, K, radii, ret):
    _init(rank, world, port)
    try:
        from tests.shard_window_fake_ops import ShardWindowFakeOps
        from tokenflow_amd import sharded
        torch.set_num_threads(1)      # the ranks share this machine's cores
        fake = ShardWindowFakeOps()
        sharded.ops = fake
        S, h, d = 6, 2, 8
        D = h * d
        bad = []
        for use_comm in (False, True):
            sh = sharded.FrameShard(K, comm=GlooComm() if use_comm else None)
            Kl, f0 = sh.Kl, sh.kf0
            loc = lambda t: t.view(3, K, S, D)[:, f0:f0 + Kl].reshape(3 * Kl, S, D)      # noqa: E731
            for R in (radii[1:3] if use_comm else radii):      # (the stand-in comm: two radii per world, R = 3 among them)
                for inject in (False, True):
                    g = torch.Generator().manual_seed(10 * K + R)
                    q, k, v = (torch.randn(3 * K, S, D, generator=g) for _ in range(3))
                    cover = R >= K - 1
                    full = (fake.ext_attn(q, k, v, h, d ** -0.5, inject) if cover
                            else fake.ext_attn_windows(q, k, v, h, d ** -0.5, inject, fake.bank_windows(K, R)))
                    fake.calls.clear()
                    out = sh.pivotal_attention(loc(q), loc(k), loc(v), h, d ** -0.5, inject, window=R)
                    what = f"K{K} W{world} R{R} inject={inject} comm={use_comm} rank {rank}"
                    if not torch.equal(out, loc(full)):
                        bad.append(f"{what}: max abs err {float((out - loc(full)).abs().max()):.3e}")
                    packs = [c for c in fake.calls if c[0] == "window_halo_pack"]
                    if cover:
                        if packs:
                            bad.append(f"{what}: a covering radius must issue today's pass")
                        continue
                    plan = sharded.window_halo_plan(K, world, rank, R)
                    if packs != [("window_halo_pack", 3 if inject else 4, tuple(plan.send))]:
                        bad.append(f"{what}: packs {packs}")
                    wins = [c for c in fake.calls if c[0] == "ext_attn_windows_views"]
                    if len(wins) != 1 or wins[0][2][1] != plan.F or wins[0][4:] != (tuple(plan.windows), "bank", plan.hl):
                        bad.append(f"{what}: windowed calls {wins}")
            for kw in (dict(window=1, n_edits=2), dict(window=-1)):
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


@pytest.mark.parametrize("world,K,radii", [(2, 5, (0, 1, 4)), (3, 7, (1, 2, 3, 6))])
def test_windowed_shard_equals_the_single_process_windowed_attention(world, K, radii):
    """K = 5 over 2 ranks (3, 2) and K = 7 over 3 (3, 2, 2): uneven shards; R = 3 spans two ranks; R = K - 1 covers the bank."""
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), K, radii, ret), nprocs=world, join=True)
    assert dict(ret) == {r: [] for r in range(world)}, dict(ret)


def _hooks_worker(rank, world, port, K, ret):
    _init(rank, world, port)
    try:
        import tokenflow_utils as tfu
        from tests import fake_diffusers as fd
        from tests.shard_window_fake_ops import ShardWindowFakeOps
        from tokenflow_amd import hooks, sharded
        torch.set_num_threads(1)
        fake = ShardWindowFakeOps()
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
            _, attn = pipe(None)
            want = attn(x.reshape(3 * K, S, D)).view(3, K, S, D).clone()
            sh = sharded.FrameShard(K)
            lo, hi = sh.kf0, sh.kf0 + sh.Kl
            xl = x[:, lo:hi].reshape(3 * sh.Kl, S, D)
            _, attn = pipe(sh, shard=True)
            got = attn(xl).view(3, sh.Kl, S, D)
            if not torch.equal(got, want[:, lo:hi]):
                bad.append(f"the opt-in pass: max abs err {float((got - want[:, lo:hi]).abs().max()):.3e}")
            if not any(c[0] == "ext_attn_windows_views" for c in fake.calls):
                bad.append("the opt-in pass issued no windowed shard call")

            def refused(what, needle, setup, **kw):
                p, a = pipe(sh, **kw)
                setup(p, a)
                try:
                    a(xl)
                    bad.append(f"{what}: no ValueError")
                except ValueError as e:
                    if needle not in str(e):
                        bad.append(f"{what}: {e}")
            refused("without shard=True", "a sliding-window bank on a registered frame shard is not supported", lambda p, a: None)
            refused("anchors", "anchor keyframes on a registered frame shard", lambda p, a: None, shard=True, anchors=[0])
            refused("segments", "keyframe segments", lambda p, a: setattr(a, "keyframe_segments", (1, 1)), shard=True)
            refused("edits", "one edit", lambda p, a: setattr(a, "n_edits", 2), shard=True)

            class Plain:      # a shard type without window= support: the existing error
                world, rank, K, Kl, kf0 = sh.world, sh.rank, sh.K, sh.Kl, sh.kf0
            p, a = pipe(sh, shard=True)
            a.__dict__["_tf_shard"] = Plain()
            try:
                a(xl)
                bad.append("a shard type without window=: no ValueError")
            except ValueError as e:
                if "on a registered frame shard is not supported" not in str(e):
                    bad.append(str(e))
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_hooks_opt_in_two_ranks():
    ret = mp.Manager().dict()
    mp.spawn(_hooks_worker, args=(2, _free_port(), 4, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)
