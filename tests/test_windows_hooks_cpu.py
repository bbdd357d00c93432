"""Host logic of the sliding-window bank hook path (`register_bank_window`) on the CPU over oracle-backed ops
(tests/window_fake_ops.py): in a pivotal pass keyframe i's uncond / cond branches attend to the keyframes i - R .. i + R only;
propagation and everything else are untouched, and a radius that covers the bank issues exactly the plain ops."""
import pytest
import torch

import tokenflow_utils as tfu
from oracle import golden_cases as gc
from oracle import tokenflow_oracle as orc
from tests import fake_diffusers as fd
from tests.window_fake_ops import WindowFakeOps, bank_windows
from tokenflow_amd import hooks

K, N, S = 5, 2, 16


def _pipe(pnp=True):
    cfg = gc.BLOCKS_CFG
    torch.manual_seed(cfg["seed"])
    pipe = fd.FakePipeline(dims=cfg["dims"], heads=cfg["heads"], cross_dim=cfg["cross_dim"]).eval()
    if pnp:
        tfu.register_extended_attention_pnp(pipe, [801])
    else:
        tfu.register_extended_attention(pipe)
    tfu.set_tokenflow(pipe.unet)
    tfu.register_time(pipe, 801)
    return pipe


def _block(pipe):
    return pipe.unet.up_blocks[2].attentions[0].transformer_blocks[0]      # one of the blocks that inject


def _x(blk, frames, seed):
    D = blk.norm1.normalized_shape[0]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3 * frames, S, D, generator=g), torch.randn(3 * frames, 7, gc.BLOCKS_CFG["cross_dim"], generator=g)


def _top(calls):
    return [c for c in calls if c[0] not in ("nn_search", "gather_blend")]


def test_register_bank_window_sets_and_clears_state():
    pipe = _pipe()
    blocks = [b for _, b in pipe.unet.transformer_blocks_in_order()]
    tfu.register_bank_window(pipe, 2)
    assert len(blocks) == 16 and all(b.bank_window == 2 and b.attn1.bank_window == 2 for b in blocks)
    tfu.register_bank_window(pipe, 0)
    assert all(b.attn1.bank_window == 0 for b in blocks)
    tfu.register_bank_window(pipe, None)
    assert all(b.bank_window is None and b.attn1.bank_window is None for b in blocks)
    with pytest.raises(ValueError):
        tfu.register_bank_window(pipe, -1)
    assert "register_bank_window" in hooks.__all__ and tfu.register_bank_window is hooks.register_bank_window


def test_fake_windows_are_the_clamped_symmetric_ones():
    from tokenflow_amd import ops
    for K_, R in ((6, 1), (6, 2), (5, 0), (5, 7), (1, 0), (25, 2)):
        assert ops.bank_windows(K_, R) == bank_windows(K_, R)


@pytest.mark.parametrize("radius", [None, K - 1, K + 2])
def test_full_radius_issues_exactly_the_plain_ops(monkeypatch, radius):
    traces = []
    for registered in (False, True):
        pipe = _pipe()
        if registered:
            tfu.register_bank_window(pipe, radius)
        ops = WindowFakeOps()
        monkeypatch.setattr(hooks, "ops", ops)
        blk = _block(pipe)
        outs = []
        with torch.no_grad():
            tfu.register_pivotal(pipe, True)
            outs.append(blk(*_x(blk, K, 1)[:1], encoder_hidden_states=_x(blk, K, 1)[1]))
            tfu.register_pivotal(pipe, False)
            for c in (0, 2):
                tfu.register_batch_idx(pipe, c)
                outs.append(blk(*_x(blk, N, 2 + c)[:1], encoder_hidden_states=_x(blk, N, 2 + c)[1]))
            tfu.register_batch_idx(pipe, range(K))
            outs.append(blk(*_x(blk, K * N, 9)[:1], encoder_hidden_states=_x(blk, K * N, 9)[1]))
        traces.append((ops.calls, outs))
    assert traces[0][0] == traces[1][0] and len(traces[0][0]) > 0
    assert not any(c[0] == "ext_attn_windows" for c in traces[1][0])
    assert all(torch.equal(a, b) for a, b in zip(traces[0][1], traces[1][1]))


@pytest.mark.parametrize("pnp", [True, False])
@pytest.mark.parametrize("radius", [0, 1, 2])
def test_pivotal_pass_is_the_per_frame_oracle_on_the_window_slices(monkeypatch, pnp, radius):
    """One injecting block: the attention of its pivotal pass against the oracle, frame by frame, on the window's slices of the
    q, k, v the block handed to the op; the chunk passes that follow are the unwindowed ones (chunk c blends keyframes c, c-1)."""
    pipe = _pipe(pnp)
    tfu.register_bank_window(pipe, radius)
    blk = _block(pipe)
    x_piv, enc_piv = _x(blk, K, 1)
    D, heads, scale = x_piv.shape[-1], blk.attn1.heads, blk.attn1.scale
    ops = WindowFakeOps()
    seen = []
    real = ops.ext_attn_windows

    def spy(q, k, v, *a, **kw):
        out = real(q, k, v, *a, **kw)
        seen.append((q.float().clone(), k.float().clone(), v.float().clone(), out.float().clone()))
        return out
    ops.ext_attn_windows = spy
    monkeypatch.setattr(hooks, "ops", ops)
    wins = tuple(bank_windows(K, radius))
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        blk(x_piv, encoder_hidden_states=enc_piv)
        assert ops.calls == [("ext_attn_windows", (3 * K, S, D), pnp, wins)]
        (q, k, v, out), = seen
        for i, (lo, n) in enumerate(wins):
            sl = lambda t: t.view(3, K, S, D)[:, lo:lo + n].reshape(3 * n, S, D)      # noqa: E731
            ref = orc.ext_attn_core(sl(q), sl(k), sl(v), heads, scale, pnp).view(3, n, S, D)[:, i - lo]
            assert torch.allclose(out.view(3, K, S, D)[:, i], ref, rtol=1e-5, atol=1e-6), i
        if radius < K - 1:      # not the full bank: some frame must differ from the whole-bank attention
            full = orc.ext_attn_core(q, k, v, heads, scale, pnp)
            assert not torch.allclose(out, full, rtol=1e-3, atol=1e-4)
        # propagation is untouched
        tfu.register_pivotal(pipe, False)
        for c in (0, 3):
            ops.calls.clear()
            tfu.register_batch_idx(pipe, c)
            xc, ec = _x(blk, N, 10 + c)
            blk(xc, encoder_hidden_states=ec)
            assert _top(ops.calls) == [("propagate", (N * S, D), (c,) if c == 0 else (c, c - 1))]
        ops.calls.clear()
        tfu.register_batch_idx(pipe, range(K))
        xr, er = _x(blk, K * N, 20)
        blk(xr, encoder_hidden_states=er)
        assert _top(ops.calls) == [("propagate_chunks", (K * N * S, D), K, 0, True)]


def test_unsupported_combinations_raise(monkeypatch):
    monkeypatch.setattr(hooks, "ops", WindowFakeOps())
    pipe = _pipe()
    tfu.register_bank_window(pipe, 1)
    tfu.register_pivotal(pipe, True)
    blk = _block(pipe)
    x, enc = _x(blk, K, 1)
    with torch.no_grad():
        blk(x, encoder_hidden_states=enc)                       # the supported path runs

        tfu.register_edits(pipe, 2)                             # a multi-edit batch
        with pytest.raises(ValueError, match="register_bank_window.*multi-edit"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_edits(pipe, 1)

        tfu.register_segments(pipe, [2, 3])                     # several keyframe segments
        with pytest.raises(ValueError, match="register_bank_window.*segments"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_segments(pipe, None)

        class _Shard:                                           # a registered frame shard
            world, Kl, kf0 = 2, 5, 0
        tfu.register_frame_shard(pipe.unet, _Shard())
        with pytest.raises(ValueError, match="register_bank_window.*frame shard"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_frame_shard(pipe.unet, None)
        blk(x, encoder_hidden_states=enc)

        # a radius that covers the bank is today's path: the combinations are today's business again
        tfu.register_bank_window(pipe, K - 1)
        tfu.register_segments(pipe, [2, 3])
        blk(x, encoder_hidden_states=enc)


def test_frame_shard_radius_is_held_against_the_whole_bank(monkeypatch):
    """On a shard the pass carries the rank's LOCAL keyframes (Kl = 5 of K = 10): a radius between Kl - 1 and K - 1 is a real
    window and must be refused, not dropped; only a radius that covers the shard's whole bank is today's path."""
    monkeypatch.setattr(hooks, "ops", WindowFakeOps())
    pipe = _pipe()
    tfu.register_pivotal(pipe, True)
    blk = _block(pipe)
    x, enc = _x(blk, K, 1)

    class _Shard:
        world, Kl, kf0, K = 2, 5, 0, 10

    class _NoK:
        world, Kl, kf0 = 2, 5, 0
    tfu.register_frame_shard(pipe.unet, _Shard())
    for radius in (1, 4, 8):                                    # 4 and 8: >= Kl - 1, < K - 1
        tfu.register_bank_window(pipe, radius)
        with torch.no_grad(), pytest.raises(ValueError, match="register_bank_window.*frame shard"):
            blk(x, encoder_hidden_states=enc)
        with pytest.raises(ValueError, match="frame shard"):
            hooks._bank_window(blk.attn1, 5)
    for radius in (9, 12, None):                                # covers the shard's bank: the sharded pass as it is today
        tfu.register_bank_window(pipe, radius)
        assert hooks._bank_window(blk.attn1, 5) is None and hooks._bank_window(blk, 5) is None
    class _One:                                                 # a world-1 shard is the unsharded pass: the window applies
        world, Kl, kf0, K = 1, 5, 0, 5
    tfu.register_frame_shard(pipe.unet, _One())
    tfu.register_bank_window(pipe, 1)
    assert hooks._bank_window(blk.attn1, 5) == 1 and hooks._active_shard(blk.attn1) is None
    tfu.register_frame_shard(pipe.unet, _NoK())                 # a shard type that does not tell its bank size: refused
    tfu.register_bank_window(pipe, 9)
    with pytest.raises(ValueError, match="frame shard"):
        hooks._bank_window(blk.attn1, 5)


def test_covering_radius_in_a_multi_edit_batch_issues_the_plain_ops(monkeypatch):
    """K = 5, E = 2: the batch holds 5 K = 25 frames; radius K - 1 covers the bank and must issue exactly the multi-edit ops of
    an unregistered run, while radius K - 2 is a real window and raises."""
    from tests.edit_forms import EditFakeOps
    E = 2
    traces = []
    for radius in (None, K - 1, K + 2):
        pipe = _pipe()
        tfu.register_edits(pipe, E)
        tfu.register_bank_window(pipe, radius)
        ops = EditFakeOps()
        monkeypatch.setattr(hooks, "ops", ops)
        blk = _block(pipe)
        D = blk.norm1.normalized_shape[0]
        g = torch.Generator().manual_seed(3)
        x = torch.randn((1 + 2 * E) * K, S, D, generator=g)
        enc = torch.randn((1 + 2 * E) * K, 7, gc.BLOCKS_CFG["cross_dim"], generator=g)
        with torch.no_grad():
            tfu.register_pivotal(pipe, True)
            out = blk(x, encoder_hidden_states=enc)
        traces.append((_top(ops.calls), out))
    assert traces[0][0] and traces[0][0][0][0] == "ext_attn_edits"
    assert all(t[0] == traces[0][0] and torch.equal(t[1], traces[0][1]) for t in traces[1:])
    tfu.register_bank_window(pipe, K - 2)
    with torch.no_grad(), pytest.raises(ValueError, match="register_bank_window.*multi-edit"):
        blk(x, encoder_hidden_states=enc)

