"""Host logic of the anchored sliding-window hook path (`register_bank_window(model, radius, anchors=...)`) on the CPU over
oracle-backed ops (tests/frame_set_fake_ops.py): in a pivotal pass keyframe i's uncond / cond branches attend to the keyframes
i - R .. i + R and to the anchor keyframes; without anchors the windowed op is issued as before, a radius that covers the bank
issues exactly the plain ops whatever the anchors, and propagation is untouched."""
import pytest
import torch

import tokenflow_utils as tfu
from oracle import golden_cases as gc
from oracle import tokenflow_oracle as orc
from tests import fake_diffusers as fd
from tests.frame_set_fake_ops import FrameSetFakeOps, bank_frame_sets
from tests.window_fake_ops import bank_windows
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


def test_register_bank_window_stores_and_clears_the_anchors():
    pipe = _pipe()
    blocks = [b for _, b in pipe.unet.transformer_blocks_in_order()]
    tfu.register_bank_window(pipe, 2, anchors=[0, 7])
    assert len(blocks) == 16
    assert all(m.bank_window == 2 and m.bank_window_anchors == (0, 7) for b in blocks for m in (b, b.attn1))
    tfu.register_bank_window(pipe, 1, anchors=8)
    assert all(m.bank_window == 1 and m.bank_window_anchors == 8 for b in blocks for m in (b, b.attn1))
    for none in (None, [], ()):
        tfu.register_bank_window(pipe, 1, anchors=none)
        assert all(m.bank_window == 1 and m.bank_window_anchors is None for b in blocks for m in (b, b.attn1))
    tfu.register_bank_window(pipe, 2)                          # the old signature: no anchors
    assert all(b.attn1.bank_window_anchors is None and not b.attn1.bank_window_edits for b in blocks)
    tfu.register_bank_window(pipe, None, anchors=[0])          # no window: nothing to anchor
    assert all(m.bank_window is None and m.bank_window_anchors is None for b in blocks for m in (b, b.attn1))
    for bad in (0, -2, [-1], [0.5], "ab", 1.5):
        with pytest.raises(ValueError, match="register_bank_window"):
            tfu.register_bank_window(pipe, 1, anchors=bad)
    assert "register_bank_window" in hooks.__all__ and tfu.register_bank_window is hooks.register_bank_window


def test_fake_frame_sets_are_the_window_plus_the_anchors():
    from tokenflow_amd import ops
    for K_, R, anc in ((6, 1, [0]), (6, 1, [0, 5]), (6, 2, []), (5, 0, [2, 2]), (5, 7, [1]), (25, 2, range(0, 25, 8))):
        assert ops.bank_frame_sets(K_, R, anc) == bank_frame_sets(K_, R, anc)
    assert bank_frame_sets(6, 1, [0]) == [0b11, 0b111, 0b1111, 0b11101, 0b111001, 0b110001]
    for bad in ([6], [-1]):
        with pytest.raises(ValueError):
            ops.bank_frame_sets(6, 1, bad)


@pytest.mark.parametrize("pnp", [True, False])
@pytest.mark.parametrize("radius,anchors,resolved", [(1, [0], (0,)), (1, (4, 0), (0, 4)), (0, 2, (0, 2, 4)), (1, 3, (0, 3)), (1, 1, (0, 1, 2, 3, 4))])
def test_pivotal_pass_is_one_frame_set_call_on_the_expected_masks(monkeypatch, pnp, radius, anchors, resolved):
    """One injecting block: ONE `ext_attn_frame_sets` per pivotal pass, with the masks of the window plus the resolved anchors (a
    sequence, or an int stride: every m-th keyframe); each frame against the oracle on the gathered slices of the q, k, v the
    block handed to the op; the chunk passes that follow are the usual ones."""
    pipe = _pipe(pnp)
    tfu.register_bank_window(pipe, radius, anchors=anchors)
    blk = _block(pipe)
    x_piv, enc_piv = _x(blk, K, 1)
    D, heads, scale = x_piv.shape[-1], blk.attn1.heads, blk.attn1.scale
    ops = FrameSetFakeOps()
    seen = []
    real = ops.ext_attn_frame_sets

    def spy(q, k, v, *a, **kw):
        out = real(q, k, v, *a, **kw)
        seen.append((q.float().clone(), k.float().clone(), v.float().clone(), out.float().clone()))
        return out
    ops.ext_attn_frame_sets = spy
    monkeypatch.setattr(hooks, "ops", ops)
    sets = tuple(bank_frame_sets(K, radius, resolved))
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        blk(x_piv, encoder_hidden_states=enc_piv)
        assert ops.calls == [("ext_attn_frame_sets", (3 * K, S, D), pnp, sets)]
        (q, k, v, out), = seen
        for i, m in enumerate(sets):
            fr = [f for f in range(K) if (m >> f) & 1]
            sl = lambda t: t.view(3, K, S, D)[:, fr].reshape(3 * len(fr), S, D)      # noqa: E731
            ref = orc.ext_attn_core(sl(q), sl(k), sl(v), heads, scale, pnp).view(3, len(fr), S, D)[:, fr.index(i)]
            assert torch.allclose(out.view(3, K, S, D)[:, i], ref, rtol=1e-5, atol=1e-6), i
        if any(m != (1 << K) - 1 for m in sets):      # not the full bank: some frame must differ from the whole-bank attention
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


def _trace(monkeypatch, register):
    pipe = _pipe()
    register(pipe)
    ops = FrameSetFakeOps()
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
    return ops.calls, outs


@pytest.mark.parametrize("none", [None, [], ()])
def test_no_anchors_issue_the_windowed_op_as_before(monkeypatch, none):
    old = _trace(monkeypatch, lambda pipe: tfu.register_bank_window(pipe, 1))
    new = _trace(monkeypatch, lambda pipe: tfu.register_bank_window(pipe, 1, anchors=none))
    assert old[0] == new[0] and old[0][0][0] == "ext_attn_windows" and old[0][0][3] == tuple(bank_windows(K, 1))
    assert not any(c[0] == "ext_attn_frame_sets" for c in new[0])
    assert all(torch.equal(a, b) for a, b in zip(old[1], new[1]))


@pytest.mark.parametrize("radius", [K - 1, K + 2])
@pytest.mark.parametrize("anchors", [[0], 2, [0, 99]])
def test_covering_radius_issues_exactly_the_plain_ops_whatever_the_anchors(monkeypatch, radius, anchors):
    plain = _trace(monkeypatch, lambda pipe: None)
    cov = _trace(monkeypatch, lambda pipe: tfu.register_bank_window(pipe, radius, anchors=anchors))
    assert plain[0] == cov[0] and len(plain[0]) > 0
    assert not any(c[0] in ("ext_attn_windows", "ext_attn_frame_sets") for c in cov[0])
    assert all(torch.equal(a, b) for a, b in zip(plain[1], cov[1]))


def test_unsupported_combinations_raise(monkeypatch):
    monkeypatch.setattr(hooks, "ops", FrameSetFakeOps())
    pipe = _pipe()
    tfu.register_pivotal(pipe, True)
    blk = _block(pipe)
    x, enc = _x(blk, K, 1)
    with torch.no_grad():
        tfu.register_bank_window(pipe, 1, anchors=[0, K - 1])
        blk(x, encoder_hidden_states=enc)                       # the supported path runs

        for bad in ([K], [0, K + 3]):                           # an anchor outside the pass: resolved against K here
            tfu.register_bank_window(pipe, 1, anchors=bad)
            with pytest.raises(ValueError, match=r"register_bank_window: anchors=.*pivotal pass of 5 keyframes"):
                blk(x, encoder_hidden_states=enc)
            with pytest.raises(ValueError, match="register_bank_window"):
                hooks._bank_anchors(blk.attn1, K)
        tfu.register_bank_window(pipe, 1, anchors=[0])

        tfu.register_segments(pipe, [2, 3])                     # several keyframe segments: the window's own refusal
        with pytest.raises(ValueError, match="register_bank_window.*segments"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_segments(pipe, None)

        class _Shard:                                           # a registered frame shard: the window's own refusal
            world, Kl, kf0 = 2, 5, 0
        tfu.register_frame_shard(pipe.unet, _Shard())
        with pytest.raises(ValueError, match="register_bank_window.*frame shard"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_frame_shard(pipe.unet, None)
        blk(x, encoder_hidden_states=enc)


def test_anchors_in_a_multi_edit_batch_raise(monkeypatch):
    """E = 2: without edits=True the window's own refusal stands, message and all; with it the windowed multi-edit pass runs
    without anchors and raises with them; a covering radius is the plain multi-edit pass whatever the anchors."""
    from tests.window_edit_fake_ops import WindowEditFakeOps
    E = 2
    monkeypatch.setattr(hooks, "ops", WindowEditFakeOps())
    pipe = _pipe()
    tfu.register_edits(pipe, E)
    tfu.register_pivotal(pipe, True)
    blk = _block(pipe)
    D = blk.norm1.normalized_shape[0]
    g = torch.Generator().manual_seed(3)
    x = torch.randn((1 + 2 * E) * K, S, D, generator=g)
    enc = torch.randn((1 + 2 * E) * K, 7, gc.BLOCKS_CFG["cross_dim"], generator=g)
    with torch.no_grad():
        tfu.register_bank_window(pipe, 1, anchors=[0])
        with pytest.raises(ValueError, match="register_bank_window.*multi-edit.*opt-in"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_bank_window(pipe, 1, edits=True)
        blk(x, encoder_hidden_states=enc)
        tfu.register_bank_window(pipe, 1, edits=True, anchors=[0])
        with pytest.raises(ValueError, match="register_bank_window: anchor keyframes in a multi-edit batch"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_bank_window(pipe, K - 1, edits=True, anchors=[0])
        blk(x, encoder_hidden_states=enc)
