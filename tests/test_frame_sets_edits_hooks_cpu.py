"""Host logic of anchor keyframes in a multi-edit batch (`register_edits(model, E)` beside
`register_bank_window(model, radius, edits=True, anchors=..., anchor_edits=True)`) on the CPU over oracle-backed ops
(tests/frame_set_edit_fake_ops.py): the pivotal pass is ONE `ops.ext_attn_frame_sets_edits` with the frame sets, the edit count
and the per-edit injection mask of the step; propagation is untouched; a covering radius issues today's ops; without the
keyword the combination raises as before."""
import pytest
import torch

import tokenflow_utils as tfu
from oracle import tokenflow_oracle as orc
from tests import edit_forms as ef
from tests.frame_set_edit_fake_ops import FrameSetEditFakeOps, bank_frame_sets
from tests.test_windows_edits_hooks_cpu import B, E, K, N, S, _block, _pipe, _top, _x
from tokenflow_amd import hooks


def test_register_bank_window_anchor_edits_sets_and_clears_state():
    pipe = _pipe()
    blocks = [b for _, b in pipe.unet.transformer_blocks_in_order()]
    state = lambda: {(m.bank_window, m.bank_window_edits, m.bank_window_anchors, m.bank_window_anchor_edits)      # noqa: E731
                     for b in blocks for m in (b, b.attn1)}
    tfu.register_bank_window(pipe, 2, edits=True, anchors=[0, 3], anchor_edits=True)
    assert len(blocks) == 16 and state() == {(2, True, (0, 3), True)}
    tfu.register_bank_window(pipe, 2, edits=True, anchors=[0, 3])          # the keyword is per call: the plain call closes it again
    assert state() == {(2, True, (0, 3), False)}
    tfu.register_bank_window(pipe, 2, True, 4, True)                       # positional, beside the older parameters
    assert state() == {(2, True, 4, True)}
    tfu.register_bank_window(pipe, None, edits=True, anchors=[0], anchor_edits=True)      # no window: nothing to open
    assert state() == {(None, False, None, False)}
    hooks._set_bank_window(blocks, 1, True, (0,))                          # existing callers of the helper keep working
    assert state() == {(1, True, (0,), False)}
    hooks._set_bank_window(blocks, 1)
    assert state() == {(1, False, None, False)}


@pytest.mark.parametrize("mode", ["shared", "schedules", "sdedit"])
@pytest.mark.parametrize("radius,anchors", [(0, [4]), (1, [0]), (1, 2), (2, [0, 4])])
def test_pivotal_pass_routes_to_the_frame_set_multi_edit_op(monkeypatch, mode, radius, anchors):
    """One injecting block: the routing and the arguments of the call (sets, E, mask), the result per edit and per frame against
    the oracle on the gathered member slices of the q, k, v the block handed to the op; the chunk passes that follow are the
    multi-edit ones of a pass without window or anchors."""
    pipe = _pipe(pnp=mode != "sdedit")
    tfu.register_edits(pipe, E)
    tfu.register_bank_window(pipe, radius, edits=True, anchors=anchors, anchor_edits=True)
    if mode == "schedules":
        tfu.register_edit_schedules(pipe, qk_schedules=[[801], []])     # only edit 0 injects at t = 801
    want_mask = {"shared": (1 << E) - 1, "schedules": 0b01, "sdedit": 0}[mode]
    blk = _block(pipe)
    x_piv, enc_piv = _x(blk, K, 1)
    D, heads, scale = x_piv.shape[-1], blk.attn1.heads, blk.attn1.scale
    ops = FrameSetEditFakeOps()
    seen = []
    real = ops.ext_attn_frame_sets_edits

    def spy(q, k, v, *a, **kw):
        out = real(q, k, v, *a, **kw)
        seen.append((q.float().clone(), k.float().clone(), v.float().clone(), out.float().clone()))
        return out
    ops.ext_attn_frame_sets_edits = spy
    monkeypatch.setattr(hooks, "ops", ops)
    anc = list(range(0, K, anchors)) if isinstance(anchors, int) else anchors
    sets = tuple(bank_frame_sets(K, radius, anc))
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        blk(x_piv, encoder_hidden_states=enc_piv)
        assert ops.calls == [("ext_attn_frame_sets_edits", (B * K, S, D), E, want_mask, sets)]
        (q, k, v, out), = seen
        whole = []
        for e in range(E):
            inj = bool((want_mask >> e) & 1)
            q3, k3, v3, o3 = (ef.edit_slice(t, e, E) for t in (q, k, v, out))
            for i, m in enumerate(sets):
                fr = [f for f in range(K) if (m >> f) & 1]
                sl = lambda t: t.view(3, K, S, D)[:, fr].reshape(3 * len(fr), S, D)      # noqa: E731
                ref = orc.ext_attn_core(sl(q3), sl(k3), sl(v3), heads, scale, inj).view(3, len(fr), S, D)[:, fr.index(i)]
                assert torch.allclose(o3.view(3, K, S, D)[:, i], ref, rtol=1e-5, atol=1e-6), (e, i)
            whole.append(torch.allclose(o3, orc.ext_attn_core(q3, k3, v3, heads, scale, inj), rtol=1e-3, atol=1e-4))
        assert not any(whole)      # radius < K - 1: not the whole-bank attention, for any edit
        # propagation is untouched: the multi-edit chunk ops of a pass without window or anchors
        tfu.register_pivotal(pipe, False)
        for c in (0, 3):
            ops.calls.clear()
            tfu.register_batch_idx(pipe, c)
            xc, ec = _x(blk, N, 10 + c)
            blk(xc, encoder_hidden_states=ec)
            assert _top(ops.calls) == [("propagate_chunks_edits", (N * S, D), 1, c, c == 0, E)]
        ops.calls.clear()
        tfu.register_batch_idx(pipe, range(K))
        xr, er = _x(blk, K * N, 20)
        blk(xr, encoder_hidden_states=er)
        assert _top(ops.calls) == [("propagate_chunks_edits", (K * N * S, D), K, 0, True, E)]


def test_without_the_keyword_the_refusal_stands(monkeypatch):
    monkeypatch.setattr(hooks, "ops", FrameSetEditFakeOps())
    pipe = _pipe()
    tfu.register_edits(pipe, E)
    tfu.register_pivotal(pipe, True)
    blk = _block(pipe)
    x, enc = _x(blk, K, 1)
    with torch.no_grad():
        for kw in ({}, {"anchor_edits": False}):
            tfu.register_bank_window(pipe, 1, edits=True, anchors=[0], **kw)
            with pytest.raises(ValueError, match="register_bank_window: anchor keyframes in a multi-edit batch.*anchor_edits=True"):
                blk(x, encoder_hidden_states=enc)
        # the new keyword does not open the window itself: edits=True is still needed
        tfu.register_bank_window(pipe, 1, anchors=[0], anchor_edits=True)
        with pytest.raises(ValueError, match="register_bank_window.*multi-edit.*edits=True"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_bank_window(pipe, 1, edits=True, anchors=[0], anchor_edits=True)
        blk(x, encoder_hidden_states=enc)                           # opted in: the pass runs
        assert [c[0] for c in hooks.ops.calls] == ["ext_attn_frame_sets_edits"]
        # without anchors the keyword opens nothing: the windowed multi-edit op, as before
        hooks.ops.calls.clear()
        tfu.register_bank_window(pipe, 1, edits=True, anchor_edits=True)
        blk(x, encoder_hidden_states=enc)
        assert [c[0] for c in hooks.ops.calls] == ["ext_attn_windows_edits"]
        # an anchor outside the pass
        tfu.register_bank_window(pipe, 1, edits=True, anchors=[K], anchor_edits=True)
        with pytest.raises(ValueError, match="anchors="):
            blk(x, encoder_hidden_states=enc)


def test_still_refused_with_the_keyword(monkeypatch):
    monkeypatch.setattr(hooks, "ops", FrameSetEditFakeOps())
    pipe = _pipe()
    tfu.register_edits(pipe, E)
    tfu.register_bank_window(pipe, 1, edits=True, anchors=[0], anchor_edits=True)
    tfu.register_pivotal(pipe, True)
    blk = _block(pipe)
    x, enc = _x(blk, K, 1)
    with torch.no_grad():
        blk(x, encoder_hidden_states=enc)                           # the supported path runs

        tfu.register_segments(pipe, [2, 3])                         # several keyframe segments
        with pytest.raises(ValueError, match="segments"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_segments(pipe, None)

        class _Shard:                                               # a registered frame shard (one that runs multi-edit batches)
            world, Kl, kf0, K, supports_edits = 2, 5, 0, 10, True
        tfu.register_frame_shard(pipe.unet, _Shard())
        with pytest.raises(ValueError, match="register_bank_window.*frame shard"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_frame_shard(pipe.unet, None)

        blk.use_ada_layer_norm_zero = True                          # the AdaLayerNormZero gated path of a multi-edit batch
        with pytest.raises(ValueError, match="AdaLayerNormZero"):
            blk(x, encoder_hidden_states=enc)
        blk.use_ada_layer_norm_zero = False
        blk(x, encoder_hidden_states=enc)

        # graph capture of a multi-edit pass
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(ValueError, match="graphs.py"):
            blk(x, encoder_hidden_states=enc)


@pytest.mark.parametrize("radius", [K - 1, K + 2])
def test_covering_radius_issues_exactly_the_multi_edit_ops(monkeypatch, radius):
    traces = []
    for registered in (False, True):
        pipe = _pipe()
        tfu.register_edits(pipe, E)
        if registered:
            tfu.register_bank_window(pipe, radius, edits=True, anchors=[0, 2], anchor_edits=True)
        ops = FrameSetEditFakeOps()
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
    assert traces[0][0] == traces[1][0] and traces[0][0][0][0] == "ext_attn_edits"
    assert not any(c[0] in ("ext_attn_frame_sets_edits", "ext_attn_windows_edits") for c in traces[1][0])
    assert all(torch.equal(a, b) for a, b in zip(traces[0][1], traces[1][1]))


def test_one_edit_with_the_keyword_is_the_single_edit_anchored_pass(monkeypatch):
    """E = 1: the keyword opens nothing -- the pass is the `ops.ext_attn_frame_sets` call of register_bank_window(anchors=...)."""
    from tests.frame_set_fake_ops import FrameSetFakeOps
    pipe = _pipe()
    tfu.register_bank_window(pipe, 1, edits=True, anchors=[0], anchor_edits=True)
    ops = FrameSetEditFakeOps()
    ops.ext_attn_frame_sets = lambda *a, **kw: FrameSetFakeOps.ext_attn_frame_sets(ops, *a, **kw)
    monkeypatch.setattr(hooks, "ops", ops)
    blk = _block(pipe)
    x, enc = _x(blk, K, 1, branches=3)
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        blk(x, encoder_hidden_states=enc)
    assert [c[0] for c in ops.calls] == ["ext_attn_frame_sets"]
