"""Host logic of the sliding-window bank in a multi-edit batch (`register_edits(model, E)` beside
`register_bank_window(model, radius, edits=True)`) on the CPU over oracle-backed ops (tests/window_edit_fake_ops.py): the
pivotal pass is ONE `ops.ext_attn_windows_edits` with the windows, the edit count and the per-edit injection mask of the step;
propagation is untouched; without the keyword the combination raises as it always did."""
import pytest
import torch

import tokenflow_utils as tfu
from oracle import golden_cases as gc
from oracle import tokenflow_oracle as orc
from tests import edit_forms as ef
from tests import fake_diffusers as fd
from tests.window_edit_fake_ops import WindowEditFakeOps, bank_windows
from tokenflow_amd import hooks

K, N, S, E = 5, 2, 16, 2
B = 1 + 2 * E


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


def _x(blk, frames, seed, branches=B):
    D = blk.norm1.normalized_shape[0]
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(branches * frames, S, D, generator=g),
            torch.randn(branches * frames, 7, gc.BLOCKS_CFG["cross_dim"], generator=g))


def _top(calls):
    return [c for c in calls if c[0] not in ("nn_search", "gather_blend")]


def test_register_bank_window_edits_sets_and_clears_state():
    pipe = _pipe()
    blocks = [b for _, b in pipe.unet.transformer_blocks_in_order()]
    tfu.register_bank_window(pipe, 2, edits=True)
    assert len(blocks) == 16
    assert all(m.bank_window == 2 and m.bank_window_edits is True for b in blocks for m in (b, b.attn1))
    tfu.register_bank_window(pipe, 2)                                    # the keyword is per call: the plain call closes it again
    assert all(m.bank_window == 2 and m.bank_window_edits is False for b in blocks for m in (b, b.attn1))
    tfu.register_bank_window(pipe, 1, edits=True)
    tfu.register_bank_window(pipe, None)
    assert all(m.bank_window is None and not m.bank_window_edits for b in blocks for m in (b, b.attn1))
    tfu.register_bank_window(pipe, None, edits=True)                     # no window: nothing to open
    assert all(m.bank_window is None and not m.bank_window_edits for b in blocks for m in (b, b.attn1))
    assert tfu.register_bank_window is hooks.register_bank_window


@pytest.mark.parametrize("mode", ["shared", "schedules", "sdedit"])
@pytest.mark.parametrize("radius", [0, 1, 2])
def test_pivotal_pass_routes_to_the_windowed_multi_edit_op(monkeypatch, mode, radius):
    """One injecting block: the routing and the arguments of the call (windows, E, mask), the result per edit and per frame
    against the oracle on the window's slices of the q, k, v the block handed to the op; the chunk passes that follow are the
    unwindowed multi-edit ones."""
    pipe = _pipe(pnp=mode != "sdedit")
    tfu.register_edits(pipe, E)
    tfu.register_bank_window(pipe, radius, edits=True)
    if mode == "schedules":
        tfu.register_edit_schedules(pipe, qk_schedules=[[801], []])     # only edit 0 injects at t = 801
    want_mask = {"shared": (1 << E) - 1, "schedules": 0b01, "sdedit": 0}[mode]
    blk = _block(pipe)
    x_piv, enc_piv = _x(blk, K, 1)
    D, heads, scale = x_piv.shape[-1], blk.attn1.heads, blk.attn1.scale
    ops = WindowEditFakeOps()
    seen = []
    real = ops.ext_attn_windows_edits

    def spy(q, k, v, *a, **kw):
        out = real(q, k, v, *a, **kw)
        seen.append((q.float().clone(), k.float().clone(), v.float().clone(), out.float().clone()))
        return out
    ops.ext_attn_windows_edits = spy
    monkeypatch.setattr(hooks, "ops", ops)
    wins = tuple(bank_windows(K, radius))
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        blk(x_piv, encoder_hidden_states=enc_piv)
        assert ops.calls == [("ext_attn_windows_edits", (B * K, S, D), E, want_mask, wins)]
        (q, k, v, out), = seen
        whole = []
        for e in range(E):
            inj = bool((want_mask >> e) & 1)
            q3, k3, v3, o3 = (ef.edit_slice(t, e, E) for t in (q, k, v, out))
            for i, (lo, n) in enumerate(wins):
                sl = lambda t: t.view(3, K, S, D)[:, lo:lo + n].reshape(3 * n, S, D)      # noqa: E731
                ref = orc.ext_attn_core(sl(q3), sl(k3), sl(v3), heads, scale, inj).view(3, n, S, D)[:, i - lo]
                assert torch.allclose(o3.view(3, K, S, D)[:, i], ref, rtol=1e-5, atol=1e-6), (e, i)
            whole.append(torch.allclose(o3, orc.ext_attn_core(q3, k3, v3, heads, scale, inj), rtol=1e-3, atol=1e-4))
        assert not any(whole)      # radius < K - 1: not the whole-bank attention, for any edit
        # propagation is untouched: the multi-edit chunk ops of an unwindowed pass
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


def test_without_the_keyword_the_combination_raises(monkeypatch):
    monkeypatch.setattr(hooks, "ops", WindowEditFakeOps())
    pipe = _pipe()
    tfu.register_edits(pipe, E)
    tfu.register_pivotal(pipe, True)
    blk = _block(pipe)
    x, enc = _x(blk, K, 1)
    for args, kw in (((1,), {}), ((1,), {"edits": False}), ((1, False), {})):
        tfu.register_bank_window(pipe, *args, **kw)
        with torch.no_grad(), pytest.raises(ValueError, match="register_bank_window.*multi-edit.*edits=True"):
            blk(x, encoder_hidden_states=enc)
    tfu.register_bank_window(pipe, 1, edits=True)
    with torch.no_grad():
        blk(x, encoder_hidden_states=enc)                           # opted in: the pass runs


def test_still_refused_with_the_keyword(monkeypatch):
    monkeypatch.setattr(hooks, "ops", WindowEditFakeOps())
    pipe = _pipe()
    tfu.register_edits(pipe, E)
    tfu.register_bank_window(pipe, 1, edits=True)
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
        blk(x, encoder_hidden_states=enc)

        # graph capture of a multi-edit pass
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(ValueError, match="graphs.py"):
            blk(x, encoder_hidden_states=enc)


@pytest.mark.parametrize("radius", [K - 1, K + 2])
@pytest.mark.parametrize("edits", [False, True])
def test_covering_radius_issues_exactly_the_multi_edit_ops(monkeypatch, radius, edits):
    traces = []
    for registered in (False, True):
        pipe = _pipe()
        tfu.register_edits(pipe, E)
        if registered:
            tfu.register_bank_window(pipe, radius, edits=edits)
        ops = WindowEditFakeOps()
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
    assert not any(c[0] == "ext_attn_windows_edits" for c in traces[1][0])
    assert all(torch.equal(a, b) for a, b in zip(traces[0][1], traces[1][1]))


def test_one_edit_with_the_keyword_is_the_single_edit_window(monkeypatch):
    """E = 1: the keyword opens nothing -- the pass is the `ops.ext_attn_windows` call of a plain register_bank_window."""
    pipe = _pipe()
    tfu.register_bank_window(pipe, 1, edits=True)
    ops = WindowEditFakeOps()
    from tests.window_fake_ops import WindowFakeOps
    ops.ext_attn_windows = lambda *a, **kw: WindowFakeOps.ext_attn_windows(ops, *a, **kw)
    monkeypatch.setattr(hooks, "ops", ops)
    blk = _block(pipe)
    x, enc = _x(blk, K, 1, branches=3)
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        blk(x, encoder_hidden_states=enc)
    assert [c[0] for c in ops.calls] == ["ext_attn_windows"]
