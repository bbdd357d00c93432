"""Host logic of the keyframe-segment hook path (`register_segments`) on the CPU over oracle-backed ops
(tests/segment_fake_ops.py): one pass carries V scenes, and for every op the slices of segment v are what the single-clip
path computes on segment v's tensors alone."""
import copy

import pytest
import torch

import tokenflow_utils as tfu
from oracle import golden_cases as gc
from tests import fake_diffusers as fd
from tests.segment_fake_ops import SegmentFakeOps
from tokenflow_amd import hooks

SEGS = (2, 3)
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
    """The ops the hooks called (FakeOps.propagate records its inner search and gather too)."""
    return [c for c in calls if c[0] not in ("nn_search", "gather_blend")]


def _window(x, frames, f0, f1):
    return x.view(3, frames, *x.shape[1:])[:, f0:f1].reshape(3 * (f1 - f0), *x.shape[1:])


def test_register_segments_sets_and_clears_state():
    pipe = _pipe()
    blocks = [b for _, b in pipe.unet.transformer_blocks_in_order()]
    tfu.register_segments(pipe, [2, 3])
    assert len(blocks) == 16 and all(b.keyframe_segments == (2, 3) and b.attn1.keyframe_segments == (2, 3) for b in blocks)
    for clear in (None, [5]):
        tfu.register_segments(pipe, [1, 4])
        tfu.register_segments(pipe, clear)
        assert all(b.keyframe_segments is None and b.attn1.keyframe_segments is None for b in blocks)
    for bad in ([], [1] * 9, [2, 0], [-1, 3]):
        with pytest.raises(ValueError):
            tfu.register_segments(pipe, bad)
    assert "register_segments" in hooks.__all__ and tfu.register_segments is hooks.register_segments


@pytest.mark.parametrize("clear", [None, [K]])
def test_one_segment_issues_exactly_the_single_shot_ops(monkeypatch, clear):
    traces = []
    for registered in (False, True):
        pipe = _pipe()
        if registered:
            tfu.register_segments(pipe, clear)
        ops = SegmentFakeOps()
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
    assert not any(c[0].endswith("_segments") for c in traces[1][0])
    assert all(torch.equal(a, b) for a, b in zip(traces[0][1], traces[1][1]))


def _single_clip_reference(pnp, x_piv, enc_piv, chunk_inputs, monkeypatch):
    """Two separate single-clip runs of the same block: segment v's pivotal pass, then its chunks with LOCAL indices."""
    outs_piv, outs_chunk = [], {}
    f0 = 0
    for Kv in SEGS:
        pipe = _pipe(pnp)
        monkeypatch.setattr(hooks, "ops", SegmentFakeOps())
        blk = _block(pipe)
        with torch.no_grad():
            tfu.register_pivotal(pipe, True)
            outs_piv.append(blk(_window(x_piv, K, f0, f0 + Kv), encoder_hidden_states=_window(enc_piv, K, f0, f0 + Kv)))
            tfu.register_pivotal(pipe, False)
            for c in range(Kv):
                tfu.register_batch_idx(pipe, c)
                x, enc = chunk_inputs[f0 + c]
                outs_chunk[f0 + c] = blk(x, encoder_hidden_states=enc)
        f0 += Kv
    return outs_piv, outs_chunk


@pytest.mark.parametrize("pnp", [True, False])
def test_per_chunk_passes_and_runs(monkeypatch, pnp):
    pipe = _pipe(pnp)
    tfu.register_segments(pipe, SEGS)
    blk = _block(pipe)
    x_piv, enc_piv = _x(blk, K, 1)
    chunk_inputs = {c: _x(blk, N, 10 + c) for c in range(K)}
    D = x_piv.shape[-1]
    ops = SegmentFakeOps()
    monkeypatch.setattr(hooks, "ops", ops)
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        out_piv = blk(x_piv, encoder_hidden_states=enc_piv)
        assert ops.calls == [("ext_attn_segments", (3 * K, S, D), pnp, SEGS)]
        kf_cached = blk.kf_attn_output.reshape(3, K, S, D)
        tfu.register_pivotal(pipe, False)
        # one chunk per pass: chunks 0 and 2 start a segment (one keyframe), the others blend [c, c-1]
        per_chunk = {}
        for c in range(K):
            ops.calls.clear()
            tfu.register_batch_idx(pipe, c)
            per_chunk[c] = blk(chunk_inputs[c][0], encoder_hidden_states=chunk_inputs[c][1])
            ids = (c,) if c in (0, 2) else (c, c - 1)
            assert _top(ops.calls) == [("propagate", (N * S, D), ids)]
            assert torch.equal(blk.attn_output, kf_cached[:, list(ids)])
        # runs of chunks: the whole video (bits 0 and 2), a run that starts mid-video (chunk 2 is bit 1), a run inside a segment
        runs = {}
        for run, mask in ((range(0, 5), 0b00101), (range(1, 4), 0b010), (range(3, 5), 0b00), (range(2, 5), 0b001)):
            ops.calls.clear()
            tfu.register_batch_idx(pipe, run)
            x = torch.cat([chunk_inputs[c][0].view(3, N, S, D) for c in run], dim=1).reshape(-1, S, D)
            enc = torch.cat([chunk_inputs[c][1].view(3, N, 7, -1) for c in run], dim=1).reshape(3 * N * len(run), 7, -1)
            runs[run] = blk(x, encoder_hidden_states=enc)
            assert _top(ops.calls) == [("propagate_chunks_segments", (len(run) * N * S, D), len(run), run[0], mask)]
            lo = run[0] if mask & 1 else run[0] - 1
            assert torch.equal(blk.attn_output, kf_cached[:, list(range(run[-1], lo - 1, -1))])
    # against two separate single-clip runs of the same block
    ref_piv, ref_chunk = _single_clip_reference(pnp, x_piv, enc_piv, chunk_inputs, monkeypatch)
    got_piv = out_piv.view(3, K, S, D)
    assert torch.equal(got_piv[:, :2].reshape(-1, S, D), ref_piv[0]) and torch.equal(got_piv[:, 2:].reshape(-1, S, D), ref_piv[1])
    for c in range(K):
        assert torch.equal(per_chunk[c].float(), ref_chunk[c].float()), c
    for run, out in runs.items():
        out = out.view(3, len(run), N, S, D)
        for j, c in enumerate(run):
            assert torch.equal(out[:, j].reshape(-1, S, D).float(), ref_chunk[c].float()), (run, c)


def test_keyframe_count_must_match(monkeypatch):
    monkeypatch.setattr(hooks, "ops", SegmentFakeOps())
    pipe = _pipe()
    tfu.register_segments(pipe, [2, 2])
    blk = _block(pipe)
    x, enc = _x(blk, K, 1)
    tfu.register_pivotal(pipe, True)
    with torch.no_grad(), pytest.raises(ValueError, match="keyframes"):
        blk(x, encoder_hidden_states=enc)


def test_unsupported_combinations_raise(monkeypatch):
    monkeypatch.setattr(hooks, "ops", SegmentFakeOps())
    pipe = _pipe()
    tfu.register_segments(pipe, SEGS)
    tfu.register_pivotal(pipe, True)
    blk = _block(pipe)
    x, enc = _x(blk, K, 1)
    with torch.no_grad():
        blk(x, encoder_hidden_states=enc)                       # the supported path runs

        tfu.register_edits(pipe, 2)                             # a multi-edit batch
        with pytest.raises(ValueError, match="multi-edit"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_edits(pipe, 1)

        class _Shard:                                           # a registered frame shard
            world, Kl, kf0 = 2, 5, 0
        tfu.register_frame_shard(pipe.unet, _Shard())
        with pytest.raises(ValueError, match="frame shard"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_frame_shard(pipe.unet, None)
        blk(x, encoder_hidden_states=enc)

        ada = copy.copy(blk)                                    # the AdaLayerNormZero gated path
        ada.__dict__ = dict(blk.__dict__)
        ada.use_ada_layer_norm_zero = True
        with pytest.raises(ValueError, match="AdaLayerNormZero"):
            ada(x, encoder_hidden_states=enc)

        # capture for graphs.py replay
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(ValueError, match="graphs.py"):
            blk(x, encoder_hidden_states=enc)
