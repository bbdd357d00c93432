"""Host logic of the ragged chunk runs (`register_chunk_frames`) on the CPU over oracle-backed ops (tests/ragged_fake_ops.py): a
run pass over chunks of unequal frame count is ONE `ops.propagate_chunks_ragged`, and its rows are what the per-chunk passes
compute, each with its own frame count."""
import copy

import pytest
import torch

import tokenflow_utils as tfu
from oracle import golden_cases as gc
from tests import fake_diffusers as fd
from tests.ragged_fake_ops import RaggedFakeOps
from tokenflow_amd import hooks

K, S = 5, 16
FRAMES = (3, 1, 2, 2, 4)          # frames of every chunk of the video


def _pipe():
    cfg = gc.BLOCKS_CFG
    torch.manual_seed(cfg["seed"])
    pipe = fd.FakePipeline(dims=cfg["dims"], heads=cfg["heads"], cross_dim=cfg["cross_dim"]).eval()
    tfu.register_extended_attention_pnp(pipe, [801])
    tfu.set_tokenflow(pipe.unet)
    tfu.register_time(pipe, 801)
    return pipe


def _block(pipe):
    return pipe.unet.up_blocks[2].attentions[0].transformer_blocks[0]      # one of the blocks that inject


def _x(blk, nb, frames, seed):
    D = blk.norm1.normalized_shape[0]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(nb * frames, S, D, generator=g), torch.randn(nb * frames, 7, gc.BLOCKS_CFG["cross_dim"], generator=g)


def _top(calls):
    """The ops the hooks called (FakeOps.propagate records its inner search and gather too)."""
    return [c for c in calls if c[0] not in ("nn_search", "gather_blend")]


def _run_inputs(chunk_inputs, run, nb):
    D = chunk_inputs[0][0].shape[-1]
    x = torch.cat([chunk_inputs[c][0].view(nb, FRAMES[c], S, D) for c in run], dim=1).reshape(-1, S, D)
    enc = torch.cat([chunk_inputs[c][1].view(nb, FRAMES[c], 7, -1) for c in run], dim=1)
    return x, enc.reshape(x.shape[0], 7, -1)


def test_register_chunk_frames_sets_and_clears_state():
    pipe = _pipe()
    blocks = [b for _, b in pipe.unet.transformer_blocks_in_order()]
    tfu.register_chunk_frames(pipe, [8, 8, 3])
    assert len(blocks) == 16 and all(b.chunk_frames == (8, 8, 3) for b in blocks)
    tfu.register_chunk_frames(pipe, None)
    assert all(b.chunk_frames is None for b in blocks)
    for bad in ([], [2, 0], [-1, 3]):
        with pytest.raises(ValueError):
            tfu.register_chunk_frames(pipe, bad)
    assert "register_chunk_frames" in hooks.__all__ and tfu.register_chunk_frames is hooks.register_chunk_frames


@pytest.mark.parametrize("segs,E", [(None, 1), ((2, 3), 1), (None, 2)], ids=["plain", "segments", "two-edits"])
def test_ragged_runs_equal_the_per_chunk_passes(monkeypatch, segs, E):
    nb = 1 + 2 * E
    pipe = _pipe()
    tfu.register_edits(pipe, E)
    tfu.register_segments(pipe, segs)
    blk = _block(pipe)
    x_piv, enc_piv = _x(blk, nb, K, 1)
    chunk_inputs = {c: _x(blk, nb, FRAMES[c], 10 + c) for c in range(K)}
    D = x_piv.shape[-1]
    starts = {0} if segs is None else {0, segs[0]}
    ops = RaggedFakeOps()
    monkeypatch.setattr(hooks, "ops", ops)
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        blk(x_piv, encoder_hidden_states=enc_piv)
        kf_cached = blk.kf_attn_output.reshape(nb, K, S, D)
        tfu.register_pivotal(pipe, False)
        # the reference: one chunk per pass, each with its own frame count -- what a user has without the registration
        per_chunk = {}
        for c in range(K):
            tfu.register_batch_idx(pipe, c)
            per_chunk[c] = blk(chunk_inputs[c][0], encoder_hidden_states=chunk_inputs[c][1])
        tfu.register_chunk_frames(pipe, FRAMES)
        for c in (0, 3):          # one-chunk passes are untouched by the registration
            ops.calls.clear()
            tfu.register_batch_idx(pipe, c)
            assert torch.equal(blk(chunk_inputs[c][0], encoder_hidden_states=chunk_inputs[c][1]), per_chunk[c])
            assert not any(call[0] == "propagate_chunks_ragged" for call in ops.calls)
        for run in (range(0, 5), range(1, 4), range(2, 5), range(3, 5)):
            ops.calls.clear()
            tfu.register_batch_idx(pipe, run)
            x, enc = _run_inputs(chunk_inputs, run, nb)
            out = blk(x, encoder_hidden_states=enc)
            fr = tuple(FRAMES[c] for c in run)
            mask = sum(1 << j for j, c in enumerate(run) if c in starts)
            assert _top(ops.calls) == [("propagate_chunks_ragged", (sum(fr) * S, D), fr, run[0], mask, E)]
            lo = run[0] if mask & 1 else run[0] - 1
            assert torch.equal(blk.attn_output, kf_cached[:, list(range(run[-1], lo - 1, -1))])
            out = out.view(nb, sum(fr), S, D)
            f0 = 0
            for c in run:
                assert torch.equal(out[:, f0:f0 + FRAMES[c]].reshape(-1, S, D).float(), per_chunk[c].float()), (run, c)
                f0 += FRAMES[c]


def test_uniform_registration_leaves_todays_trace(monkeypatch):
    """A registration whose run is of equal chunks issues today's ops: the trace and the bits of the unregistered pass."""
    traces = []
    for registered in (False, True):
        pipe = _pipe()
        if registered:
            tfu.register_chunk_frames(pipe, [2] * K)
        ops = RaggedFakeOps()
        monkeypatch.setattr(hooks, "ops", ops)
        blk = _block(pipe)
        outs = []
        with torch.no_grad():
            tfu.register_pivotal(pipe, True)
            outs.append(blk(*_x(blk, 3, K, 1)[:1], encoder_hidden_states=_x(blk, 3, K, 1)[1]))
            tfu.register_pivotal(pipe, False)
            for run in (range(K), range(1, 4)):
                tfu.register_batch_idx(pipe, run)
                x, enc = _x(blk, 3, 2 * len(run), 9)
                outs.append(blk(x, encoder_hidden_states=enc))
        traces.append((ops.calls, outs))
    assert traces[0][0] == traces[1][0] and len(traces[0][0]) > 0
    assert not any(c[0] == "propagate_chunks_ragged" for c in traces[1][0])
    assert all(torch.equal(a, b) for a, b in zip(traces[0][1], traces[1][1]))
    # ... also inside a ragged registration, where the chunks of the run happen to be equal
    pipe = _pipe()
    tfu.register_chunk_frames(pipe, FRAMES)
    ops = RaggedFakeOps()
    monkeypatch.setattr(hooks, "ops", ops)
    blk = _block(pipe)
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        blk(*_x(blk, 3, K, 1)[:1], encoder_hidden_states=_x(blk, 3, K, 1)[1])
        tfu.register_pivotal(pipe, False)
        ops.calls.clear()
        tfu.register_batch_idx(pipe, range(2, 4))
        x, enc = _x(blk, 3, 4, 9)
        blk(x, encoder_hidden_states=enc)
    assert _top(ops.calls) == [("propagate_chunks", (4 * S, x.shape[-1]), 2, 2, False)]


def _after_pivotal(monkeypatch, frames=FRAMES):
    monkeypatch.setattr(hooks, "ops", RaggedFakeOps())
    pipe = _pipe()
    blk = _block(pipe)
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        blk(*_x(blk, 3, K, 1)[:1], encoder_hidden_states=_x(blk, 3, K, 1)[1])
        tfu.register_pivotal(pipe, False)
    if frames is not None:
        tfu.register_chunk_frames(pipe, frames)
    return pipe, blk


def test_without_registration_the_old_error_stays(monkeypatch):
    pipe, blk = _after_pivotal(monkeypatch, None)
    tfu.register_batch_idx(pipe, range(0, 3))
    x, enc = _x(blk, 3, 7, 2)
    with torch.no_grad(), pytest.raises(ValueError, match="7 frames per branch do not split into 3 chunks"):
        blk(x, encoder_hidden_states=enc)


def test_frame_count_must_match(monkeypatch):
    pipe, blk = _after_pivotal(monkeypatch)
    tfu.register_batch_idx(pipe, range(0, 3))              # chunks 0..2 hold 3 + 1 + 2 frames
    x, enc = _x(blk, 3, 7, 2)
    with torch.no_grad(), pytest.raises(ValueError, match="hold 6 frames"):
        blk(x, encoder_hidden_states=enc)
    tfu.register_chunk_frames(pipe, FRAMES[:2])            # a run past the registered chunks
    with torch.no_grad(), pytest.raises(ValueError, match="video of 2 chunks"):
        blk(*_x(blk, 3, 6, 2)[:1], encoder_hidden_states=_x(blk, 3, 6, 2)[1])


def test_unsupported_combinations_raise(monkeypatch):
    pipe, blk = _after_pivotal(monkeypatch)
    tfu.register_batch_idx(pipe, range(0, 3))
    x, enc = _x(blk, 3, 6, 2)
    with torch.no_grad():
        blk(x, encoder_hidden_states=enc)                       # the supported path runs

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

        tfu.register_segments(pipe, (2, 3))                     # segments together with several edits: refused as today
        tfu.register_edits(pipe, 2)
        with pytest.raises(ValueError, match="multi-edit"):
            blk(*_x(blk, 5, 6, 2)[:1], encoder_hidden_states=_x(blk, 5, 6, 2)[1])
        tfu.register_edits(pipe, 1)
        tfu.register_segments(pipe, None)

        # capture for graphs.py replay
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(ValueError, match="graphs.py"):
            blk(x, encoder_hidden_states=enc)
