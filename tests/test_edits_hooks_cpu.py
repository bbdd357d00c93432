"""Host logic of the multi-edit hook path (`register_edits`) on the CPU over oracle-backed ops (tests/edit_forms.py):
one pass carries E edits of one source video, B = 1 + 2E branches, and for every op and every block the slices of
edit e are what the single-edit path computes on [source | uncond_e | cond_e]."""
import copy

import pytest
import torch

import tokenflow_utils as tfu
from oracle import golden_cases as gc
from tests import edit_forms as ef
from tests import fake_diffusers as fd
from tests.fake_ops import FakeOps
from tokenflow_amd import hooks


def _exact_attn(out3, q3, k3, v3, heads, scale, inject, what):
    """Oracle-backed ops: the multi-edit op must return the oracle's own numbers for every edit."""
    from oracle import tokenflow_oracle as orc
    ref = orc.ext_attn_core(q3, k3, v3, heads, scale, inject)
    assert torch.equal(out3.float(), ref.to(out3.dtype).float()), what
    return 0.0


def _fake_indices(tgt, piv, inv, ids):
    return FakeOps().nn_search(tgt, piv, inv, ids)


@pytest.mark.parametrize("E", [2, 3])
def test_multi_edit_cfg1_dry_run(monkeypatch, E):
    """Steps 0 / 10 / 16 = q/k + feature injection / feature injection only / none.  Call counts do not multiply by E,
    every op call equals E oracle calls on its own inputs, NN-search inputs and indices equal the single-edit
    pipeline's, block outputs within 1e-5 of the output range of it."""
    ef.run_edits_cfg1(ef.EditFakeOps, torch.device("cpu"), monkeypatch, E, [0, 10, 16], _exact_attn, _fake_indices)


def _small_pipe():
    cfg = gc.BLOCKS_CFG
    torch.manual_seed(cfg["seed"])
    return fd.FakePipeline(dims=cfg["dims"], heads=cfg["heads"], cross_dim=cfg["cross_dim"]).eval()


def _trace(pipe, ops, monkeypatch):
    monkeypatch.setattr(hooks, "ops", ops)
    cfg = gc.BLOCKS_CFG
    blocks = [b for _, b in pipe.unet.transformer_blocks_in_order()]
    outs = []
    for t in cfg["timesteps"]:
        tfu.register_time(pipe, t)
        inp = gc.blocks_inputs(t)
        with torch.no_grad():
            tfu.register_pivotal(pipe, True)
            outs += [blk(x, encoder_hidden_states=inp["enc"]) for blk, x in zip(blocks, inp["pivotal"])]
            tfu.register_pivotal(pipe, False)
            for c in range(cfg["n_chunks"]):
                tfu.register_batch_idx(pipe, c)
                outs += [blk(x, encoder_hidden_states=inp["enc_n"]) for blk, x in zip(blocks, inp["chunks"][c])]
            outs.append(pipe.unet.up_blocks[1].resnets[1](inp["res_x"], inp["res_temb"]))
    return outs


def test_one_edit_issues_exactly_the_single_edit_ops(monkeypatch):
    """`register_edits(model, 1)` changes nothing: the recorded call trace of the plain oracle-backed ops (which have no
    *_edits op at all) and every output are those of a pipeline that never heard of edits."""
    cfg = gc.BLOCKS_CFG
    pipes = []
    for _ in range(2):
        pipe = _small_pipe()
        tfu.register_extended_attention_pnp(pipe, torch.tensor(cfg["schedule"]))
        tfu.register_conv_injection(pipe, torch.tensor(cfg["conv_schedule"]))
        tfu.set_tokenflow(pipe.unet)
        pipes.append(pipe)
    tfu.register_edits(pipes[1], 1)
    blk = pipes[1].unet.mid_block.attentions[0].transformer_blocks[0]
    assert blk.n_edits == 1 and blk.attn1.n_edits == 1 and pipes[1].unet.up_blocks[1].resnets[1].n_edits == 1
    a, b = FakeOps(), FakeOps()
    out_a, out_b = _trace(pipes[0], a, monkeypatch), _trace(pipes[1], b, monkeypatch)
    assert a.calls == b.calls and len(a.calls) > 0
    assert all(torch.equal(x, y) for x, y in zip(out_a, out_b))


def test_register_edits_sets_state_and_validates():
    pipe = _small_pipe()
    tfu.set_tokenflow(pipe.unet)
    tfu.register_edits(pipe, 3)
    blocks = [b for _, b in pipe.unet.transformer_blocks_in_order()]
    assert len(blocks) == 16 and all(b.n_edits == 3 and b.attn1.n_edits == 3 for b in blocks)
    assert pipe.unet.up_blocks[1].resnets[1].n_edits == 3
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            tfu.register_edits(pipe, bad)


def test_unsupported_combinations_raise(monkeypatch):
    monkeypatch.setattr(hooks, "ops", ef.EditFakeOps())
    pipe = _small_pipe()
    tfu.register_extended_attention_pnp(pipe, [])
    tfu.set_tokenflow(pipe.unet)
    tfu.register_time(pipe, 1)
    tfu.register_pivotal(pipe, True)
    tfu.register_edits(pipe, 2)
    blk = pipe.unet.down_blocks[0].attentions[0].transformer_blocks[0]
    D = gc.BLOCKS_CFG["dims"][0]
    x, enc = torch.randn(10, 16, D), torch.randn(10, 7, 32)
    with torch.no_grad():
        blk(x, encoder_hidden_states=enc)                    # the supported path runs
        with pytest.raises(ValueError, match="branches"):    # a batch that does not hold 1 + 2E branches
            blk(torch.randn(9, 16, D), encoder_hidden_states=torch.randn(9, 7, 32))

        class _Shard:                                        # a registered frame shard
            world, Kl, kf0 = 2, 2, 0
        tfu.register_frame_shard(pipe.unet, _Shard())
        with pytest.raises(ValueError, match="frame shard"):
            blk(x, encoder_hidden_states=enc)
        tfu.register_frame_shard(pipe.unet, None)
        blk(x, encoder_hidden_states=enc)

        ada = copy.copy(blk)                                 # the AdaLayerNormZero gated path
        ada.__dict__ = dict(blk.__dict__)
        ada.use_ada_layer_norm_zero = True
        with pytest.raises(ValueError, match="AdaLayerNormZero"):
            ada(x, encoder_hidden_states=enc)

        # replay through graphs.py: a capture in progress
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(ValueError, match="graphs.py"):
            blk(x, encoder_hidden_states=enc)
