"""Per-edit injection schedules of a multi-edit pass on the host: the launch plans of the masked attention entry point
(the library records the launches it would make; no GPU) and the hook logic of `register_edit_schedules` over
oracle-backed ops (tests/edit_schedule_forms.py)."""
import pytest
import torch

import tokenflow_utils as tfu
from oracle import golden_cases as gc
from tests import edit_forms as ef
from tests import edit_schedule_forms as esf
from tests import fake_diffusers as fd
from tests.fake_ops import FakeOps
from tokenflow_amd import _lib, hooks, ops

MV4 = "one<40,1,4,MV4,2,fq0>"
PLAN_SHAPES = [(8, 4096, 8, 40), (4, 1024, 8, 40), (4, 1024, 8, 64)]     # (K, S, H, Dh)
MULTI_V = [None, False, True]
TF_ERR_SHAPE = -3     # include/tokenflow_hip.h


def test_abi_11():
    assert _lib.ABI_VERSION == 11 and _lib.load().tf_abi_version() == 11
    for name in ("tf_ext_attn_fwd_edits_masked", "tf_ext_attn_edits_masked_plan", "tf_inject_copy_edits_masked"):
        assert hasattr(_lib.load(), name)


# --------------------------------------------------------------------------------------------------------------- plans
@pytest.mark.parametrize("K,S,H,dh", PLAN_SHAPES)
@pytest.mark.parametrize("E", [3, 4])
@pytest.mark.parametrize("multi_v", MULTI_V)
def test_uniform_masks_are_the_unmasked_plans(K, S, H, dh, E, multi_v):
    for dtype in (torch.bfloat16, torch.float16):
        kw = dict(dtype=dtype, multi_v=multi_v)
        assert ops.attn_edits_plan(K, K, S, H, dh, False, E, inject_mask=0, **kw) == \
            ops.attn_edits_plan(K, K, S, H, dh, False, E, **kw)
        assert ops.attn_edits_plan(K, K, S, H, dh, False, E, inject_mask=(1 << E) - 1, **kw) == \
            ops.attn_edits_plan(K, K, S, H, dh, True, E, **kw)


def _without_pack(plan):
    return [t for t in plan if t != "vt_pack"]


@pytest.mark.parametrize("K,S,H", [s[:3] for s in PLAN_SHAPES[:2]])
@pytest.mark.parametrize("E", [3, 4])
def test_mixed_masks_with_the_four_bank_form(K, S, H, E):
    """Dh = 40, multi_v=True: one pre-pass; the injecting edits in pairs (MV4), an odd one in the DUAL launch where a pair
    exists (its own bank-only launches where it is alone); then every non-injecting edit's own bank-only launches; the source
    launches last."""
    dh = 40
    bank_non = _without_pack(ops.attn_plan(K, K, S, H, dh, False, part="bank"))
    bank_inj = _without_pack(ops.attn_plan(K, K, S, H, dh, True, part="bank"))
    src = _without_pack(ops.attn_plan(K, K, S, H, dh, False, part="source"))
    for mask in range(1, (1 << E) - 1):
        n_inj, n_non = esf.popcount(mask), E - esf.popcount(mask)
        plan = ops.attn_edits_plan(K, K, S, H, dh, False, E, multi_v=True, inject_mask=mask)
        assert plan.count("vt_pack") == 1 and plan[0] == "vt_pack", (mask, plan)
        body = plan[1:]
        assert body.count(MV4) == n_inj // 2 and body[:n_inj // 2] == [MV4] * (n_inj // 2), (mask, plan)
        rest = body[n_inj // 2:]
        if n_inj >= 2:
            odd = rest[:n_inj % 2]
            assert all(",DUAL," in t for t in odd) and sum(1 for t in body if ",DUAL," in t) == n_inj % 2, (mask, plan)
        else:       # one injecting edit alone: the launches of its own TF_ATTN_BANK_ONLY | TF_ATTN_INJECT call
            odd = rest[:len(bank_inj)]
            assert odd == bank_inj, (mask, plan)
        rest = rest[len(odd):]
        assert rest == bank_non * n_non + src, (mask, plan)


@pytest.mark.parametrize("E", [3, 4])
def test_mixed_masks_composition(E):
    """Without the four-bank form (multi_v=False at Dh = 40; any hint at Dh = 64): injecting edits' bank-only launches
    ascending, then the others', then the source; no MV4 token for any mask at Dh = 64."""
    for (K, S, H, dh), multi_v in [(PLAN_SHAPES[0], False), (PLAN_SHAPES[1], False)] + [(PLAN_SHAPES[2], m) for m in MULTI_V]:
        bank_non = _without_pack(ops.attn_plan(K, K, S, H, dh, False, part="bank"))
        bank_inj = _without_pack(ops.attn_plan(K, K, S, H, dh, True, part="bank"))
        src = _without_pack(ops.attn_plan(K, K, S, H, dh, False, part="source"))
        for mask in range(1 << E):
            plan = ops.attn_edits_plan(K, K, S, H, dh, False, E, multi_v=multi_v, inject_mask=mask)
            assert MV4 not in plan and plan.count("vt_pack") <= 1
            if 0 < mask < (1 << E) - 1:
                n_inj = esf.popcount(mask)
                assert _without_pack(plan) == bank_inj * n_inj + bank_non * (E - n_inj) + src, (dh, mask, plan)


def test_default_rule_counts_the_injecting_edits():
    """cfg1 level 0 is a measured-default class: without a hint mask 0b101 plans one MV4 launch, mask 0b001 none."""
    assert ops.attn_edits_plan(4, 4, 1024, 8, 40, False, 3, inject_mask=0b101).count(MV4) == 1
    assert ops.attn_edits_plan(4, 4, 1024, 8, 40, False, 3, inject_mask=0b001).count(MV4) == 0
    assert ops.attn_edits_plan(4, 4, 1024, 8, 40, False, 3, multi_v=True, inject_mask=0b010).count(MV4) == 0
    assert ops.attn_edits_plan(2, 2, 320, 2, 40, False, 3, inject_mask=0b101).count(MV4) == 0      # not a measured class


def test_plan_errors():
    with pytest.raises(ValueError):
        ops.attn_edits_plan(4, 4, 1024, 8, 40, True, 3, inject_mask=0b101)       # inject=True beside a mask
    with pytest.raises(ValueError):
        ops.attn_edits_plan(4, 4, 1024, 8, 40, False, 3, inject_mask=0b1000)     # a bit at or above E
    for E in (0, 9):
        with pytest.raises(ValueError):
            ops.attn_edits_plan(4, 4, 1024, 8, 40, False, E, inject_mask=0)
    # the C entry points say the same
    import ctypes
    lib, buf = _lib.load(), ctypes.create_string_buffer(1024)
    assert lib.tf_ext_attn_edits_masked_plan(4, 4, 1024, 8, 40, 3, 0b101, _lib.TF_ATTN_INJECT, _lib.TF_BF16, buf, 1024) == TF_ERR_SHAPE
    assert lib.tf_ext_attn_edits_masked_plan(4, 4, 1024, 8, 40, 3, 0b1000, 0, _lib.TF_BF16, buf, 1024) == TF_ERR_SHAPE
    assert lib.tf_ext_attn_edits_masked_plan(4, 4, 1024, 8, 40, 9, 0, 0, _lib.TF_BF16, buf, 1024) == TF_ERR_SHAPE
    assert lib.tf_ext_attn_edits_masked_plan(4, 4, 1024, 8, 40, 3, 0b101, 0, _lib.TF_BF16, buf, 1024) > 0


# --------------------------------------------------------------------------------------------------------------- hooks
def _exact_attn(out3, q3, k3, v3, heads, scale, inject, what):
    from oracle import tokenflow_oracle as orc
    ref = orc.ext_attn_core(q3, k3, v3, heads, scale, inject)
    assert torch.equal(out3.float(), ref.to(out3.dtype).float()), what
    return 0.0


def _fake_indices(tgt, piv, inv, ids):
    return FakeOps().nn_search(tgt, piv, inv, ids)


def test_edit_schedules_cfg1_dry_run(monkeypatch):
    """Steps 0 / 6 / 12 / 17: q/k masks 0b101 (a pair that is not adjacent), 0b001, 0, 0; feature masks all, all, 0b101, 0.
    Call counts are the single-edit harness's, uniform masks arrive as today's positional calls and mixed ones as
    keywords on the 8 injected blocks only, and every edit equals the single-edit pipeline installed with ITS schedules."""
    esf.run_edit_schedules_cfg1(esf.ScheduleEditFakeOps, torch.device("cpu"), monkeypatch, _exact_attn, _fake_indices)


def _small_pipe():
    cfg = gc.BLOCKS_CFG
    torch.manual_seed(cfg["seed"])
    pipe = fd.FakePipeline(dims=cfg["dims"], heads=cfg["heads"], cross_dim=cfg["cross_dim"]).eval()
    tfu.register_extended_attention_pnp(pipe, [5, 3])
    tfu.register_conv_injection(pipe, [5])
    tfu.set_tokenflow(pipe.unet)
    return pipe


def _injected_attns(pipe):
    return [pipe.unet.up_blocks[r].attentions[b].transformer_blocks[0].attn1 for r, bs in hooks._INJECTED_UP.items() for b in bs]


def test_register_edit_schedules_validates_and_clears():
    pipe = _small_pipe()
    tfu.register_edits(pipe, 3)
    conv = pipe.unet.up_blocks[1].resnets[1]
    for bad in ([[5], [3]], [[5]] * 4):
        with pytest.raises(ValueError):
            tfu.register_edit_schedules(pipe, qk_schedules=bad)
        with pytest.raises(ValueError):
            tfu.register_edit_schedules(pipe, conv_schedules=bad)
        with pytest.raises(ValueError):       # nothing is set when one of the two is wrong
            tfu.register_edit_schedules(pipe, qk_schedules=[[5], [], [3]], conv_schedules=bad)
        assert "_tf_edit_schedule_sets" not in conv.__dict__
        assert not any("_tf_edit_schedule_sets" in m.__dict__ for m in _injected_attns(pipe))
    tfu.register_edit_schedules(pipe, qk_schedules=[torch.tensor([5, 3]), None, [3]], conv_schedules=[[5], [], [5, 3]])
    attns = _injected_attns(pipe)
    assert len(attns) == 8
    others = [b.attn1 for _, b in pipe.unet.transformer_blocks_in_order() if b.attn1 not in attns]
    assert len(others) == 8 and not any("_tf_edit_schedule_sets" in m.__dict__ for m in others)
    tfu.register_time(pipe, 5)
    assert [hooks._inject_mask(m, 3) for m in attns] == [0b001] * 8 and hooks._inject_mask(conv, 3) == 0b101
    assert all(hooks._inject_mask(m, 3) == 0 for m in others)
    tfu.register_time(pipe, torch.tensor(3))
    assert [hooks._inject_mask(m, 3) for m in attns] == [0b101] * 8 and hooks._inject_mask(conv, 3) == 0b100
    tfu.register_time(pipe, 1000)             # the reference's `or t == 1000`, for the edits that have a schedule
    assert hooks._inject_mask(attns[0], 3) == 0b101 and hooks._inject_mask(conv, 3) == 0b101
    tfu.register_time(pipe, 7)
    assert hooks._inject_mask(attns[0], 3) == 0 and hooks._inject_mask(conv, 3) == 0
    # None removes one kind and keeps the other; the shared schedule holds again
    tfu.register_time(pipe, 3)
    tfu.register_edit_schedules(pipe, qk_schedules=None, conv_schedules=[[5], [], [5, 3]])
    assert hooks._inject_mask(attns[0], 3) == 0b111 and hooks._inject_mask(conv, 3) == 0b100
    tfu.register_edit_schedules(pipe, qk_schedules=[[3], [], []])
    assert hooks._inject_mask(attns[0], 3) == 0b001 and hooks._inject_mask(conv, 3) == 0        # shared conv schedule: [5]
    # re-running an installer removes them on the modules it touches
    tfu.register_edit_schedules(pipe, qk_schedules=[[3], [], []], conv_schedules=[[3], [], []])
    tfu.register_conv_injection(pipe, [3])
    assert hooks._inject_mask(conv, 3) == 0b111 and hooks._inject_mask(attns[0], 3) == 0b001
    tfu.register_extended_attention_pnp(pipe, [5])
    assert hooks._inject_mask(attns[0], 3) == 0
    # a module whose number of edits changed underneath the schedules
    tfu.register_edit_schedules(pipe, qk_schedules=[[3], [], []])
    tfu.register_edits(pipe, 2)
    with pytest.raises(ValueError):
        hooks._inject_mask(attns[0], 2)


def test_clearing_restores_the_shared_calls_and_sdedit_ignores_schedules(monkeypatch):
    """After `register_edit_schedules(model, None, None)` the pass issues the calls of a pipeline that never had per-edit
    schedules; the SDEdit installer never injects whatever schedules are registered."""
    D = gc.BLOCKS_CFG["dims"][0]
    x, enc = torch.randn(7 * 2, 16, D), torch.randn(7 * 2, 7, gc.BLOCKS_CFG["cross_dim"])

    def trace(pipe, t):
        fake = esf.ScheduleEditFakeOps()
        monkeypatch.setattr(hooks, "ops", fake)
        tfu.register_time(pipe, t)
        tfu.register_pivotal(pipe, True)
        blk = pipe.unet.up_blocks[3].attentions[0].transformer_blocks[0]
        with torch.no_grad():
            out = blk(x, encoder_hidden_states=enc)
        return fake.calls, out

    plain, sched = _small_pipe(), _small_pipe()
    for pipe in (plain, sched):
        tfu.register_edits(pipe, 3)
    tfu.register_edit_schedules(sched, qk_schedules=[[5], [], [5]], conv_schedules=[[5], [], []])
    calls, _ = trace(sched, 5)
    assert [c for c in calls if c[0] == "ext_attn_edits"] == [("ext_attn_edits", (14, 16, D), False, 3, 0b101)]
    tfu.register_edit_schedules(sched, None, None)
    for t in (5, 3, 7):
        (ca, oa), (cb, ob) = trace(plain, t), trace(sched, t)
        assert ca == cb and torch.equal(oa, ob) and not any(len(c) == 5 for c in ca if c[0] == "ext_attn_edits")
    tfu.register_edit_schedules(sched, qk_schedules=[[5], [], [5]])
    tfu.register_extended_attention(sched)
    calls, _ = trace(sched, 5)
    assert [c for c in calls if c[0] == "ext_attn_edits"] == [("ext_attn_edits", (14, 16, D), False, 3)]
