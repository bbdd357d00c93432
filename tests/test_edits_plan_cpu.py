"""Launch plans of the multi-edit entry points (host only: the library records the launches it would make).

A multi-edit batch is a composition: ONE V^T pre-pass, the source branch once, every edit's bank branches through the
launches of a bank-only call -- or, under q/k injection at head dim 40 with the four-bank form on, one MV4 launch per
PAIR of edits and the DUAL launch for an odd last one.  One NN search whatever the number of edits."""
import ctypes

import pytest
import torch

from tokenflow_amd import _lib, ops

MV4 = "one<40,1,4,MV4,2,fq0>"
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(dh, S) for dh in (40, 64, 80, 160) for S in (45, 64, 256, 1024, 4096)]
H, K = 8, 8


def _is_bank_group_end(tok):
    return tok.startswith("merge") or tok.startswith("fused")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh,S", SHAPES)
def test_without_injection_one_source_launch_and_e_bank_groups(dh, S, dtype):
    bank = ops.attn_plan(K, K, S, H, dh, False, dtype=dtype, part="bank")
    src = ops.attn_plan(K, K, S, H, dh, False, dtype=dtype, part="source")
    packs = [t for t in bank + src if t == "vt_pack"]
    bank_l, src_l = [t for t in bank if t != "vt_pack"], [t for t in src if t != "vt_pack"]
    assert len(src_l) == 1
    for E in (2, 3, 4):
        plan = ops.attn_edits_plan(K, K, S, H, dh, False, E, dtype=dtype)
        assert plan == (["vt_pack"] if packs else []) + bank_l * E + src_l, (E, plan)
        assert plan.count("vt_pack") <= 1 and MV4 not in plan


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh,S", SHAPES)
@pytest.mark.parametrize("multi_v", [None, False, True])
def test_with_injection(dh, S, dtype, multi_v):
    """Composition (TF_ATTN_NO_MULTI_V, and the default below S = 1024): E bank groups of the bank-only call.  Four-bank
    form on (TF_ATTN_MULTI_V at every S; the default in the measured classes: 1024 <= S <= 4096, 8 heads, 4 to 8
    keyframes, every keyframe's queries), head dim 40:
    floor(E/2) MV4 launches + (E mod 2) DUAL launches, all one-pass."""
    bank = [t for t in ops.attn_plan(K, K, S, H, dh, True, dtype=dtype, part="bank") if t != "vt_pack"]
    src = [t for t in ops.attn_plan(K, K, S, H, dh, True, dtype=dtype, part="source") if t != "vt_pack"]
    for E in (2, 3, 4):
        plan = ops.attn_edits_plan(K, K, S, H, dh, True, E, dtype=dtype, multi_v=multi_v)
        assert plan.count("vt_pack") <= 1
        if dh == 40 and (multi_v or (multi_v is None and 1024 <= S <= 4096)):   # the measured default (K = H = 8 here)
            body = [t for t in plan if t != "vt_pack"]
            assert plan[0] == "vt_pack" and plan.count("vt_pack") == 1
            assert body[:E // 2] == [MV4] * (E // 2), plan
            odd = body[E // 2:len(body) - len(src)]
            assert len(odd) == E % 2 and all(",DUAL," in t for t in odd), plan
            assert body[len(body) - len(src):] == src
            assert not any(t.startswith("merge") for t in plan)          # one-pass launches
        else:
            assert [t for t in plan if t != "vt_pack"] == bank * E + src, (E, plan)
            assert MV4 not in plan


def test_small_grid_regimes_compose_the_part_calls():
    """cfg1-like grids: the split form (DUAL + merge per edit) and the fused small-problem kernel per part."""
    for K_, S, inject in [(4, 1024, True), (4, 1024, False), (4, 256, True), (4, 256, False), (2, 64, True)]:
        bank = ops.attn_plan(K_, K_, S, H, 40, inject, part="bank")
        src = ops.attn_plan(K_, K_, S, H, 40, inject, part="source")
        plan = ops.attn_edits_plan(K_, K_, S, H, 40, inject, 3, multi_v=False)
        strip = lambda p: [t for t in p if t != "vt_pack"]
        assert strip(plan) == strip(bank) * 3 + strip(src), (K_, S, inject, plan)
        assert plan.count("vt_pack") == (1 if "vt_pack" in bank + src else 0)
    assert any(t.startswith("merge") for t in ops.attn_edits_plan(4, 4, 1024, H, 40, True, 2, multi_v=False))
    assert all(t.startswith("fused") for t in ops.attn_edits_plan(4, 4, 256, H, 40, False, 2))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("dh,S", SHAPES)
def test_one_edit_is_the_single_edit_plan(dh, S, inject, dtype):
    for multi_v in (None, True, False):
        assert ops.attn_edits_plan(K, K, S, H, dh, inject, 1, dtype=dtype, multi_v=multi_v) == \
            ops.attn_plan(K, K, S, H, dh, inject, dtype=dtype)


def test_existing_plans_are_untouched():
    assert ops.attn_plan(8, 8, 4096, 8, 40, True) == ["vt_pack", "il<40,8,DUAL,4,2>", "il<40,8,SOURCE,4,3>"]
    assert ops.attn_plan(8, 8, 4096, 8, 40, False) == ["vt_pack", "il<40,8,ALL,4,3>"]


def test_argument_errors():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1024)
    plan = lambda E, dt=_lib.TF_BF16, flags=1: lib.tf_ext_attn_edits_plan(8, 8, 256, 8, 40, E, flags, dt, buf, len(buf))
    assert plan(0) == -3 and plan(_lib.TF_MAX_EDITS + 1) == -3            # TF_ERR_SHAPE
    assert plan(2, _lib.TF_F32) == -2                                      # TF_ERR_DTYPE
    assert plan(2, flags=1 | _lib.TF_ATTN_BANK_ONLY) == -3
    assert plan(2, flags=1 | _lib.TF_ATTN_MULTI_V | _lib.TF_ATTN_NO_MULTI_V) == -3
    assert plan(_lib.TF_MAX_EDITS) > 0
    assert lib.tf_ext_attn_edits_plan(8, 8, 4096, 8, 40, 4, 1, _lib.TF_BF16, buf, 8) == -5    # TF_ERR_WORKSPACE: buffer
    assert lib.tf_ext_attn_edits_workspace_bytes(8, 256, 8, 40, 0, _lib.TF_BF16) == 0
    assert lib.tf_ext_attn_edits_workspace_bytes(8, 256, 8, 40, 1, _lib.TF_BF16) == \
        lib.tf_ext_attn_workspace_bytes(8, 256, 8, 40, _lib.TF_BF16)
    assert lib.tf_ext_attn_edits_workspace_bytes(8, 256, 8, 40, 3, _lib.TF_BF16) > \
        lib.tf_ext_attn_workspace_bytes(8, 256, 8, 40, _lib.TF_BF16)
    gplan = lambda E: lib.tf_nn_gather_blend_edits_plan(5, 8, 4096, 320, 1, E, buf, len(buf))
    assert gplan(0) == -3 and gplan(_lib.TF_MAX_EDITS + 1) == -3 and gplan(2) == 2
    assert lib.tf_inject_copy_edits(None, 64, 5, 2, None) == -1             # TF_ERR_NULL
    with pytest.raises(_lib.TokenflowHipError):       # no CPU fallback for the new ops either
        ops.ext_attn_edits(torch.zeros(5, 8, 320), torch.zeros(5, 8, 320), torch.zeros(5, 8, 320), 8, 1.0, True, 2)
    with pytest.raises(_lib.TokenflowHipError):
        ops.inject_copy_edits_(torch.zeros(5, 8), 2)


@pytest.mark.parametrize("n,C,S,D", [(5, 8, 4096, 320), (2, 4, 1024, 320), (5, 8, 256, 1280), (2, 3, 45, 1280), (2, 1, 1024, 320)])
@pytest.mark.parametrize("first", [False, True])
def test_propagation_searches_once(n, C, S, D, first):
    """The search launches are those of the single-edit call (tf_nn_search_plan; the gather merges the splits itself, so
    no finalize) -- once, whatever E -- followed by ONE gather over all 1 + 2E branches."""
    single = C == 1 and first
    search = [t for t in ops.nn_plan(n * S, S, D, 1 if single else 2, C) if t != "finalize"]
    for E in (1, 2, 3, 8):
        assert ops.propagate_edits_plan(n, C, S, D, first, E) == search + [f"gather[branches={1 + 2 * E}]"]


def test_default_covers_only_the_measured_shape_classes():
    """Without a hint the four-bank form is taken where it was measured against the composition (every keyframe's queries,
    8 heads, 4 to 8 keyframes, 1024 <= S <= 4096) and nowhere else; the hint still reaches the other grids."""
    for K_, Kq, S, H_, on in [(8, 8, 4096, 8, True), (4, 4, 1024, 8, True), (8, 8, 2304, 8, True), (8, 4, 4096, 8, False),
                              (8, 8, 4096, 2, False), (16, 16, 1024, 8, False), (2, 2, 4096, 8, False), (8, 8, 9216, 8, False),
                              (8, 8, 256, 8, False)]:
        assert (MV4 in ops.attn_edits_plan(K_, Kq, S, H_, 40, True, 2)) == on, (K_, Kq, S, H_)
        assert MV4 in ops.attn_edits_plan(K_, Kq, S, H_, 40, True, 2, multi_v=True)
