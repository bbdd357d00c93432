"""Launch plans of the PARTS of a multi-edit attention call (tf_ext_attn_edits_part_plan; host only: the library records the
launches it would make).

The part call is the masked composition cut in two -- the bank branches of every edit behind the single V^T pre-pass, the
source branch -- for a frame-sharded rank, which computes the first on the buffer its exchange delivered and the second on
its own tensors.  Where every part takes the fused small-problem kernel they share ONE launch of up to 1 + E tensor sets."""
import ctypes
import re

import pytest

from tokenflow_amd import _lib, ops

SHAPES = [(4, 2, 1024, 1, 40), (8, 1, 4096, 1, 40), (4, 2, 192, 2, 80), (4, 2, 64, 2, 160)]   # K, Kq, S, H, Dh
CASES = [(E, m) for E in (2, 3) for m in range(1 << E)]


def _strip(plan):
    return [t for t in plan if t != "vt_pack"]


def _source_tokens(K, Kq, S, H, dh, E, mask, **kw):
    """Step 4 of the masked composition: the TF_ATTN_SOURCE_ONLY call, given TF_ATTN_INJECT iff every edit injects."""
    return _strip(ops.attn_plan(K, Kq, S, H, dh, mask == (1 << E) - 1, part="source", **kw))


@pytest.mark.parametrize("E,mask", CASES)
@pytest.mark.parametrize("K,Kq,S,H,dh", SHAPES)
@pytest.mark.parametrize("no_split", [False, True])
def test_streaming_parts_are_the_masked_plan_cut_in_two(K, Kq, S, H, dh, E, mask, no_split):
    kw = dict(fused=False, no_split=no_split)
    for multi_v in (False, True):
        masked = ops.attn_edits_plan(K, Kq, S, H, dh, False, E, inject_mask=mask, multi_v=multi_v, **kw)
        src = _source_tokens(K, Kq, S, H, dh, E, mask, **kw)
        assert masked[0] == "vt_pack" and masked.count("vt_pack") == 1 and masked[-len(src):] == src
        bank = ops.attn_edits_part_plan(K, Kq, S, H, dh, E, mask, part="bank", multi_v=multi_v, **kw)
        assert bank == masked[:-len(src)], (bank, masked)                  # the masked plan minus its source launches
        source = ops.attn_edits_part_plan(K, Kq, S, H, dh, E, mask, part="source", multi_v=multi_v, **kw)
        assert source == ["vt_pack"] + src                                  # the source launches alone, behind their pre-pass
        for compact in (False, True):
            assert ops.attn_edits_part_plan(K, Kq, S, H, dh, E, mask, part="all", qk_compact=compact, multi_v=multi_v,
                                            **kw) == masked


@pytest.mark.parametrize("E,mask", CASES)
@pytest.mark.parametrize("K,Kq,S,H,dh", SHAPES)
@pytest.mark.parametrize("no_split", [False, True])
def test_fused_parts_share_one_launch(K, Kq, S, H, dh, E, mask, no_split):
    """The decision is each part's own (the masked plan shows it): all fused -> ONE token with the set count; otherwise the
    composition of the masked call, cut as above."""
    masked = ops.attn_edits_plan(K, Kq, S, H, dh, False, E, inject_mask=mask, no_split=no_split, multi_v=False)
    src = _source_tokens(K, Kq, S, H, dh, E, mask, no_split=no_split)
    plans = {p: ops.attn_edits_part_plan(K, Kq, S, H, dh, E, mask, part=p, no_split=no_split, multi_v=False)
             for p in ("all", "bank", "source")}
    if all(t.startswith("fused[") for t in masked):
        assert len(masked) == E + 1
        geom = re.fullmatch(r"fused\[(qw=\d,kw=\d,qb=1,prec=\d)\]", masked[0]).group(1)
        if no_split:   # KW and PREC by shape alone: the joint launch has the parts' arithmetic
            assert "kw=4" in geom and all(re.search(r"kw=4,qb=1,prec=" + geom[-1], t) for t in masked)
        for part, n_sets in (("all", E + 1), ("bank", E)):
            plan = plans[part]
            assert len(plan) == 1 and plan[0].startswith("fused[qw="), (part, plan)
            if n_sets > 2:
                assert plan[0].endswith(f",sets={n_sets}]"), (part, plan)
            else:
                assert "sets=" not in plan[0] and re.fullmatch(r"fused\[qw=\d,kw=\d,qb=1,prec=\d\]", plan[0]), plan
            if no_split:
                assert re.search(r"kw=4,qb=1,prec=" + geom[-1], plan[0]), (plan, masked)
        assert plans["source"] == src and len(src) == 1 and "sets=" not in src[0]
    else:
        assert not any(t.startswith("fused") for t in masked)    # these shapes: all parts fused or none
        assert plans["all"] == masked
        assert plans["bank"] == masked[:-len(src)]
        assert _strip(plans["source"]) == src


def test_which_shapes_take_the_joint_launch():
    """(4, 2, 192, 2, 80) and (4, 2, 64, 2, 160) are small problems in both modes; a rank's 1024-token frames only in the
    default mode (small grid); 4096-token frames stream."""
    joint = lambda sh, ns: ops.attn_edits_part_plan(*sh, 3, 0b101, no_split=ns)
    for sh in SHAPES[2:]:
        for ns in (False, True):
            assert len(joint(sh, ns)) == 1 and joint(sh, ns)[0].endswith(",sets=4]")
    assert joint(SHAPES[0], False) == ["fused[qw=1,kw=4,qb=1,prec=0,sets=4]"]
    assert joint(SHAPES[0], True)[0] == "vt_pack" and joint(SHAPES[1], False)[0] == "vt_pack"
    # the existing entry points keep one launch per part
    assert ops.attn_edits_plan(4, 2, 192, 2, 80, False, 3, inject_mask=0b101) == ["fused[qw=1,kw=4,qb=1,prec=1]"] * 4
    # nine sets: the largest batch
    assert ops.attn_edits_part_plan(4, 2, 64, 2, 160, 8, 0b10110101) == ["fused[qw=1,kw=4,qb=1,prec=1,sets=9]"]


def test_one_edit_is_the_single_edit_part():
    for K, Kq, S, H, dh in SHAPES:
        for inj in (0, 1):
            for part in ("all", "bank", "source"):
                assert ops.attn_edits_part_plan(K, Kq, S, H, dh, 1, inj, part=part, qk_compact=True) == \
                    ops.attn_plan(K, Kq, S, H, dh, bool(inj), part=part)


def test_argument_errors():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1024)
    BANK, SRC = _lib.TF_ATTN_BANK_ONLY, _lib.TF_ATTN_SOURCE_ONLY
    plan = lambda E=2, mask=0, compact=0, flags=0: lib.tf_ext_attn_edits_part_plan(4, 2, 192, 2, 80, E, mask, compact, flags,
                                                                                  _lib.TF_BF16, buf, len(buf))
    assert plan() == 1 and plan(flags=BANK) == 1 and plan(flags=SRC) == 1
    assert plan(flags=BANK | SRC) == -3                                    # TF_ERR_SHAPE: both part bits
    assert plan(flags=_lib.TF_ATTN_INJECT) == -3                           # the mask is the injection state
    assert plan(mask=0b100) == -3 and plan(E=3, mask=0b100) == 1           # mask bits at or above E
    assert plan(compact=2) == -3 and plan(compact=-1) == -3 and plan(compact=1) == 1
    assert plan(E=0) == -3 and plan(E=_lib.TF_MAX_EDITS + 1) == -3
    assert plan(flags=_lib.TF_ATTN_MULTI_V | _lib.TF_ATTN_NO_MULTI_V) == -3
    # the existing entry points keep refusing the part bits
    assert lib.tf_ext_attn_edits_masked_plan(4, 2, 192, 2, 80, 2, 0, BANK, _lib.TF_BF16, buf, len(buf)) == -3
    with pytest.raises(ValueError):
        ops.attn_edits_part_plan(4, 2, 192, 2, 80, 2, 0b100)
