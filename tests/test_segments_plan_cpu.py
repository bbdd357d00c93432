"""Launch plans of the keyframe-segment entry points (tf_ext_attn_fwd_segments, tf_nn_gather_blend_chunks_segments) on the
host: the plan functions run the real dispatch under the plan recorder and touch no device."""
import ctypes
import re

import pytest

from tokenflow_amd import _lib, ops

NEW_SYMBOLS = ("tf_ext_attn_segments_workspace_bytes", "tf_ext_attn_fwd_segments", "tf_ext_attn_segments_plan",
               "tf_nn_gather_blend_chunks_segments", "tf_nn_gather_blend_chunks_norm_segments",
               "tf_nn_gather_blend_segments_plan")


def test_abi_and_exports():
    lib = _lib.load()
    assert lib.tf_abi_version() == 11 and _lib.ABI_VERSION == 11
    assert _lib.TF_MAX_SEGMENTS == 8
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name


@pytest.mark.parametrize("K,S,H,Dh,inject,kw", [
    (5, 48, 2, 40, True, {}),
    (5, 320, 2, 80, False, {"no_split": True}),
    (8, 1024, 8, 40, True, {}),
    (4, 4096, 8, 40, True, {}),
    (5, 512, 2, 40, False, {"fused": False}),
])
def test_one_segment_is_the_single_call(K, S, H, Dh, inject, kw):
    assert ops.attn_segments_plan(K, [K], S, H, Dh, inject, **kw) == ops.attn_plan(K, K, S, H, Dh, inject, **kw)


@pytest.mark.parametrize("segs", [[2, 3], [1, 1, 3], [1] * 8])
@pytest.mark.parametrize("S,H,Dh", [(48, 2, 40), (192, 2, 160)])
@pytest.mark.parametrize("no_split", [False, True])
def test_fused_size_is_one_multi_set_launch(segs, S, H, Dh, no_split):
    K = sum(segs)
    for inject in (False, True):
        own = [ops.attn_plan(k, k, S, H, Dh, inject, no_split=no_split) for k in segs]
        assert all(len(p) == 1 and p[0].startswith("fused[") for p in own)
        plan = ops.attn_segments_plan(K, segs, S, H, Dh, inject, no_split=no_split)
        assert len(plan) == 1 and re.fullmatch(r"fused\[qw=\d,kw=\d,qb=\d,prec=\d,sets=%d\]" % len(segs), plan[0]), plan
        if no_split:    # the fused plan is a function of the shape alone: the geometry of every segment's own launch
            assert {p[0][:-1] for p in own} == {plan[0].split(",sets=")[0]}


@pytest.mark.parametrize("segs", [[2, 3], [1, 1, 3]])
@pytest.mark.parametrize("S,H,Dh,kw", [
    (320, 2, 64, {"fused": False}),
    (512, 2, 40, {"fused": False}),
    (512, 2, 40, {"fused": False, "hints": _lib.TF_ATTN_HINT_MIX}),
    (320, 2, 80, {"no_split": True}),
    (4096, 8, 40, {}),
    (2048, 10, 64, {}),
])
def test_streaming_is_one_pre_pass_and_every_segments_own_launches(segs, S, H, Dh, kw):
    K = sum(segs)
    for inject in (False, True):
        want = ["vt_pack"]
        for k in segs:
            own = ops.attn_plan(k, k, S, H, Dh, inject, **kw)
            assert own[0] == "vt_pack" and "vt_pack" not in own[1:] and not any(t.startswith("fused") for t in own)
            want += own[1:]
        assert ops.attn_segments_plan(K, segs, S, H, Dh, inject, **kw) == want


@pytest.mark.parametrize("segs,S,H,Dh", [([2, 3], 512, 8, 40), ([1, 17], 256, 8, 40), ([3, 2, 4], 512, 8, 40)])
def test_mixed_fused_and_streaming_segments(segs, S, H, Dh):
    """Default mode: a segment's own decision depends on its grid.  The fused ones share one launch behind the streaming ones."""
    K = sum(segs)
    own = [ops.attn_plan(k, k, S, H, Dh, True) for k in segs]
    fused = [p for p in own if p[0].startswith("fused")]
    assert 0 < len(fused) < len(segs)
    want = ["vt_pack"] + [t for p in own if p not in fused for t in p[1:]]
    plan = ops.attn_segments_plan(K, segs, S, H, Dh, True)
    assert plan[:-1] == want
    assert plan[-1] == fused[0][0][:-1] + ",sets=%d]" % len(fused)


def test_joint_grid_may_leave_the_fused_range():
    """Default mode, S in (256, 1024]: fused on small grids only.  Eight small segments make a large joint grid: they stream."""
    segs, S, H, Dh = [2] * 8, 512, 8, 40
    assert all(ops.attn_plan(k, k, S, H, Dh, True)[0].startswith("fused") for k in segs)
    plan = ops.attn_segments_plan(sum(segs), segs, S, H, Dh, True)
    own = ops.attn_plan(2, 2, S, H, Dh, True, fused=False)
    assert plan == ["vt_pack"] + own[1:] * 8


def _attn_plan_rc(K, segs, S=64, H=2, Dh=40, flags=0, dtype=_lib.TF_BF16):
    buf = ctypes.create_string_buffer(4096)
    arr = (ctypes.c_int * max(len(segs), 1))(*segs) if segs is not None else None
    return _lib.load().tf_ext_attn_segments_plan(K, len(segs) if segs is not None else 1, arr, S, H, Dh, flags, dtype, buf,
                                                 len(buf))


@pytest.mark.parametrize("flag", [_lib.TF_ATTN_BANK_ONLY, _lib.TF_ATTN_SOURCE_ONLY, _lib.TF_ATTN_MULTI_V,
                                  _lib.TF_ATTN_NO_MULTI_V, _lib.TF_ATTN_MULTI_V64, _lib.TF_ATTN_RUN_MULTI_V])
def test_attention_flag_refusals(flag):
    assert _attn_plan_rc(5, [2, 3], flags=flag) == -3
    assert _attn_plan_rc(5, [5], flags=flag) == -3


def test_attention_shape_refusals():
    assert _attn_plan_rc(5, [2, 3]) == 1
    assert _attn_plan_rc(5, [2, 2]) == -3            # the segments do not hold the pass's keyframes
    assert _attn_plan_rc(5, [2, 4]) == -3
    assert _attn_plan_rc(5, [5, 0]) == -3            # a segment without keyframes
    assert _attn_plan_rc(9, [1] * 9) == -3           # more than TF_MAX_SEGMENTS
    assert _attn_plan_rc(5, []) == -3
    assert _attn_plan_rc(5, None) == -1              # null seg_K
    assert _attn_plan_rc(5, [2, 3], Dh=48) == -3
    assert _attn_plan_rc(5, [2, 3], dtype=_lib.TF_F32) == -2
    with pytest.raises(ValueError):
        ops.attn_segments_plan(5, [2, 2], 64, 2, 40, True)


def test_attention_call_refuses_before_the_device():
    """The entry point itself with placeholder pointers: every refusal returns before a launch (no GPU here)."""
    lib = _lib.load()
    ph = 1 << 12
    seg = (ctypes.c_int * 2)(2, 3)

    def rc(K=5, n_seg=2, seg_K=seg, flags=0, ws_bytes=1 << 40, q=ph, ws=ph):
        return lib.tf_ext_attn_fwd_segments(q, ph, ph, ph, K, n_seg, seg_K, 64, 2, 40, 80, 0.158, flags, _lib.TF_BF16, ws,
                                            ws_bytes, None)
    assert rc(flags=_lib.TF_ATTN_BANK_ONLY) == -3
    assert rc(K=6) == -3
    assert rc(n_seg=9) == -3
    assert rc(seg_K=None) == -1
    assert rc(q=None) == -1
    assert rc(ws_bytes=16) == -5
    assert rc(q=ph + 2) == -4
    need = lib.tf_ext_attn_segments_workspace_bytes(5, 64, 2, 40, _lib.TF_BF16)
    assert need >= lib.tf_ext_attn_workspace_bytes(5, 64, 2, 40, _lib.TF_BF16) > 0


# ---------------------------------------------------------------------------------------------- propagation
@pytest.mark.parametrize("n,C,S,D", [(2, 5, 64, 320), (2, 5, 256, 640), (2, 5, 64, 1280), (4, 8, 1024, 320), (1, 1, 64, 320)])
def test_propagation_plan_is_the_chunk_search_and_one_gather(n, C, S, D):
    for mask in (0, 1, 0b101 & ((1 << C) - 1), (1 << C) - 1):
        # (C = 1: tf_nn_search_plan is the plan of tf_nn_search and ends with its finalize; the gather merges the splits itself)
        want = [t for t in ops.nn_plan(n * S, S, D, 2, C) if t != "finalize"] + ["gather[branches=3]"]
        assert ops.propagate_segments_plan(n, C, S, D, mask) == want


def test_one_segment_propagation_is_the_search_plan():
    """[K]: mask 1 (a run from chunk 0) and mask 0 (a run from a later chunk) record tf_nn_search_plan's tokens exactly."""
    for mask in (0, 1):
        assert ops.propagate_segments_plan(2, 5, 64, 320, mask)[:-1] == ops.nn_plan(128, 64, 320, 2, 5)


def test_propagation_refusals():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    assert lib.tf_nn_gather_blend_segments_plan(2, 5, 64, 320, 1 << 5, buf, len(buf)) == -3      # a bit at C
    assert lib.tf_nn_gather_blend_segments_plan(2, 65, 64, 320, 0, buf, len(buf)) == -3          # C > 64
    assert lib.tf_nn_gather_blend_segments_plan(2, 64, 64, 320, 1 << 63, buf, len(buf)) == 2     # C = 64: every bit is a chunk
    assert lib.tf_nn_gather_blend_segments_plan(2, 5, 64, 324, 0, buf, len(buf)) == -3
    ph = 1 << 12

    def rc(C=5, K=6, slot0=1, mask=0b100, ws_bytes=1 << 40, tgt=ph):
        return lib.tf_nn_gather_blend_chunks_segments(tgt, ph, ph, ph, ph, ph, ph, K, 2, C, 64, 320, slot0, mask, _lib.TF_BF16,
                                                      _lib.TF_BF16, _lib.TF_BF16, _lib.TF_F32, _lib.TF_BF16, ph, ws_bytes, None)
    assert rc(slot0=0) == -3               # chunk 0 blends slot0 - 1 unless bit 0 is set
    assert rc(mask=1 << 5) == -3
    assert rc(K=5) == -3                   # slot0 + C > K
    assert rc(C=65, K=70) == -3
    assert rc(tgt=None) == -1
    assert rc(tgt=ph + 2) == -4
    assert rc(ws_bytes=0) == -5
    with pytest.raises(ValueError):
        ops.propagate_segments_plan(2, 5, 64, 320, 1 << 5)
