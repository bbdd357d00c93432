"""Launch plans and refusals of the ragged chunk runs (tf_nn_gather_blend_chunks_ragged) on the host: the plan function runs the
real entry point under the plan recorder and touches no device."""
import ctypes
import os
import re

import pytest

from tests import ragged_forms as rf
from tokenflow_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tf_nn_gather_blend_ragged_workspace_bytes", "tf_nn_gather_blend_chunks_ragged",
               "tf_nn_gather_blend_chunks_norm_ragged", "tf_nn_gather_blend_ragged_plan")


def test_header_declarations_and_exports():
    lib = _lib.load()
    assert lib.tf_abi_version() == 11 and _lib.ABI_VERSION == 11          # additive: the ABI number stays
    header = open(os.path.join(ROOT, "include", "tokenflow_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert re.search(r"TF_API (int|size_t) %s\(" % name, header), name
    assert hasattr(ops, "propagate_chunks_ragged") and hasattr(ops, "propagate_ragged_plan")


@pytest.mark.parametrize("n,C,S,D", [(2, 5, 64, 320), (2, 5, 256, 640), (3, 4, 45, 1280), (4, 8, 1024, 320), (2, 3, 4040, 72)])
def test_uniform_frames_are_todays_plans(n, C, S, D):
    for mask in (0, 1, 0b101 & ((1 << C) - 1), (1 << C) - 1):
        assert ops.propagate_ragged_plan([n] * C, S, D, mask) == ops.propagate_segments_plan(n, C, S, D, mask)
    for E in (2, 3):
        for first in (False, True):
            assert ops.propagate_ragged_plan([n] * C, S, D, int(first), E) == ops.propagate_edits_plan(n, C, S, D, first, E)


@pytest.mark.parametrize("n,S,D", [(2, 64, 320), (3, 45, 1280)])
def test_one_chunk_is_todays_plan(n, S, D):
    for mask in (0, 1):
        assert ops.propagate_ragged_plan([n], S, D, mask) == ops.propagate_segments_plan(n, 1, S, D, mask)
        assert ops.propagate_ragged_plan([n], S, D, mask, 2) == ops.propagate_edits_plan(n, 1, S, D, bool(mask), 2)


@pytest.mark.parametrize("S,D,form", rf.SMALL + rf.LARGE)
def test_ragged_tokens_and_the_form_rule(S, D, form):
    """',ragged' in the search token and on the gather; the form is the uniform C-chunk search's at the mean chunk size, and it
    is the form every chunk's own one-chunk search takes at these shapes (the precondition of the GPU identity tests)."""
    lists = rf.SMALL_FRAMES if (S, D, form) in rf.SMALL else rf.LARGE_FRAMES
    for frames in lists:
        if len(set(frames)) == 1:
            continue
        C, F = len(frames), sum(frames)
        for mask, _slot0 in rf.masks(C):
            for E in (1, 2):
                if E > 1 and mask > 1:
                    continue
                plan = ops.propagate_ragged_plan(frames, S, D, mask, E)
                assert len(plan) == 2 and plan[1] == f"gather[branches={1 + 2 * E},ragged]", plan
                m = re.fullmatch(r"(.+)\[splits=(\d+),ragged\]", plan[0])
                assert m and m.group(1) == form, plan
                mean = -(-F * S // C)
                assert ops.nn_plan(mean, S, D, 2, C)[0].split("[")[0] == form
        for n in set(frames):
            for P in (1, 2):
                assert ops.nn_plan(n * S, S, D, P)[0].split("[")[0] == form, (n, P)


def test_split_rule_takes_the_real_panel_count():
    """wide at (4040, 72): 128-target panels, 32 pivot tiles of 128.  [2, 3, 2] has 64 + 95 + 64 = 223 panels x 2 keyframes; the
    multi-chunk rule doubles the splits while the grid is below 4096 workgroups and a split keeps >= 128 pivots: 446 -> 16."""
    panels = sum(-(-n * 4040 // 128) for n in (2, 3, 2))
    assert panels == 223
    splits = 1
    while panels * 2 * splits < 4096 and splits * 2 <= 32:
        splits *= 2
    assert ops.propagate_ragged_plan([2, 3, 2], 4040, 72)[0] == f"wide[splits={splits},ragged]"


def _plan_rc(frames, C=None, S=64, D=320, mask=0, n_edits=1):
    buf = ctypes.create_string_buffer(512)
    arr = None if frames is None else (ctypes.c_int * max(len(frames), 1))(*frames)
    return _lib.load().tf_nn_gather_blend_ragged_plan(arr, len(frames) if C is None else C, S, D, mask, n_edits, buf, len(buf))


def test_plan_refusals():
    assert _plan_rc([3, 1, 2]) == 2
    assert _plan_rc(None, C=3) == -1                      # null chunk_frames
    assert _plan_rc([], C=0) == -3                        # C outside 1 .. 64
    assert _plan_rc([1, 2] * 33) == -3
    assert _plan_rc([1, 2] * 32, mask=1 << 63) == 2       # C = 64: every bit is a chunk
    assert _plan_rc([3, 0, 2]) == -3                      # a chunk without frames
    assert _plan_rc([3, -1, 2]) == -3
    assert _plan_rc([3, 1, 2], mask=1 << 3) == -3         # a bit at C
    assert _plan_rc([3, 1, 2], D=324) == -3
    assert _plan_rc([3, 1, 2], n_edits=0) == -3
    assert _plan_rc([3, 1, 2], n_edits=_lib.TF_MAX_EDITS + 1) == -3
    assert _plan_rc([3, 1, 2], mask=0b10, n_edits=2) == -3   # segments and multi-edit batches do not combine
    assert _plan_rc([3, 1, 2], mask=0b01, n_edits=2) == 2
    # sum n_j * S >= 2^31: 2 * 2^15 frames of 2^15 tokens
    assert _plan_rc([1 << 15, (1 << 15) - 1], S=1 << 15) == 2
    assert _plan_rc([1 << 15, 1 << 15], S=1 << 15) == -3
    for bad in ([], [1] * 65, [2, 0]):
        with pytest.raises(ValueError):
            ops.propagate_ragged_plan(bad, 64, 320)
    with pytest.raises(ValueError):
        ops.propagate_ragged_plan([3, 1, 2], 64, 320, 1 << 3)


def test_call_refuses_before_the_device():
    """The entry points themselves with placeholder pointers: every refusal returns before a launch (no GPU here)."""
    lib = _lib.load()
    ph = 1 << 12
    fr = (ctypes.c_int * 3)(3, 1, 2)

    def rc(frames=fr, C=3, K=4, slot0=1, mask=0b100, n_edits=1, ws_bytes=1 << 40, tgt=ph, norm=False):
        head = (tgt, ph, ph, ph, ph, ph, ph, K, frames, C, 64, 320, slot0, mask, _lib.TF_BF16, _lib.TF_BF16, _lib.TF_BF16,
                _lib.TF_F32, _lib.TF_BF16, n_edits)
        if norm:
            return lib.tf_nn_gather_blend_chunks_norm_ragged(*head, ph, ph, 1e-5, _lib.TF_BF16, ph, _lib.TF_BF16, ph, ws_bytes, None)
        return lib.tf_nn_gather_blend_chunks_ragged(*head, ph, ws_bytes, None)

    for norm in (False, True):
        assert rc(slot0=0, norm=norm) == -3                # chunk 0 blends slot0 - 1 unless bit 0 is set
        assert rc(mask=1 << 3, norm=norm) == -3
        assert rc(K=3, norm=norm) == -3                    # slot0 + C > K
        assert rc(C=0, norm=norm) == -3
        assert rc(C=65, K=70, norm=norm) == -3
        assert rc(frames=(ctypes.c_int * 3)(3, 0, 2), norm=norm) == -3
        assert rc(frames=None, norm=norm) == -1
        assert rc(tgt=None, norm=norm) == -1
        assert rc(tgt=ph + 2, norm=norm) == -4
        assert rc(ws_bytes=0, norm=norm) == -5
        assert rc(n_edits=2, norm=norm) == -3              # mask 0b100 with two edits
        assert rc(n_edits=9, mask=0, norm=norm) == -3


def test_workspace_bytes():
    lib = _lib.load()

    def ws(frames, S, D):
        return lib.tf_nn_gather_blend_ragged_workspace_bytes((ctypes.c_int * len(frames))(*frames), len(frames), S, D)

    # equal frames: the chunk form's scratch
    assert ws([2] * 5, 256, 640) == lib.tf_nn_gather_blend_chunks_workspace_bytes(2 * 256, 256, 640, 5)
    # ragged: splits x 2 keyframes x targets x 8 bytes
    for frames, S, D in (([2, 3, 2], 4040, 72), ([3, 1, 2, 5], 96, 320), ([3, 2, 3, 2], 2180, 640)):
        splits = int(re.search(r"splits=(\d+)", ops.propagate_ragged_plan(frames, S, D)[0]).group(1))
        assert ws(frames, S, D) == max(256, splits * 2 * sum(frames) * S * 8)
    assert ws([3, 0], 64, 320) == 0 and lib.tf_nn_gather_blend_ragged_workspace_bytes(None, 2, 64, 320) == 0
