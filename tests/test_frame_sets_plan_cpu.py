"""Launch plans of the frame-set bank entry point (tf_ext_attn_fwd_frame_sets) on the host: the plan function runs the real
dispatch under the plan recorder and touches no device.  A table of contiguous ranges IS the windowed call (and the plain call
where every range is the bank); anything else issues the launches of the plain call for a bank of max_i popcount(sets[i])
frames, with ',set' appended to the launch that holds the bank problems; a null table is TF_ERR_NULL (-1), every other refusal
TF_ERR_SHAPE (-3)."""
import ctypes
import os
import re

import pytest
import torch

from tokenflow_amd import _lib, ops

NEW_SYMBOLS = ("tf_ext_attn_fwd_frame_sets", "tf_ext_attn_frame_sets_plan")
K_ATTN = 6
IRREGULAR = [(0, 1), (0, 3), (1, 4), (3, 1), (2, 4), (4, 2)]      # the windowed suite's table with windows of 1 and 3 frames


def mask(*frames):
    m = 0
    for f in frames:
        m |= 1 << f
    return m


# the set tables of the GPU suite, written out
TABLES = {
    "R1+a0": [mask(0, 1), mask(0, 1, 2), mask(0, 1, 2, 3), mask(0, 2, 3, 4), mask(0, 3, 4, 5), mask(0, 4, 5)],
    "R1+a0a5": [mask(0, 1, 5), mask(0, 1, 2, 5), mask(0, 1, 2, 3, 5), mask(0, 2, 3, 4, 5), mask(0, 3, 4, 5), mask(0, 4, 5)],
    "scattered": [mask(0), mask(1, 3, 5), mask(0, 2, 4), mask(0, 3), mask(1, 2, 4, 5), mask(0, 5)],
}
K_MAX = {"R1+a0": 4, "R1+a0a5": 5, "scattered": 4}

# (S, H, Dh, kwargs, form of the bank launch under no_split): the cases of tests/test_windows_gpu.py
ATTN_CASES = [
    (48, 2, 40, {}, "fused"),
    (192, 2, 160, {}, "fused"),
    (320, 2, 64, {"fused": False}, "one<64"),
    (512, 2, 40, {"fused": False, "hints": _lib.TF_ATTN_HINT_MIX}, "il<40"),
    (576, 2, 64, {"fused": False}, "il<64"),
    (520, 2, 64, {"fused": False}, "pp<64"),
    (320, 2, 80, {}, "il<80"),
    (128, 2, 160, {"fused": False}, "one<160"),
]


def as_masks(windows):
    return [((1 << n) - 1) << lo for lo, n in windows]


def test_abi_and_exports():
    lib = _lib.load()
    assert lib.tf_abi_version() == 11 and _lib.ABI_VERSION == 11
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_header_declares_the_two_functions():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tokenflow_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("TF_API int tf_ext_attn_fwd_frame_sets(const void* q, const void* k, const void* v, void* out, int K, int Kq, "
            "int q_frame0, int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags, int dtype, "
            "const uint64_t* sets, void* ws, size_t ws_bytes, void* stream);") in flat
    assert ("TF_API int tf_ext_attn_frame_sets_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int flags, int dtype, "
            "const uint64_t* sets, char* buf, size_t len);") in flat
    assert "#define TF_ABI_VERSION 11" in flat


def test_bank_frame_sets():
    assert ops.bank_frame_sets(6, 1, [0]) == TABLES["R1+a0"]
    assert ops.bank_frame_sets(6, 1, (0, 5, 5, 0)) == TABLES["R1+a0a5"]
    assert ops.bank_frame_sets(6, 1) == ops.bank_frame_sets(6, 1, []) == as_masks(ops.bank_windows(6, 1))
    assert ops.bank_frame_sets(5, 9, [3]) == [31] * 5
    assert max(bin(m).count("1") for m in ops.bank_frame_sets(25, 2, range(0, 25, 8))) <= 2 * 2 + 1 + 4
    assert [max(bin(m).count("1") for m in TABLES[t]) for t in TABLES] == [K_MAX[t] for t in TABLES]
    for bad in ([6], [-1], [1.5], [True]):
        with pytest.raises(ValueError, match="anchor"):
            ops.bank_frame_sets(6, 1, bad)
    with pytest.raises(ValueError):
        ops.bank_frame_sets(0, 1)


@pytest.mark.parametrize("S,H,Dh,kw,form", ATTN_CASES, ids=[f"S{c[0]}-Dh{c[2]}" for c in ATTN_CASES])
@pytest.mark.parametrize("inject", [False, True])
def test_contiguous_sets_are_the_windowed_call(S, H, Dh, kw, form, inject):
    """Token for token, ',win' and no ',set': ranges delegate to tf_ext_attn_fwd_windows, whole banks on to the plain call."""
    K = K_ATTN
    for windows in (ops.bank_windows(K, 1), ops.bank_windows(K, 2), IRREGULAR):
        for no_split in (False, True):
            plan = ops.attn_frame_sets_plan(K, as_masks(windows), S, H, Dh, inject, no_split=no_split, **kw)
            assert plan == ops.attn_windows_plan(K, windows, S, H, Dh, inject, no_split=no_split, **kw)
            assert any(",win" in t for t in plan) and not any(",set" in t for t in plan), plan
    for kw2 in (kw, dict(kw, no_split=True), dict(kw, out_dtype=torch.float32)):
        assert ops.attn_frame_sets_plan(K, [mask(*range(K))] * K, S, H, Dh, inject, **kw2) == ops.attn_plan(K, K, S, H, Dh, inject, **kw2)


@pytest.mark.parametrize("S,H,Dh,kw,form", ATTN_CASES, ids=[f"S{c[0]}-Dh{c[2]}" for c in ATTN_CASES])
@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("inject", [False, True])
def test_set_plan(S, H, Dh, kw, form, table, inject):
    """The launches of the plain call for a bank of K' frames: ONE ',set' launch of the named form under no_split, ONE pre-pass
    unless the launch is fused, merge and source launches as in the plain call."""
    K, sets = K_ATTN, TABLES[table]
    plans = {ns: ops.attn_frame_sets_plan(K, sets, S, H, Dh, inject, no_split=ns, **kw) for ns in (False, True)}
    for ns, plan in plans.items():
        marked = [t for t in plan if t.endswith(",set") or t.endswith(",set]")]
        assert len(marked) == 1 and not any(",win" in t for t in plan), plan
        assert plan.count("vt_pack") == (0 if plan[0].startswith("fused") else 1), plan
        # the tokens of a Kq = K call on a bank of K' frames: the same forms, the same split, the same merge and source launches
        # (the plan function takes the query frames of its bank, so the windowed plan of K'-frame ranges stands in for it)
        ranges = [(max(0, min(i, K - K_MAX[table])), K_MAX[table]) for i in range(K)]
        assert [t.replace(",set", "") for t in plan] == \
            [t.replace(",win", "") for t in ops.attn_windows_plan(K, ranges, S, H, Dh, inject, no_split=ns, **kw)], plan
    want = "one<64" if inject and form == "pp<64" else form      # (injection at Dh 64, ragged S: the DUAL one-tile form)
    marked = [t for t in plans[True] if ",set" in t]
    assert marked[0].startswith(want), plans[True]
    assert not any(t.startswith("merge") for t in plans[True]), plans[True]
    if table == "scattered":      # where the windowed `irregular` table splits into 4 runs, so does this one: empty runs
        irregular = ops.attn_windows_plan(K, IRREGULAR, S, H, Dh, inject, no_split=False, **kw)
        assert ("merge[nseg=4]" in plans[False]) == ("merge[nseg=4]" in irregular), (plans[False], irregular)
        if not plans[False][0].startswith("fused") and Dh != 160:
            assert "merge[nseg=4]" in plans[False], plans[False]


def _plan_rc(K, Kq, q_frame0, sets, flags=0, S=64, H=2, Dh=40):
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.c_uint64 * len(sets))(*sets)
    return lib.tf_ext_attn_frame_sets_plan(K, Kq, q_frame0, S, H, Dh, flags, _lib.TF_BF16, ctypes.cast(a, ctypes.c_void_p), buf,
                                           len(buf)), buf.value.decode()


def _last_error():
    return _lib.load().tf_last_error().decode()


def test_refusals():
    TF_ERR_SHAPE, TF_ERR_NULL = -3, -1
    good = [mask(0, 1), mask(1, 3), mask(0, 2), mask(0, 3)]
    ok = _plan_rc(4, 4, 0, good)
    assert ok[0] == 1 and ok[1].endswith(",set]"), ok
    # K > 64: a set is a 64-bit mask (full sets included); 64 is fine
    assert _plan_rc(65, 4, 0, good)[0] == TF_ERR_SHAPE
    assert "at most 64 bank frames" in _last_error()
    assert _plan_rc(64, 64, 0, [mask(i, 63 - i) for i in range(64)], S=32)[0] > 0
    assert _plan_rc(64, 64, 0, [(1 << 64) - 1] * 64, S=32)[0] > 0
    # Kq > TF_MAX_WINDOW_FRAMES cannot be reached with K <= 64: the bank check answers
    assert _lib.TF_MAX_WINDOW_FRAMES == 64
    # an empty set / a bit at or above K / a set without its own frame
    for sets, what in (([mask(0, 1), 0, mask(0, 2), mask(0, 3)], "is empty"),
                       ([mask(0, 1), mask(1, 4), mask(0, 2), mask(0, 3)], "at or above"),
                       ([mask(0, 1), mask(1, 3), mask(0, 2), mask(0, 3, 63)], "at or above"),
                       ([mask(0, 1), mask(0, 3), mask(0, 2), mask(0, 3)], "own frame"),
                       ([mask(1), mask(1, 3), mask(0, 2), mask(0, 3)], "own frame")):
        assert _plan_rc(4, 4, 0, sets)[0] == TF_ERR_SHAPE, sets
        assert what in _last_error(), (what, _last_error())
    # the own frame is the BANK frame q_frame0 + i
    assert _plan_rc(6, 2, 3, [mask(0, 3), mask(1, 4)])[0] > 0
    assert _plan_rc(6, 2, 3, [mask(0, 2), mask(1, 4)])[0] == TF_ERR_SHAPE
    # the flags the windowed call refuses, on set tables, on ranges and on full sets: the check comes before the delegation
    for flag in (_lib.TF_ATTN_BANK_ONLY, _lib.TF_ATTN_SOURCE_ONLY, _lib.TF_ATTN_FOLD_SCALE, _lib.TF_ATTN_MULTI_V,
                 _lib.TF_ATTN_NO_MULTI_V, _lib.TF_ATTN_MULTI_V64, _lib.TF_ATTN_RUN_MULTI_V):
        for sets in (good, as_masks(ops.bank_windows(4, 1)), [15] * 4):
            assert _plan_rc(4, 4, 0, sets, flags=flag)[0] == TF_ERR_SHAPE, (flag, sets)
            assert "no frame-set form" in _last_error()
    # a null table
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    assert lib.tf_ext_attn_frame_sets_plan(4, 4, 0, 64, 2, 40, 0, _lib.TF_BF16, None, buf, len(buf)) == TF_ERR_NULL


@pytest.mark.parametrize("S,H,Dh,flags", [(1024, 8, 40, 0), (1024, 8, 40, _lib.TF_ATTN_INJECT), (64, 5, 64, _lib.TF_ATTN_NO_FUSED),
                                          (2304, 10, 64, _lib.TF_ATTN_INJECT), (256, 8, 40, 0)])
def test_forms_are_those_of_the_largest_set(S, H, Dh, flags):
    """The fused decision, the split and the kernel forms follow max popcount at the call's Kq -- not the bank size, not the span
    of a set, not the other sets."""
    a = _plan_rc(8, 4, 0, [mask(0, 2), mask(1, 3, 5), mask(0, 2, 4), mask(3, 7)], flags, S, H, Dh)
    b = _plan_rc(25, 4, 0, [mask(0, 24), mask(1, 12, 20), mask(2, 3, 24), mask(0, 3)], flags, S, H, Dh)
    c = _plan_rc(25, 4, 10, [mask(10), mask(0, 11, 24), mask(12), mask(13)], flags, S, H, Dh)
    assert a[0] > 0 and a == b == c, (a, b, c)
    ranges = _plan_rc(25, 4, 0, as_masks([(0, 2), (0, 3), (1, 3), (2, 2)]), flags, S, H, Dh)
    assert a[1].replace(",set", "") == ranges[1].replace(",win", "") and a[1] != ranges[1], (a, ranges)


@pytest.mark.parametrize("S,H,Dh", [(64, 2, 40), (256, 8, 40), (1024, 8, 40), (576, 5, 64), (320, 2, 80), (128, 2, 160), (4096, 5, 64)])
def test_partial_results_of_every_set_size_fit_the_banks_workspace(S, H, Dh):
    """The split form's partial results live in the workspace of the K-frame bank while the split is planned for the largest set
    K' < K: the call checks the fit and would answer TF_ERR_WORKSPACE (-5).  The sweep of tests/test_windows_plan_cpu.py over
    dilated sets (every second frame around the own one, clipped to the bank): no bank of up to 64 keyframes and no set size
    refuses."""
    for K in range(3, 65):
        for n in range(1, K // 2 + 1):
            sets = []
            for i in range(K):
                same = list(range(i % 2, K, 2))                      # the frames of i's parity; n of them around i
                j = max(0, min(i // 2 - n // 2, len(same) - n))
                sets.append(mask(*same[j:j + n]))
                assert (sets[-1] >> i) & 1 and not sets[-1] >> K and bin(sets[-1]).count("1") == n, (K, n, i, bin(sets[-1]))
            for flags in (_lib.TF_ATTN_NO_FUSED, _lib.TF_ATTN_NO_FUSED | _lib.TF_ATTN_INJECT):
                rc, plan = _plan_rc(K, K, 0, sets, flags, S, H, Dh)
                assert rc > 0 and (",set" in plan or n == 1), (K, n, flags, rc, _last_error())


def test_ops_argument_errors():
    with pytest.raises(ValueError, match="sets for"):
        ops.attn_frame_sets_plan(4, [3] * 3, 64, 2, 40, False)
    with pytest.raises(ValueError, match="does not hold its own frame"):
        ops.attn_frame_sets_plan(4, [3, 3, 3, 12], 64, 2, 40, False)
    with pytest.raises(ValueError, match="inside"):
        ops.attn_frame_sets_plan(4, [3, 3, 4 | 16, 12], 64, 2, 40, False)
    with pytest.raises(ValueError, match="inside"):
        ops.attn_frame_sets_plan(4, [3, 0, 4, 12], 64, 2, 40, False)
    with pytest.raises(ValueError, match="at most 64 bank frames"):
        ops.attn_frame_sets_plan(65, [1 << (i % 64) for i in range(65)], 64, 2, 40, False)
    with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_frame_sets_plan"):
        ops.attn_frame_sets_plan(4, ops.bank_frame_sets(4, 1, [0]), 64, 2, 40, False, hints=_lib.TF_ATTN_MULTI_V)
