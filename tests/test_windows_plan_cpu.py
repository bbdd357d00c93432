"""Launch plans of the sliding-window bank entry point (tf_ext_attn_fwd_windows) on the host: the plan function runs the real
dispatch under the plan recorder and touches no device.  A windowed call issues the launches of the plain call for a bank of
max_i win_n[i] frames, with ',win' appended to the launch that holds the bank problems; full windows ARE the plain call; every
refusal comes back as TF_ERR_SHAPE (-3)."""
import ctypes
import re

import pytest

from tokenflow_amd import _lib, ops

NEW_SYMBOLS = ("tf_ext_attn_fwd_windows", "tf_ext_attn_windows_plan")
IRREGULAR = [(0, 1), (0, 3), (1, 4), (3, 1), (2, 4), (4, 2)]


def test_abi_and_exports():
    lib = _lib.load()
    assert lib.tf_abi_version() == 11 and _lib.ABI_VERSION == 11
    assert _lib.TF_MAX_WINDOW_FRAMES == 64
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_bank_windows():
    assert ops.bank_windows(6, 1) == [(0, 2), (0, 3), (1, 3), (2, 3), (3, 3), (4, 2)]
    assert ops.bank_windows(6, 2) == [(0, 3), (0, 4), (0, 5), (1, 5), (2, 4), (3, 3)]
    assert ops.bank_windows(4, 0) == [(i, 1) for i in range(4)]
    assert ops.bank_windows(5, 4) == ops.bank_windows(5, 99) == [(0, 5)] * 5
    assert sum(n for _, n in ops.bank_windows(25, 2)) == 119          # against 625 frame-banks of the full bank
    for bad in ((0, 1), (3, -1)):
        with pytest.raises(ValueError):
            ops.bank_windows(*bad)


@pytest.mark.parametrize("K,S,H,Dh,inject,kw", [
    (5, 48, 2, 40, True, {}),
    (5, 320, 2, 80, False, {"no_split": True}),
    (8, 1024, 8, 40, True, {}),
    (4, 4096, 8, 40, True, {}),
    (5, 512, 2, 40, False, {"fused": False}),
    (10, 9216, 5, 64, True, {}),
    (6, 192, 2, 160, False, {"out_dtype": __import__("torch").float32}),
])
def test_full_windows_are_the_plain_call(K, S, H, Dh, inject, kw):
    """Token for token: every window = [0, K) delegates to tf_ext_attn_fwd_strided."""
    for radius in (K - 1, K + 3):
        assert ops.attn_windows_plan(K, ops.bank_windows(K, radius), S, H, Dh, inject, **kw) == \
            ops.attn_plan(K, K, S, H, Dh, inject, **kw)


STREAM_CASES = [
    (320, 4, 64, {"fused": False}, r"one<64,.*ALL.*>"),
    (512, 8, 40, {"fused": False, "hints": _lib.TF_ATTN_HINT_MIX}, r"il<40,8,ALL,4,3>"),
    (576, 2, 64, {"fused": False, "no_split": True}, r"il<64,.*ALL.*>"),
    (520, 2, 64, {"fused": False, "no_split": True}, r"pp<64,ALL>"),
    (512, 4, 80, {"fused": False}, r"il<80,.*ALL.*>"),
    (1024, 8, 40, {}, r"il<40,8,ALL.*>"),
    (4096, 5, 64, {}, r"il<64,8,ALL.*>"),
]


@pytest.mark.parametrize("windows", [ops.bank_windows(6, 1), ops.bank_windows(6, 2), IRREGULAR], ids=["R1", "R2", "irregular"])
@pytest.mark.parametrize("S,H,Dh,kw,bank", STREAM_CASES, ids=[f"S{c[0]}-Dh{c[2]}" for c in STREAM_CASES])
def test_streaming_plan(windows, S, H, Dh, kw, bank):
    """['vt_pack', '<bank token>,win', (merge), <source tokens>]: ONE pre-pass, ONE windowed launch."""
    K = 6
    plan = ops.attn_windows_plan(K, windows, S, H, Dh, False, **kw)
    assert plan[0] == "vt_pack" and plan.count("vt_pack") == 1, plan
    assert re.fullmatch(bank + ",win", plan[1]), plan
    assert sum(t.endswith(",win") for t in plan) == 1, plan
    assert all(re.fullmatch(r"merge\[nseg=\d+\]", t) for t in plan[2:]), plan          # the ALL form holds the source problems
    if kw.get("no_split"):
        assert len(plan) == 2, plan
    # under injection: the DUAL launch carries the windows, the source launch is the plain one
    plan = ops.attn_windows_plan(K, windows, S, H, Dh, True, **kw)
    assert plan[0] == "vt_pack" and plan.count("vt_pack") == 1, plan
    assert plan[1].endswith(",win") and ("DUAL" in plan[1] or Dh == 160 or S < 256), plan
    assert sum(t.endswith(",win") for t in plan) == 1, plan
    if "DUAL" in plan[1]:
        assert "SOURCE" in plan[-1] and not plan[-1].endswith(",win"), plan


@pytest.mark.parametrize("windows", [ops.bank_windows(6, 1), ops.bank_windows(6, 2), IRREGULAR], ids=["R1", "R2", "irregular"])
@pytest.mark.parametrize("S,H,Dh", [(48, 2, 40), (192, 2, 160), (64, 4, 64), (100, 4, 80)])
@pytest.mark.parametrize("no_split", [False, True])
def test_fused_plan(windows, S, H, Dh, no_split):
    """One fused launch, no pre-pass; under no_split the geometry of every frame's own call (a function of the shape alone)."""
    for inject in (False, True):
        plan = ops.attn_windows_plan(6, windows, S, H, Dh, inject, no_split=no_split)
        assert len(plan) == 1 and re.fullmatch(r"fused\[qw=\d,kw=\d,qb=\d,prec=\d,win\]", plan[0]), plan
        if no_split:
            for lo, n in windows:
                own = ops.attn_plan(n, 1, S, H, Dh, inject, no_split=True)
                assert len(own) == 1 and re.sub(r"qw=\d,", "", own[0][:-1]) == re.sub(r"qw=\d,", "", plan[0][:-5]), (own, plan)


def _plan_rc(K, Kq, q_frame0, lo, n, flags=0, S=64, H=2, Dh=40):
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.c_int * len(lo))(*lo)
    b = (ctypes.c_int * len(n))(*n)
    return lib.tf_ext_attn_windows_plan(K, Kq, q_frame0, S, H, Dh, flags, _lib.TF_BF16, ctypes.cast(a, ctypes.c_void_p),
                                        ctypes.cast(b, ctypes.c_void_p), buf, len(buf)), buf.value.decode()


@pytest.mark.parametrize("S,H,Dh,flags", [(1024, 8, 40, 0), (1024, 8, 40, _lib.TF_ATTN_INJECT), (64, 5, 64, _lib.TF_ATTN_NO_FUSED),
                                          (2304, 10, 64, _lib.TF_ATTN_INJECT), (256, 8, 40, 0)])
def test_forms_are_those_of_the_longest_window(S, H, Dh, flags):
    """The fused decision, the split and the kernel forms follow max win_n at the call's Kq -- not the bank size K, not the
    other windows: 4 query frames whose longest window holds 3 frames plan alike on a 4-frame and on a 25-frame bank."""
    a = _plan_rc(4, 4, 0, [0, 0, 1, 2], [2, 3, 3, 2], flags, S, H, Dh)
    b = _plan_rc(25, 4, 0, [0, 0, 1, 2], [2, 3, 3, 2], flags, S, H, Dh)
    c = _plan_rc(25, 4, 10, [10, 9, 12, 13], [1, 3, 1, 1], flags, S, H, Dh)
    assert a[0] > 0 and a == b == c, (a, b, c)
    longer = _plan_rc(25, 4, 0, [0, 0, 0, 0], [25, 2, 3, 4], flags, S, H, Dh)
    full = _plan_rc(25, 4, 0, [0] * 4, [25] * 4, flags, S, H, Dh)
    assert longer[1].replace(",win", "") == full[1] and longer[1] != full[1], (longer, full)


@pytest.mark.parametrize("S,H,Dh", [(64, 2, 40), (256, 8, 40), (1024, 8, 40), (576, 5, 64), (320, 2, 80), (128, 2, 160), (4096, 5, 64)])
def test_partial_results_of_every_window_length_fit_the_banks_workspace(S, H, Dh):
    """The split form's partial results live in the workspace of the K-frame bank (tf_ext_attn_workspace_bytes(K)), while the
    split is planned for the longest window K' < K: the call checks the fit and would answer TF_ERR_WORKSPACE (-5).  Sweep: no
    bank of up to 64 keyframes and no window length refuses."""
    for K in range(2, _lib.TF_MAX_WINDOW_FRAMES + 1):
        for n in range(1, K):
            lo = [max(0, min(i - n // 2, K - n)) for i in range(K)]       # n-frame windows that hold their own frame
            for flags in (_lib.TF_ATTN_NO_FUSED, _lib.TF_ATTN_NO_FUSED | _lib.TF_ATTN_INJECT):
                rc, plan = _plan_rc(K, K, 0, lo, [n] * K, flags, S, H, Dh)
                assert rc > 0 and ",win" in plan, (K, n, flags, rc, _lib.load().tf_last_error())


def test_refusals():
    TF_ERR_SHAPE, TF_ERR_NULL = -3, -1
    ok = _plan_rc(4, 4, 0, [0, 0, 1, 2], [2, 3, 3, 2])
    assert ok[0] == 1 and ok[1].endswith(",win]"), ok
    # Kq > TF_MAX_WINDOW_FRAMES (full windows included: the table has no room for them)
    K = _lib.TF_MAX_WINDOW_FRAMES + 1
    assert _plan_rc(K, K, 0, [0] * K, [K] * K)[0] == TF_ERR_SHAPE
    assert "query frames" in _lib.load().tf_last_error().decode()
    assert _plan_rc(K, K - 1, 0, [0] * (K - 1), [K] * (K - 1))[0] > 0           # 64 query frames of a 65-frame bank
    # a window without frames / outside [0, K) / without its own frame
    for lo, n, what in (([0, 0, 1, 2], [2, 0, 3, 2], "holds 0 frames"),
                        ([0, 0, 1, 2], [2, -1, 3, 2], "holds -1 frames"),
                        ([0, -1, 1, 2], [2, 3, 3, 2], "outside"),
                        ([0, 0, 1, 2], [2, 3, 3, 3], "outside"),
                        ([0, 0, 1, 2], [2, 5, 3, 2], "outside"),
                        ([0, 2, 1, 2], [2, 2, 3, 2], "own frame"),
                        ([0, 0, 0, 2], [2, 3, 2, 2], "own frame")):
        assert _plan_rc(4, 4, 0, lo, n)[0] == TF_ERR_SHAPE, (lo, n)
        assert what in _lib.load().tf_last_error().decode(), (what, _lib.load().tf_last_error())
    # the own frame is the BANK frame q_frame0 + i
    assert _plan_rc(6, 2, 3, [2, 3], [3, 3])[0] > 0
    assert _plan_rc(6, 2, 3, [0, 3], [3, 3])[0] == TF_ERR_SHAPE
    # flags without a windowed form
    for flag in (_lib.TF_ATTN_BANK_ONLY, _lib.TF_ATTN_SOURCE_ONLY, _lib.TF_ATTN_FOLD_SCALE, _lib.TF_ATTN_MULTI_V,
                 _lib.TF_ATTN_NO_MULTI_V, _lib.TF_ATTN_MULTI_V64, _lib.TF_ATTN_RUN_MULTI_V):
        assert _plan_rc(4, 4, 0, [0, 0, 1, 2], [2, 3, 3, 2], flags=flag)[0] == TF_ERR_SHAPE, flag
        assert "no windowed form" in _lib.load().tf_last_error().decode()
        # ... refused with full windows too: the check comes before the delegation
        assert _plan_rc(4, 4, 0, [0] * 4, [4] * 4, flags=flag)[0] == TF_ERR_SHAPE, flag
    # null tables
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    assert lib.tf_ext_attn_windows_plan(4, 4, 0, 64, 2, 40, 0, _lib.TF_BF16, None, None, buf, len(buf)) == TF_ERR_NULL


def test_ops_argument_errors():
    with pytest.raises(ValueError, match="windows for"):
        ops.attn_windows_plan(4, [(0, 2)] * 3, 64, 2, 40, False)
    with pytest.raises(ValueError, match="own frame"):
        ops.attn_windows_plan(4, [(0, 2), (0, 2), (0, 2), (2, 2)], 64, 2, 40, False)
    with pytest.raises(ValueError, match="inside"):
        ops.attn_windows_plan(4, [(0, 2), (0, 2), (2, 3), (2, 2)], 64, 2, 40, False)
    with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_windows_plan"):
        ops.attn_windows_plan(4, ops.bank_windows(4, 1), 64, 2, 40, False, hints=_lib.TF_ATTN_MULTI_V)
