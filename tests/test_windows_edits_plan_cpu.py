"""Launch plans of the sliding-window bank entry point for a multi-edit batch (tf_ext_attn_fwd_windows_edits) on the host: the
plan function runs the real dispatch under the plan recorder and touches no device.  One edit IS the windowed call, full
windows ARE the masked multi-edit call; otherwise ONE pre-pass, every bank launch marked ',win', the source launch plain, and
with the four-bank hint exactly one 'MV4,..,win' launch per pair of injecting edits; every refusal comes back as an error."""
import ctypes
import os
import re

import pytest
import torch

from tokenflow_amd import _lib, ops

NEW_SYMBOLS = ("tf_ext_attn_fwd_windows_edits", "tf_ext_attn_windows_edits_plan")
K = 6
R1 = ops.bank_windows(K, 1)
IRREGULAR = [(0, 1), (0, 3), (1, 4), (3, 1), (2, 4), (4, 2)]
TABLES = {"R1": R1, "irregular": IRREGULAR}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tokenflow_hip.h")


def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"TF_API\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_abi_exports_and_signatures():
    lib = _lib.load()
    assert lib.tf_abi_version() == 11 and _lib.ABI_VERSION == 11
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    fwd = _declaration("tf_ext_attn_fwd_windows_edits")
    assert fwd == ["const void* q", "const void* k", "const void* v", "void* out", "int K", "int Kq", "int q_frame0", "int S", "int H",
                   "int Dh", "int64_t ld", "const int64_t* strides", "float scale", "int flags", "int dtype", "int n_edits",
                   "unsigned inject_mask", "const int* win_lo", "const int* win_n", "void* ws", "size_t ws_bytes", "void* stream"]
    plan = _declaration("tf_ext_attn_windows_edits_plan")
    assert plan == ["int K", "int Kq", "int q_frame0", "int S", "int H", "int Dh", "int n_edits", "unsigned inject_mask", "int flags",
                    "int dtype", "const int* win_lo", "const int* win_n", "char* buf", "size_t len"]
    # the ctypes signatures: one argument type per declared argument, of the declared kind
    kind = lambda a: (ctypes.c_void_p if "*" in a and "char*" not in a else ctypes.c_char_p if "char*" in a else      # noqa: E731
                      ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_float if a.startswith("float") else
                      ctypes.c_size_t if a.startswith("size_t") else ctypes.c_uint if a.startswith("unsigned") else ctypes.c_int)
    for name, decl in zip(NEW_SYMBOLS, (fwd, plan)):
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and list(args) == [kind(a) for a in decl], name


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("S,H,Dh,kw", [(48, 2, 40, {}), (320, 2, 64, {"fused": False}), (576, 2, 64, {"fused": False, "no_split": True}),
                                      (1024, 8, 40, {}), (128, 2, 160, {"out_dtype": torch.float32})])
def test_one_edit_is_the_windowed_call(table, S, H, Dh, kw):
    for inject in (False, True):
        for mv in ({}, {"multi_v": True}, {"multi_v": False}, {"multi_v64": True}):      # the hints have nothing to select
            assert ops.attn_windows_edits_plan(K, TABLES[table], S, H, Dh, 1, int(inject), **kw, **mv) == \
                ops.attn_windows_plan(K, TABLES[table], S, H, Dh, inject, **kw)


@pytest.mark.parametrize("Kb,S,H,Dh,kw", [(5, 48, 2, 40, {}), (6, 320, 2, 64, {"fused": False}), (8, 1024, 8, 40, {}),
                                         (10, 9216, 5, 64, {}), (6, 512, 2, 40, {"fused": False, "no_split": True}),
                                         (6, 320, 2, 64, {"fused": False, "multi_v64": True}), (6, 192, 2, 160, {})])
def test_full_windows_are_the_masked_multi_edit_call(Kb, S, H, Dh, kw):
    """Token for token, the measured whole-bank defaults of the four-bank form included ((8, 1024, 8, 40), (10, 9216, 5, 64))."""
    for E, mask in ((2, 0), (2, 0b11), (3, 0b101), (3, 0b010)):
        for radius in (Kb - 1, Kb + 3):
            assert ops.attn_windows_edits_plan(Kb, ops.bank_windows(Kb, radius), S, H, Dh, E, mask, **kw) == \
                ops.attn_edits_plan(Kb, Kb, S, H, Dh, False, E, inject_mask=mask, **kw)


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("S,Dh", [(320, 64), (512, 40)])
def test_composition_of_three_edits_with_a_mixed_mask(table, S, Dh):
    """E = 3, mask 0b101, one pass, streaming: ONE pre-pass; every bank launch reads the windows, the source launch does not;
    with the four-bank hint the two injecting edits (not neighbours) are ONE windowed four-bank launch and the remaining edit
    follows it."""
    H, wins = 2, TABLES[table]
    plan = ops.attn_windows_edits_plan(K, wins, S, H, Dh, 3, 0b101, no_split=True, fused=False, multi_v=False)
    assert plan.count("vt_pack") == 1 and plan[0] == "vt_pack", plan
    assert len(plan) == 5 and all(t.endswith(",win") for t in plan[1:4]) and ",win" not in plan[4], plan
    assert [("DUAL" in t, "ALL" in t) for t in plan[1:4]] == [(True, False), (True, False), (False, True)], plan
    assert "SOURCE" in plan[4] and not any("MV4" in t for t in plan), plan
    # the single-edit windowed call of each edit names the same bank launch
    for e, inj in enumerate((True, False, True)):
        own = ops.attn_windows_plan(K, wins, S, H, Dh, inj, no_split=True, fused=False)
        assert own[1] == plan[1 + (0, 2, 1)[e]], (e, own, plan)
    hint = {"multi_v": True} if Dh == 40 else {"multi_v64": True}
    token = "one<40,1,4,MV4,2,fq0>,win" if Dh == 40 else "one<64,1,8,MV4,2,fq1>,win"
    mv = ops.attn_windows_edits_plan(K, wins, S, H, Dh, 3, 0b101, no_split=True, fused=False, **hint)
    assert mv.count("vt_pack") == 1 and mv[0] == "vt_pack" and len(mv) == 4, mv
    assert [t for t in mv if "MV4" in t] == [token] and mv[1] == token, mv
    assert mv[2].endswith(",win") and "ALL" in mv[2] and "SOURCE" in mv[3] and ",win" not in mv[3], mv
    # the other head dim's hint selects nothing; multi_v=False switches the form off
    other = {"multi_v64": True} if Dh == 40 else {"multi_v": True}
    assert ops.attn_windows_edits_plan(K, wins, S, H, Dh, 3, 0b101, no_split=True, fused=False, **other) == \
        ops.attn_windows_edits_plan(K, wins, S, H, Dh, 3, 0b101, no_split=True, fused=False)
    # three injecting edits: a pair and the odd edit in the DUAL launch beside it, both windowed, both one pass
    odd = ops.attn_windows_edits_plan(K, wins, S, H, Dh, 3, 0b111, fused=False, **hint)
    assert odd[:2] == ["vt_pack", token] and "DUAL" in odd[2] and odd[2].endswith(",win") and len(odd) == 4, odd
    assert not any(t.startswith("merge") for t in odd), odd


def test_pair_launches_are_one_pass_and_planned_for_the_longest_window():
    """The default mode splits the windows of this grid (merge launches); a pair launch stays one pass.  The kernel forms are
    those of a bank of K' = max win_n frames: the plan of the full-bank call at K = K'."""
    S, H, Dh = 320, 2, 64
    plan = ops.attn_windows_edits_plan(K, IRREGULAR, S, H, Dh, 2, 0b11, fused=False, multi_v=False)
    assert plan.count("merge[nseg=4]") == 2, plan
    mv = ops.attn_windows_edits_plan(K, IRREGULAR, S, H, Dh, 2, 0b11, fused=False, multi_v64=True)
    assert mv == ["vt_pack", "one<64,1,8,MV4,2,fq1>,win", "one<64,1,4,SOURCE,2,fq1>"], mv
    Kmax = max(n for _, n in IRREGULAR)
    for mask in (0, 0b01, 0b11):
        win = ops.attn_windows_edits_plan(K, IRREGULAR, S, H, Dh, 2, mask, fused=False, multi_v=False)
        assert [t.replace(",win", "") for t in win] == \
            ops.attn_edits_plan(Kmax, Kmax, S, H, Dh, False, 2, inject_mask=mask, fused=False, multi_v=False), (mask, win)


def test_default_of_the_four_bank_form_in_a_windowed_call():
    """Without a hint a windowed call takes the four-bank form only where profiles/r19_window_edits_ab.txt measured it ahead of
    the DUAL composition: radius 2 at the level-0 shapes of BASELINE configs 5, 4 and 2.  The whole-bank defaults say nothing
    about windows ((8, 1024, 8, 40) and (25, 1024, 10, 64) take the form on a whole bank and not on windows); the hints override
    the rule both ways."""
    mv = lambda plan: sum("MV4" in t and t.endswith(",win") for t in plan)      # noqa: E731
    for Kb, S, H, Dh, R, want in ((25, 4096, 5, 64, 2, 1), (10, 9216, 5, 64, 2, 1), (8, 4096, 8, 40, 2, 1), (16, 4096, 5, 64, 2, 1),
                                  (25, 4096, 5, 64, 1, 0), (25, 4096, 5, 64, 3, 0), (8, 4096, 8, 40, 1, 0), (8, 1024, 8, 40, 2, 0),
                                  (25, 1024, 10, 64, 2, 0), (6, 4096, 8, 40, 2, 0)):
        wins = ops.bank_windows(Kb, R)
        hint = {"multi_v": True} if Dh == 40 else {"multi_v64": True}
        for E, mask in ((2, 0b11), (3, 0b111), (3, 0b101)):
            assert mv(ops.attn_windows_edits_plan(Kb, wins, S, H, Dh, E, mask)) == want, (Kb, S, H, Dh, R)
            assert mv(ops.attn_windows_edits_plan(Kb, wins, S, H, Dh, E, mask, **hint)) == 1
            assert mv(ops.attn_windows_edits_plan(Kb, wins, S, H, Dh, E, mask, multi_v=False)) == 0
        assert mv(ops.attn_windows_edits_plan(Kb, wins, S, H, Dh, 2, 0b01)) == 0      # one injecting edit: no pair
    for Kb, S, H, Dh in ((8, 1024, 8, 40), (25, 1024, 10, 64)):
        assert any("MV4" in t for t in ops.attn_edits_plan(Kb, Kb, S, H, Dh, True, 2))


def test_refusals():
    S, H, Dh, E = 64, 2, 40, 2
    plan = lambda **kw: ops.attn_windows_edits_plan(K, kw.pop("windows", R1), S, H, Dh, kw.pop("E", E), kw.pop("mask", 0), **kw)      # noqa: E731
    assert plan()
    # the table: what the windowed call refuses (ops checks it first; the library's own check is exercised below)
    for bad in (R1[:-1], [(0, 2)] * K, [(0, 0)] + R1[1:], [(0, 2)] * (K - 1) + [(4, 3)], [(-1, 2)] + R1[1:]):
        with pytest.raises(ValueError):
            plan(windows=bad)
    with pytest.raises(ValueError):
        ops.attn_windows_edits_plan(65, ops.bank_windows(65, 1), S, H, Dh, E, 0)          # Kq > TF_MAX_WINDOW_FRAMES
    # flags without a windowed form
    for bits in (_lib.TF_ATTN_FOLD_SCALE, _lib.TF_ATTN_BANK_ONLY, _lib.TF_ATTN_SOURCE_ONLY, _lib.TF_ATTN_RUN_MULTI_V):
        with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_fwd_windows_edits"):
            plan(hints=bits)
    # what the masked call refuses
    with pytest.raises(_lib.TokenflowHipError, match="TF_ATTN_INJECT beside a mask"):
        plan(hints=_lib.TF_ATTN_INJECT)
    with pytest.raises(_lib.TokenflowHipError, match="exclude each other"):
        plan(hints=_lib.TF_ATTN_MULTI_V, multi_v=False)
    with pytest.raises(_lib.TokenflowHipError, match="exclude each other"):
        plan(multi_v=False, multi_v64=True)
    for E_bad, mask in ((2, 0b100), (2, -1), (0, 0), (_lib.TF_MAX_EDITS + 1, 0)):
        with pytest.raises(ValueError):
            plan(E=E_bad, mask=mask)
    # the library's own checks, past the Python layer: TF_ERR_SHAPE (-3), TF_ERR_NULL (-1) for a missing table
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1024)
    arr = lambda xs: ctypes.cast((ctypes.c_int * len(xs))(*xs), ctypes.c_void_p)      # noqa: E731

    def raw(lo, n, Kb=K, Kq=K, E_=E, mask=0, flags=0):
        return lib.tf_ext_attn_windows_edits_plan(Kb, Kq, 0, S, H, Dh, E_, mask, flags, _lib.TF_BF16, lo, n, buf, len(buf))
    lo, n = [w[0] for w in R1], [w[1] for w in R1]
    assert raw(arr(lo), arr(n)) > 0
    assert raw(None, arr(n)) == -1 and raw(arr(lo), None) == -1
    assert raw(arr([0] * K), arr([2] * K)) == -3                                         # a window without its own frame
    assert raw(arr(lo), arr([0] + n[1:])) == -3 and raw(arr(lo), arr(n[:-1] + [3])) == -3   # empty / outside the bank
    lo65, n65 = zip(*ops.bank_windows(65, 1))
    assert raw(arr(list(lo65)), arr(list(n65)), Kb=65, Kq=65) == -3
    assert raw(arr(lo), arr(n), mask=0b100) == -3 and raw(arr(lo), arr(n), E_=0) == -3 and raw(arr(lo), arr(n), E_=9) == -3
    assert raw(arr(lo), arr(n), E_=1, mask=0b10) == -3 and raw(arr(lo), arr(n), E_=1, flags=_lib.TF_ATTN_INJECT) == -3
    for bits in (_lib.TF_ATTN_FOLD_SCALE, _lib.TF_ATTN_BANK_ONLY, _lib.TF_ATTN_SOURCE_ONLY, _lib.TF_ATTN_RUN_MULTI_V,
                 _lib.TF_ATTN_INJECT, _lib.TF_ATTN_MULTI_V | _lib.TF_ATTN_NO_MULTI_V, _lib.TF_ATTN_MULTI_V64 | _lib.TF_ATTN_NO_MULTI_V):
        assert raw(arr(lo), arr(n), flags=bits) == -3, bits
    for bits in (_lib.TF_ATTN_MULTI_V, _lib.TF_ATTN_NO_MULTI_V, _lib.TF_ATTN_MULTI_V64):   # accepted here ...
        assert raw(arr(lo), arr(n), flags=bits) > 0, bits
    # ... while the plain windowed call keeps refusing them
    for bits in (_lib.TF_ATTN_MULTI_V, _lib.TF_ATTN_NO_MULTI_V, _lib.TF_ATTN_MULTI_V64):
        with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_fwd_windows"):
            ops.attn_windows_plan(K, R1, S, H, Dh, True, hints=bits)
