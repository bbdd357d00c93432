"""Launch plans of the frame-set bank entry point for a multi-edit batch (tf_ext_attn_fwd_frame_sets_edits) on the host: the
plan function runs the real dispatch under the plan recorder and touches no device.  One edit IS the frame-set call, contiguous
sets ARE the windowed multi-edit call, full sets the masked multi-edit call; otherwise ONE pre-pass, every bank launch marked
',set', the source launch plain, and with the four-bank hint exactly one 'MV4,..,set' launch per pair of injecting edits; every
refusal comes back as an error that names the entry point."""
import ctypes
import os
import re

import pytest
import torch

from tokenflow_amd import _lib, ops
from tests.test_frame_sets_plan_cpu import IRREGULAR, K_MAX, TABLES, as_masks, mask

NEW_SYMBOLS = ("tf_ext_attn_fwd_frame_sets_edits", "tf_ext_attn_frame_sets_edits_plan")
K = 6
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tokenflow_hip.h")
MV4_SET = {40: "one<40,1,4,MV4,2,fq0>,set", 64: "one<64,1,8,MV4,2,fq1>,set"}

# (S, H, Dh, kwargs, form of a bank launch under no_split): the composition cases of the GPU suite
CASES = [
    (48, 2, 40, {}, "fused"),
    (320, 2, 64, {"fused": False}, "one<64"),
    (512, 2, 40, {"fused": False, "hints": _lib.TF_ATTN_HINT_MIX}, "il<40"),
    (576, 2, 64, {"fused": False}, "il<64"),
    (128, 2, 160, {"fused": False}, "one<160"),
]


def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"TF_API\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _set_marked(plan):
    return [t for t in plan if t.endswith(",set") or t.endswith(",set]")]


def test_abi_exports_and_signatures():
    lib = _lib.load()
    assert lib.tf_abi_version() == 11 and _lib.ABI_VERSION == 11
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    fwd = _declaration("tf_ext_attn_fwd_frame_sets_edits")
    assert fwd == ["const void* q", "const void* k", "const void* v", "void* out", "int K", "int Kq", "int q_frame0", "int S", "int H",
                   "int Dh", "int64_t ld", "const int64_t* strides", "float scale", "int flags", "int dtype", "int n_edits",
                   "unsigned inject_mask", "const uint64_t* sets", "void* ws", "size_t ws_bytes", "void* stream"]
    plan = _declaration("tf_ext_attn_frame_sets_edits_plan")
    assert plan == ["int K", "int Kq", "int q_frame0", "int S", "int H", "int Dh", "int n_edits", "unsigned inject_mask", "int flags",
                    "int dtype", "const uint64_t* sets", "char* buf", "size_t len"]
    kind = lambda a: (ctypes.c_void_p if "*" in a and "char*" not in a else ctypes.c_char_p if "char*" in a else      # noqa: E731
                      ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_float if a.startswith("float") else
                      ctypes.c_size_t if a.startswith("size_t") else ctypes.c_uint if a.startswith("unsigned") else ctypes.c_int)
    for name, decl in zip(NEW_SYMBOLS, (fwd, plan)):
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and list(args) == [kind(a) for a in decl], name
    flat = re.sub(r"\s+", " ", open(HEADER).read())
    assert "Not built: the four-bank form, multi-edit batches" not in flat      # the frame-set section's to-do list is updated


@pytest.mark.parametrize("table", ["R1+a0", "scattered"])
@pytest.mark.parametrize("S,H,Dh,kw,form", CASES, ids=[f"S{c[0]}-Dh{c[2]}" for c in CASES])
def test_composition(table, S, H, Dh, kw, form):
    """',set' on exactly E bank launches (merges beside them in the default mode), one pre-pass or none when everything is fused,
    the injecting edits first, the source launch last and plain; each edit names the bank launch of its own frame-set call."""
    sets = TABLES[table]
    for E, m in ((2, 0), (2, 0b11), (2, 0b01), (3, 0b101), (3, 0b111), (3, 0b010)):
        for ns in (False, True):
            plan = ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, E, m, no_split=ns, multi_v=False, **kw)
            marked = _set_marked(plan)
            assert len(marked) == E and not any(",win" in t or "MV4" in t for t in plan), plan
            streaming = [t for t in plan if not t.startswith("fused")]
            assert plan.count("vt_pack") == (1 if streaming else 0) and (not streaming or plan[0] == "vt_pack"), plan
            assert ",set" not in plan[-1] and ("SOURCE" in plan[-1] or plan[-1].startswith("fused")), plan
            if ns:
                assert not any(t.startswith("merge") for t in plan) and all(t.startswith(form) for t in marked), plan
                order = [e for e in range(E) if (m >> e) & 1] + [e for e in range(E) if not (m >> e) & 1]
                for pos, e in enumerate(order):
                    own = ops.attn_frame_sets_plan(K, sets, S, H, Dh, bool((m >> e) & 1), no_split=True, **kw)
                    assert _set_marked(own) == [marked[pos]], (e, own, plan)


@pytest.mark.parametrize("table", ["R1+a0", "scattered"])
@pytest.mark.parametrize("S,Dh", [(320, 64), (512, 40), (45, 40), (45, 64), (320, 40)])
def test_four_bank_set_form(table, S, Dh):
    """The hints at head dims 40 and 64: mask 0b101 pairs the two injecting edits that are no neighbours (gap 4) into ONE four-bank
    set launch, the third edit follows through its own set launch; three injecting edits are a pair and the odd one in the DUAL
    set launch; pair launches are one pass and never fused."""
    H, sets = 2, TABLES[table]
    hint = {"multi_v": True} if Dh == 40 else {"multi_v64": True}
    token = MV4_SET[Dh]
    mv = ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, 3, 0b101, no_split=True, fused=False, **hint)
    assert mv[:2] == ["vt_pack", token] and [t for t in mv if "MV4" in t] == [token] and len(mv) == 4, mv
    assert mv[2].endswith(",set") and "ALL" in mv[2] and "SOURCE" in mv[3] and ",set" not in mv[3], mv
    both = ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, 2, 0b11, **hint)        # default mode, fused allowed elsewhere
    assert both[:2] == ["vt_pack", token] and len(both) == 3 and ",set" not in both[2], both
    odd = ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, 3, 0b111, fused=False, **hint)
    assert odd[:2] == ["vt_pack", token] and "DUAL" in odd[2] and odd[2].endswith(",set") and len(odd) == 4, odd
    assert not any(t.startswith("merge") for t in odd), odd
    # the other head dim's hint selects nothing; multi_v=False switches the form off; one injecting edit is no pair
    other = {"multi_v64": True} if Dh == 40 else {"multi_v": True}
    plain = ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, 3, 0b101, no_split=True, fused=False)
    assert ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, 3, 0b101, no_split=True, fused=False, **other) == plain
    assert ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, 3, 0b101, no_split=True, fused=False, multi_v=False) == plain
    assert not any("MV4" in t for t in plain), plain
    assert not any("MV4" in t for t in ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, 2, 0b01, fused=False, **hint))
    # the form exists at head dims 40 and 64 only
    assert not any("MV4" in t for t in ops.attn_frame_sets_edits_plan(K, sets, 320, H, 80, 2, 0b11, multi_v=True, multi_v64=True))


def test_planned_for_the_largest_set():
    """The kernel forms, the split and the fused decision are those of a bank of K' = max popcount frames."""
    S, H, Dh = 320, 2, 64
    for table in ("R1+a0", "scattered"):
        Kmax = K_MAX[table]
        for m in (0, 0b01, 0b11):
            got = ops.attn_frame_sets_edits_plan(K, TABLES[table], S, H, Dh, 2, m, fused=False, multi_v=False)
            assert [t.replace(",set", "") for t in got] == \
                ops.attn_edits_plan(Kmax, Kmax, S, H, Dh, False, 2, inject_mask=m, fused=False, multi_v=False), (table, m, got)


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("S,H,Dh,kw", [(48, 2, 40, {}), (320, 2, 64, {"fused": False}), (576, 2, 64, {"fused": False, "no_split": True}),
                                      (1024, 8, 40, {}), (128, 2, 160, {"out_dtype": torch.float32})])
def test_one_edit_is_the_frame_set_call(table, S, H, Dh, kw):
    for inject in (False, True):
        for mv in ({}, {"multi_v": True}, {"multi_v": False}, {"multi_v64": True}):      # the hints have nothing to select
            assert ops.attn_frame_sets_edits_plan(K, TABLES[table], S, H, Dh, 1, int(inject), **kw, **mv) == \
                ops.attn_frame_sets_plan(K, TABLES[table], S, H, Dh, inject, **kw)


@pytest.mark.parametrize("Kb,S,H,Dh,kw", [(6, 48, 2, 40, {}), (6, 320, 2, 64, {"fused": False}), (8, 4096, 8, 40, {}),
                                         (25, 4096, 5, 64, {}), (6, 512, 2, 40, {"fused": False, "no_split": True}),
                                         (6, 320, 2, 64, {"fused": False, "multi_v64": True}), (6, 192, 2, 160, {})])
def test_contiguous_sets_are_the_windowed_multi_edit_call(Kb, S, H, Dh, kw):
    """Token for token, ',win' and no ',set', the measured windowed default of the four-bank form included ((8, 4096, 8, 40) and
    (25, 4096, 5, 64) at radius 2); and so full sets are the masked multi-edit call."""
    tables = [ops.bank_windows(Kb, 1), ops.bank_windows(Kb, 2)] + ([IRREGULAR] if Kb == 6 else [])
    for E, m in ((2, 0), (2, 0b11), (3, 0b101), (3, 0b010)):
        for windows in tables:
            plan = ops.attn_frame_sets_edits_plan(Kb, as_masks(windows), S, H, Dh, E, m, **kw)
            assert plan == ops.attn_windows_edits_plan(Kb, windows, S, H, Dh, E, m, **kw)
            assert any(",win" in t for t in plan) and not any(",set" in t for t in plan), plan
        full = ops.attn_frame_sets_edits_plan(Kb, [mask(*range(Kb))] * Kb, S, H, Dh, E, m, **kw)
        assert full == ops.attn_edits_plan(Kb, Kb, S, H, Dh, False, E, inject_mask=m, **kw)
        assert full == ops.attn_frame_sets_edits_plan(Kb, ops.bank_frame_sets(Kb, Kb + 3, [0]), S, H, Dh, E, m, **kw)
    assert any("MV4" in t for t in ops.attn_frame_sets_edits_plan(8, as_masks(ops.bank_windows(8, 2)), 4096, 8, 40, 2, 0b11))


# mv4_set_default, as profiles/r21_frame_sets_edits_ab.txt has it: (K, S, H, Dh, radius, anchors) -> the form is the default
MV4_SET_DEFAULT = [
    # the measured cells (radius 2 with anchor 0, a largest set of 6 frames: the form ahead in all of them) and the box they span
    (25, 4096, 5, 64, 2, [0], 1), (10, 9216, 5, 64, 2, [0], 1), (8, 4096, 8, 40, 2, [0], 1), (16, 4096, 5, 64, 2, [0], 1),
    (25, 4096, 5, 64, 2, [12], 1),
    # not measured: other radii and anchor counts (largest sets of 4, 8 and 7 frames), other frame sizes, head counts, banks
    (25, 4096, 5, 64, 1, [0], 0), (25, 4096, 5, 64, 3, [0], 0), (25, 4096, 5, 64, 2, [0, 24], 0), (8, 4096, 8, 40, 1, [0], 0),
    (8, 1024, 8, 40, 2, [0], 0), (25, 1024, 10, 64, 2, [0], 0), (6, 4096, 8, 40, 2, [0], 0), (30, 4096, 5, 64, 2, [0], 0),
]


def test_default_of_the_four_bank_form_in_a_frame_set_call():
    """Without a hint a frame-set call takes the four-bank form exactly where the record shows it ahead of the DUAL composition by
    more than both spreads.  The whole-bank and the windowed defaults say nothing about sets; the hints override both ways."""
    mv = lambda plan: sum("MV4" in t and t.endswith(",set") for t in plan)      # noqa: E731
    for Kb, S, H, Dh, R, anchors, want in MV4_SET_DEFAULT:
        sets = ops.bank_frame_sets(Kb, R, anchors)
        hint = {"multi_v": True} if Dh == 40 else {"multi_v64": True}
        for E, m in ((2, 0b11), (3, 0b111), (3, 0b101)):
            assert mv(ops.attn_frame_sets_edits_plan(Kb, sets, S, H, Dh, E, m)) == want, (Kb, S, H, Dh, R, anchors)
            assert mv(ops.attn_frame_sets_edits_plan(Kb, sets, S, H, Dh, E, m, **hint)) == 1
            assert mv(ops.attn_frame_sets_edits_plan(Kb, sets, S, H, Dh, E, m, multi_v=False)) == 0
        assert mv(ops.attn_frame_sets_edits_plan(Kb, sets, S, H, Dh, 2, 0b01)) == 0      # one injecting edit: no pair


def _raw(sets, Kb=4, Kq=4, q_frame0=0, E=2, m=0, flags=0, S=64, H=2, Dh=40):
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = None if sets is None else ctypes.cast((ctypes.c_uint64 * len(sets))(*sets), ctypes.c_void_p)
    return lib.tf_ext_attn_frame_sets_edits_plan(Kb, Kq, q_frame0, S, H, Dh, E, m, flags, _lib.TF_BF16, a, buf, len(buf))


def _last_error():
    return _lib.load().tf_last_error().decode()


def test_refusals():
    TF_ERR_SHAPE, TF_ERR_NULL = -3, -1
    NAME = "tf_ext_attn_fwd_frame_sets_edits"
    good = [mask(0, 1), mask(1, 3), mask(0, 2), mask(0, 3)]
    assert _raw(good) > 0
    # the table: what the frame-set call refuses
    assert _raw(None) == TF_ERR_NULL and NAME in _last_error()
    assert _raw(good, Kb=65) == TF_ERR_SHAPE and "at most 64 bank frames" in _last_error() and NAME in _last_error()
    assert _raw([mask(i, 63 - i) for i in range(64)], Kb=64, Kq=64, S=32) > 0
    assert _lib.TF_MAX_WINDOW_FRAMES == 64      # Kq > TF_MAX_WINDOW_FRAMES cannot be reached with K <= 64: the bank check answers
    for sets, what in (([mask(0, 1), 0, mask(0, 2), mask(0, 3)], "is empty"),
                       ([mask(0, 1), mask(1, 4), mask(0, 2), mask(0, 3)], "at or above"),
                       ([mask(0, 1), mask(0, 3), mask(0, 2), mask(0, 3)], "own frame")):
        assert _raw(sets) == TF_ERR_SHAPE, sets
        assert what in _last_error() and NAME in _last_error(), _last_error()
    assert _raw([mask(0, 3), mask(1, 4)], Kb=6, Kq=2, q_frame0=3) > 0
    assert _raw([mask(0, 2), mask(1, 4)], Kb=6, Kq=2, q_frame0=3) == TF_ERR_SHAPE
    # the flags without a frame-set form, on set tables, on ranges and on full sets; then what the masked call refuses
    tables = (good, as_masks(ops.bank_windows(4, 1)), [15] * 4)
    for bits in (_lib.TF_ATTN_FOLD_SCALE, _lib.TF_ATTN_BANK_ONLY, _lib.TF_ATTN_SOURCE_ONLY, _lib.TF_ATTN_RUN_MULTI_V):
        for sets in tables:
            assert _raw(sets, flags=bits) == TF_ERR_SHAPE and "no frame-set form" in _last_error() and NAME in _last_error()
    for sets in tables:
        for kw in ({"flags": _lib.TF_ATTN_INJECT}, {"flags": _lib.TF_ATTN_MULTI_V | _lib.TF_ATTN_NO_MULTI_V},
                   {"flags": _lib.TF_ATTN_MULTI_V64 | _lib.TF_ATTN_NO_MULTI_V}, {"m": 0b100}, {"E": 0}, {"E": _lib.TF_MAX_EDITS + 1},
                   {"E": 1, "m": 0b10}, {"E": 1, "flags": _lib.TF_ATTN_INJECT}):
            assert _raw(sets, **kw) == TF_ERR_SHAPE, (sets, kw)
            assert NAME in _last_error(), _last_error()
        for bits in (_lib.TF_ATTN_MULTI_V, _lib.TF_ATTN_NO_MULTI_V, _lib.TF_ATTN_MULTI_V64):      # accepted here ...
            assert _raw(sets, flags=bits) > 0 and _raw(sets, flags=bits, E=1) > 0, bits
    # ... while the single-edit frame-set call keeps refusing them
    for bits in (_lib.TF_ATTN_MULTI_V, _lib.TF_ATTN_NO_MULTI_V, _lib.TF_ATTN_MULTI_V64):
        with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_fwd_frame_sets:"):
            ops.attn_frame_sets_plan(4, good, 64, 2, 40, True, hints=bits)
    # the Python layer
    plan = lambda **kw: ops.attn_frame_sets_edits_plan(4, kw.pop("sets", good), 64, 2, 40, kw.pop("E", 2), kw.pop("m", 0), **kw)      # noqa: E731
    assert plan()
    for bad in (good[:-1], [3, 3, 3, 12], [3, 0, 4, 12], [3, 3, 4 | 16, 12]):
        with pytest.raises(ValueError):
            plan(sets=bad)
    for E_bad, m in ((2, 0b100), (2, -1), (0, 0), (_lib.TF_MAX_EDITS + 1, 0)):
        with pytest.raises(ValueError):
            plan(E=E_bad, m=m)
    with pytest.raises(_lib.TokenflowHipError, match=NAME):
        plan(hints=_lib.TF_ATTN_FOLD_SCALE)
    with pytest.raises(_lib.TokenflowHipError, match="exclude each other"):
        plan(multi_v=False, multi_v64=True)


@pytest.mark.parametrize("S,H,Dh", [(64, 2, 40), (256, 8, 40), (1024, 8, 40), (576, 5, 64), (320, 2, 80), (128, 2, 160), (4096, 5, 64)])
def test_partial_results_of_every_set_size_fit_the_banks_workspace(S, H, Dh):
    """The split is planned for the largest set K' < K while the partial results live in the workspace of the K-frame bank: the
    call checks the fit (TF_ERR_WORKSPACE, -5).  The sweep of tests/test_windows_plan_cpu.py over dilated sets: no bank of up to 64
    keyframes and no set size refuses, for a mixed mask (a DUAL and an ALL bank launch)."""
    for Kb in range(3, 65):
        for n in range(1, Kb // 2 + 1):
            sets = []
            for i in range(Kb):
                same = list(range(i % 2, Kb, 2))                      # the frames of i's parity; n of them around i
                j = max(0, min(i // 2 - n // 2, len(same) - n))
                sets.append(mask(*same[j:j + n]))
            rc = _raw(sets, Kb=Kb, Kq=Kb, E=2, m=0b01, flags=_lib.TF_ATTN_NO_FUSED, S=S, H=H, Dh=Dh)
            assert rc > 0, (Kb, n, rc, _last_error())
