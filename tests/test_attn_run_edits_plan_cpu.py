"""Launch plans and refusals of the run form of the multi-edit attention (tf_ext_attn_run_edits_plan), without a GPU.

  * the plan of a run call is ONE vt_pack, then each edit's own bank-only run tokens (injecting edits first, then the
    others, ascending), then the source token where the run holds the query frames, then merge[runs=N,edits=E];
  * one edit records exactly tf_ext_attn_run_plan;
  * every refusal of the header returns TF_ERR_SHAPE with the function's name in tf_last_error and launches nothing (the
    calls are made under no device: placeholders that a launch would fault on);
  * the workspace size is 0 for bad arguments and, for one edit, the single-edit run set's.
"""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import attn_run_edit_forms as ef  # noqa: E402
from tests import attn_run_forms as rf  # noqa: E402


def _ops():
    from tokenflow_amd import ops
    return ops


def _edits_of(mask, E):
    inj = [e for e in range(E) if (mask >> e) & 1]
    return inj + [e for e in range(E) if not (mask >> e) & 1]


@pytest.mark.parametrize("S,H,dh", ef.SHAPES, ids=lambda x: str(x))
@pytest.mark.parametrize("E,mask", [(2, 0b00), (2, 0b11), (2, 0b01), (2, 0b10), (3, 0), (3, 0b111), (3, 0b101), (3, 0b010)])
def test_run_edits_plan_is_the_composition_of_the_edits_own_run_plans(S, H, dh, E, mask):
    ops = _ops()
    K, Kq, runs = rf.BASE["K"], rf.BASE["Kq"], rf.BASE["runs"]
    for r, (f0, n) in enumerate(runs):
        bank_only = r != 0
        got = ops.attn_run_edits_plan(K, Kq, n, len(runs), S, H, dh, E, mask, bank_only=bank_only)
        want = ["vt_pack"]
        for e in _edits_of(mask, E):
            own = ops.attn_run_plan(K, Kq, n, len(runs), S, H, dh, bool((mask >> e) & 1), bank_only=True)
            assert own[0] == "vt_pack" and own[-1] == f"merge[runs={len(runs)}]", own
            assert all(t.endswith(",run>") for t in own[1:-1]), own
            want += own[1:-1]
        if not bank_only:
            # what computes the source branch of the query frames in a run call: the kernel of the source-only call
            src = ops.attn_plan(Kq, Kq, S, H, dh, mask == (1 << E) - 1, part="source", no_split=True, fused=False)
            assert len(src) == 2 and ",SOURCE," in src[1], src
            want.append(src[1])
        want.append(f"merge[runs={len(runs)},edits={E}]")
        assert got == want, (S, H, dh, E, mask, r, got, want)
        assert got.count("vt_pack") == 1 and not any(t.startswith(("fused[", "merge[nseg")) or ",MV4," in t for t in got), got


@pytest.mark.parametrize("S,H,dh", ef.SHAPES, ids=lambda x: str(x))
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("bank_only", [False, True])
def test_one_edit_records_the_single_edit_run_plan(S, H, dh, inject, bank_only):
    ops = _ops()
    K, Kq, n_runs = rf.BASE["K"], rf.BASE["Kq"], 3
    for n in (1, 2) if bank_only else (2,):
        assert ops.attn_run_edits_plan(K, Kq, n, n_runs, S, H, dh, 1, int(inject), bank_only=bank_only) == \
            ops.attn_run_plan(K, Kq, n, n_runs, S, H, dh, inject, bank_only=bank_only)


def test_cases_plan_a_dual_and_an_all_run_launch_at_each_head_dim_and_the_edits_merge():
    """The coverage of the GPU cases (tests/test_attn_runs_edits_gpu.py runs exactly ef.CASES)."""
    ops = _ops()
    toks = {t for c in ef.CASES for p in ef.case_plans(ops, c) for t in p}
    for dh in (40, 64, 80):
        assert any(f"<{dh}," in t and ",DUAL," in t and t.endswith(",run>") for t in toks), (dh, sorted(toks))
    for dh in (40, 64, 80, 160):
        assert any(f"<{dh}," in t and ",ALL," in t and t.endswith(",run>") for t in toks), (dh, sorted(toks))
    assert "merge[runs=3,edits=2]" in toks and "merge[runs=3,edits=3]" in toks
    assert any(t.startswith("il<") for t in toks) and any(t.startswith("one<") for t in toks) and "pp<64,ALL,run>" in toks


def test_refusals_return_shape_error_name_the_function_and_launch_nothing():
    from tokenflow_amd import _lib
    lib = _lib.load()
    K, Kq, q0, S, H, Dh, n_runs, E = 5, 2, 2, 256, 2, 40, 3, 2
    D = H * Dh
    dt = _lib.TF_BF16
    fs = S * D
    strides = (ctypes.c_int64 * 9)(Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, D)
    nbytes = lib.tf_ext_attn_runs_edits_workspace_bytes(K, Kq, S, H, Dh, n_runs, E, dt)
    assert nbytes > 0
    ph = 1 << 12   # placeholder pointers: aligned, never dereferenced by a refused call (a launch on them would fault)

    def run(f0=2, n=2, r=0, nr=n_runs, Kq_=Kq, q0_=q0, Dh_=Dh, flags=0, E_=E, mask=0b01, compact=0, dtype=dt):
        return lib.tf_ext_attn_run_edits(ph, ph, ph, ph, K, Kq_, q0_, f0, n, r, nr, S, H, Dh_, D,
                                         ctypes.cast(strides, ctypes.c_void_p), 1.0, flags, dtype, E_, mask, compact, ph,
                                         nbytes, None)

    def merge(nr=n_runs, Dh_=Dh, flags=0, E_=E, mask=0b01, o_fs=fs):
        return lib.tf_ext_attn_runs_merge_edits(ph, K, Kq, S, H, Dh_, nr, E_, mask, Kq * fs, o_fs, flags, dt, ph, nbytes, None)

    L = _lib
    bad_run = [
        # everything tf_ext_attn_run refuses
        lambda: run(Dh_=48), lambda: run(n=0), lambda: run(f0=4, n=2), lambda: run(f0=-1, n=2, flags=L.TF_ATTN_BANK_ONLY),
        lambda: run(r=3), lambda: run(r=-1), lambda: run(nr=0), lambda: run(nr=K + 1),
        lambda: run(f0=0, n=2), lambda: run(f0=2, n=1), lambda: run(Kq_=6), lambda: run(q0_=4),
        lambda: run(flags=L.TF_ATTN_SOURCE_ONLY), lambda: run(flags=L.TF_ATTN_FUSED), lambda: run(flags=L.attn_hint(qw=2)),
        lambda: run(flags=L.attn_hint(kw=4)), lambda: run(flags=L.TF_ATTN_HINT_QB2), lambda: run(flags=L.TF_ATTN_PRECISE_P),
        lambda: run(flags=L.TF_ATTN_NO_PRECISE_P),
        # the multi-edit call's own
        lambda: run(flags=L.TF_ATTN_INJECT), lambda: run(mask=0b100), lambda: run(E_=1, mask=0b10),
        lambda: run(E_=0, mask=0), lambda: run(E_=L.TF_MAX_EDITS + 1), lambda: run(flags=L.TF_ATTN_MULTI_V),
        lambda: run(flags=L.TF_ATTN_MULTI_V | L.TF_ATTN_NO_MULTI_V), lambda: run(compact=4), lambda: run(compact=-1),
        # ... and with one edit, which delegates
        lambda: run(E_=1, mask=1, flags=L.TF_ATTN_INJECT), lambda: run(E_=1, mask=0, flags=L.TF_ATTN_MULTI_V),
        lambda: run(E_=1, mask=0, f0=0, n=2), lambda: run(E_=1, mask=0, flags=L.TF_ATTN_SOURCE_ONLY),
    ]
    for i, call in enumerate(bad_run):
        rc = call()
        msg = lib.tf_last_error().decode()
        assert rc == -3, (i, rc, msg)
        assert "tf_ext_attn_run_edits" in msg, (i, msg)
    bad_merge = [lambda: merge(Dh_=48), lambda: merge(nr=0), lambda: merge(o_fs=fs + 4), lambda: merge(flags=L.TF_ATTN_INJECT),
                 lambda: merge(mask=0b100), lambda: merge(E_=0, mask=0), lambda: merge(E_=L.TF_MAX_EDITS + 1),
                 lambda: merge(flags=L.TF_ATTN_MULTI_V)]
    for i, call in enumerate(bad_merge):
        rc = call()
        msg = lib.tf_last_error().decode()
        assert rc == -3, (i, rc, msg)
        assert "tf_ext_attn_runs_merge_edits" in msg, (i, msg)
    # other error classes keep their codes
    assert run(dtype=L.TF_F32) == -2 and "tf_ext_attn_run_edits" in lib.tf_last_error().decode()
    assert lib.tf_ext_attn_run_edits(0, ph, ph, ph, K, Kq, q0, 2, 2, 0, n_runs, S, H, Dh, D, ctypes.cast(strides, ctypes.c_void_p),
                                     1.0, 0, dt, E, 1, 0, ph, nbytes, None) == -1
    assert lib.tf_ext_attn_run_edits(ph, ph, ph, ph, K, Kq, q0, 2, 2, 0, n_runs, S, H, Dh, D, ctypes.cast(strides, ctypes.c_void_p),
                                     1.0, 0, dt, E, 1, 0, ph, nbytes - 1, None) == -5
    assert lib.tf_ext_attn_run_edits(ph + 2, ph, ph, ph, K, Kq, q0, 2, 2, 0, n_runs, S, H, Dh, D,
                                     ctypes.cast(strides, ctypes.c_void_p), 1.0, 0, dt, E, 1, 0, ph, nbytes, None) == -4


def test_plan_refusals_raise_with_the_functions_name():
    ops = _ops()
    from tokenflow_amd import _lib
    from tokenflow_amd._lib import TokenflowHipError
    for bad in (_lib.TF_ATTN_SOURCE_ONLY, _lib.TF_ATTN_FUSED, _lib.attn_hint(qw=2), _lib.TF_ATTN_PRECISE_P):
        with pytest.raises(TokenflowHipError, match="tf_ext_attn_run_edits"):
            ops.attn_run_edits_plan(5, 2, 2, 3, 256, 2, 40, 2, 0b01, hints=bad)
    for bad in (_lib.TF_ATTN_INJECT, _lib.TF_ATTN_MULTI_V):
        with pytest.raises(TokenflowHipError, match="tf_ext_attn_run_edits_plan"):
            ops.attn_run_edits_plan(5, 2, 2, 3, 256, 2, 40, 2, 0b01, hints=bad)
    assert ops.attn_run_edits_plan(5, 2, 2, 3, 256, 2, 40, 2, 0b11, hints=_lib.TF_ATTN_NO_MULTI_V) == \
        ops.attn_run_edits_plan(5, 2, 2, 3, 256, 2, 40, 2, 0b11)            # accepted and ignored
    with pytest.raises(TokenflowHipError, match="tf_ext_attn_run_edits.*source branch"):
        ops.attn_run_edits_plan(5, 2, 1, 3, 256, 2, 40, 2, 0b01)             # query frames do not fit the run
    with pytest.raises(TokenflowHipError, match="tf_ext_attn_run_edits_plan.*head dim"):
        ops.attn_run_edits_plan(5, 2, 2, 3, 256, 2, 48, 2, 0)
    with pytest.raises(ValueError, match="attn_run_edits_plan"):
        ops.attn_run_edits_plan(5, 2, 2, 3, 256, 2, 40, 2, 0b100)
    with pytest.raises(ValueError, match="attn_run_edits_plan"):
        ops.attn_run_edits_plan(5, 2, 2, 3, 256, 2, 40, 9, 0)


def test_workspace_size():
    from tokenflow_amd import _lib
    lib = _lib.load()
    size = lib.tf_ext_attn_runs_edits_workspace_bytes
    dt = _lib.TF_BF16
    good = (5, 2, 256, 2, 40, 3)
    for bad in [(0, 2, 256, 2, 40, 3), (5, 0, 256, 2, 40, 3), (5, 6, 256, 2, 40, 3), (5, 2, 0, 2, 40, 3), (5, 2, 256, 0, 40, 3),
                (5, 2, 256, 2, 48, 3), (5, 2, 256, 2, 40, 0), (5, 2, 256, 2, 40, 6)]:
        assert size(*bad, 2, dt) == 0, bad
    assert size(*good, 0, dt) == 0 and size(*good, _lib.TF_MAX_EDITS + 1, dt) == 0 and size(*good, 2, _lib.TF_F32) == 0
    for S, H, dh in ef.SHAPES:
        one = lib.tf_ext_attn_runs_workspace_bytes(5, 2, S, H, dh, 3, dt)
        assert one > 0 and size(5, 2, S, H, dh, 3, 1, dt) >= one
        assert size(5, 2, S, H, dh, 3, 3, dt) > size(5, 2, S, H, dh, 3, 2, dt) > size(5, 2, S, H, dh, 3, 1, dt)


def test_existing_run_plans_do_not_know_the_edits_merge():
    ops = _ops()
    for i, (_, kw) in enumerate(rf.sweep()):
        if i % 53 == 0:
            assert not any("edits=" in t for t in rf.plan(ops, kw))
