"""Launch plans of the attention and NN-search dispatchers, without a GPU (tf_ext_attn_plan / tf_nn_search_plan record
the launches of the real dispatch code instead of issuing them).

  * the forms the default build can reach over a wide sweep equal the committed set (tests/golden/kernel_plans.json);
  * every reachable form has a GPU case in tests/kernel_forms.py, and every case's plan contains its form;
  * no call without TF_ATTN_HINT_MIX changed plan against the committed digests (bench.py's cfg2 calls in full);
  * properties of the planner the header promises (the mixed-shape hint, the bit-stable mode, the part composition).

`python -m tests.test_kernel_plan_cpu --write` regenerates the golden file (after a deliberate change of the dispatch).
"""
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import kernel_forms as kf  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_plans.json")
# read once per process by the library: a set one changes the plans the sweep describes
PLANNER_ENV = ("TOKENFLOW_ATTN_NSEG", "TOKENFLOW_SPLIT_OVER", "TOKENFLOW_FUSED_MAX_S")


def _ops():
    bad = [e for e in os.environ if e.startswith("TF_NN_") or e in PLANNER_ENV]
    if bad:
        pytest.skip(f"planner overrides set in the environment ({', '.join(sorted(bad))}): the sweep describes the defaults")
    from tokenflow_amd import ops
    return ops


def _digests(ops):
    """Per (head dim, S) group of the unhinted attention sweep and per D of the NN sweep: a digest of every call's plan."""
    groups = {}
    for key, kw in list(kf.sweep_attn(False)) + list(kf.sweep_nn()):
        g = f"attn d{kw['dh']} S{kw['S']}" if "dh" in kw else f"nn D{kw['D']}"
        groups.setdefault(g, hashlib.sha256()).update(f"{key} -> {';'.join(kf.plan(ops, kw))}\n".encode())
    return {g: h.hexdigest()[:16] for g, h in sorted(groups.items())}


def _reachable(ops):
    toks = set()
    for _, kw in list(kf.sweep_attn(False)) + list(kf.sweep_attn(True)) + list(kf.sweep_nn()):
        toks.update(kf.plan(ops, kw))
    return sorted(toks)


def _table(ops):
    return {"reachable": _reachable(ops), "unhinted_digests": _digests(ops),
            "bench_cfg2": {key: kf.plan(ops, kw) for key, kw in kf.bench_calls()}}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def reachable():
    return _reachable(_ops())


def test_reachable_tokens_equal_the_committed_set(golden, reachable):
    new, gone = sorted(set(reachable) - set(golden["reachable"])), sorted(set(golden["reachable"]) - set(reachable))
    assert not new and not gone, f"kernel forms appeared: {new}; vanished: {gone}"


def test_every_reachable_form_has_a_gpu_case(reachable):
    forms = {kf.form(t) for t in reachable}
    uncovered = sorted(forms - set(kf.CASES))
    assert not uncovered, f"no case in tests/kernel_forms.py runs {uncovered}"
    stale = sorted(set(kf.CASES) - forms)
    assert not stale, f"tests/kernel_forms.py lists forms the sweep cannot reach: {stale}"


def test_every_case_plans_its_form():
    ops = _ops()
    for f, cases in kf.CASES.items():
        assert cases, f"{f}: no case"
        for c in cases:
            got = kf.plan(ops, c)
            assert f in [kf.form(t) for t in got], f"{f}: case {c} plans {got}"


def test_unhinted_plans_unchanged(golden):
    ops = _ops()
    got = _digests(ops)
    changed = sorted(g for g in set(got) | set(golden["unhinted_digests"]) if got.get(g) != golden["unhinted_digests"].get(g))
    assert not changed, f"plans of calls without TF_ATTN_HINT_MIX changed in groups {changed}"
    for key, kw in kf.bench_calls():
        assert kf.plan(ops, kw) == golden["bench_cfg2"][key], key


def test_bench_cfg2_level0_takes_the_mixed_form(golden):
    """bench.py's level-0 call (K = 8, S = 4096, 8 heads of 40, no injection) is the mixed-shape kernel's default."""
    assert golden["bench_cfg2"]["attn K8 Kq8 S4096 H8 d40 inj0 all ns0 fusedNone fold0 o320 hints0"] == \
        ["vt_pack", "il<40,8,ALL,4,3>"]


@pytest.mark.parametrize("K,S,H", [(1, 256, 1), (2, 256, 2), (4, 320, 3), (2, 576, 2), (3, 1024, 1), (4, 1024, 8)])
@pytest.mark.parametrize("no_split", [False, True])
@pytest.mark.parametrize("inject", [False, True])
def test_hint_mix_takes_the_mixed_form_at_tile_multiples(K, S, H, no_split, inject):
    """TF_ATTN_HINT_MIX at S % 64 == 0, S >= 256: the mixed-shape form (DMA 3) for the ALL launch, or for the SOURCE launch
    beside the dual-V kernel under injection, one-pass and split, whatever the grid."""
    ops = _ops()
    p = ops.attn_plan(K, K, S, H, 40, inject, no_split=no_split, fused=False, hints=kf.HINT_MIX)
    want = "il<40,8,SOURCE,4,3>" if inject else "il<40,8,ALL,4,3>"
    assert want in p, p
    assert all(t.startswith(("vt_pack", "merge", "il<40,8,DUAL,4,2>", want)) for t in p), p
    src = ops.attn_plan(K, K, S, H, 40, inject, part="source", no_split=no_split, fused=False, hints=kf.HINT_MIX)
    assert src == ["vt_pack", "il<40,8,SOURCE,4,3>"], src


@pytest.mark.parametrize("S", [200, 723, 1000])
def test_hint_mix_is_a_no_op_on_ragged_frames(S):
    ops = _ops()
    for inject in (False, True):
        for no_split in (False, True):
            a = ops.attn_plan(4, 4, S, 8, 40, inject, no_split=no_split, fused=False)
            assert ops.attn_plan(4, 4, S, 8, 40, inject, no_split=no_split, fused=False, hints=kf.HINT_MIX) == a


def test_bit_stable_mode_never_takes_the_mixed_form():
    """TF_ATTN_NO_SPLIT without the hint: the kernel choice is a function of the shape alone, never DMA form 3."""
    ops = _ops()
    for _, kw in kf.sweep_attn(False):
        if kw["no_split"]:
            p = kf.plan(ops, kw)
            assert not any(t.startswith("il<") and t.endswith(",3>") for t in p), (kw, p)


def test_part_composition():
    """A bank-only call launches no SOURCE kernel; a source-only call launches nothing but the pre-pass and SOURCE
    kernels (or the fused kernel); a full injected streaming call is DUAL (+ merge) then SOURCE, or ALL."""
    ops = _ops()
    for _, kw in kf.sweep_attn(False):
        p = [t for t in kf.plan(ops, kw) if t != "vt_pack"]
        if kw["part"] == "bank":
            assert not any(",SOURCE," in t for t in p), (kw, p)
        elif kw["part"] == "source":
            assert not any(t.startswith("merge") or ",ALL," in t or ",DUAL," in t for t in p), (kw, p)
            assert all(",SOURCE," in t or t.startswith("fused[") for t in p), (kw, p)
        elif any(",DUAL," in t for t in p):
            assert kw["inject"] and ",SOURCE," in p[-1], (kw, p)


def test_plan_query_rejects_bad_arguments():
    ops = _ops()
    from tokenflow_amd._lib import TokenflowHipError
    with pytest.raises(TokenflowHipError, match="head dim"):
        ops.attn_plan(2, 2, 256, 2, 48, False)
    with pytest.raises(TokenflowHipError, match="tf_ext_attn_plan"):
        ops.attn_plan(2, 3, 256, 2, 40, False)
    with pytest.raises(TokenflowHipError, match="tf_nn_search_plan"):
        ops.nn_plan(256, 256, 36, 1)


if __name__ == "__main__" and "--write" in sys.argv:
    from tokenflow_amd import ops as _o
    with open(GOLDEN, "w") as f:
        json.dump(_table(_o), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
