"""Launch plans of the run form of the extended attention (tf_ext_attn_run_plan), without a GPU.

  * every form a wide sweep of run calls reaches has a GPU case in tests/attn_run_forms.py, and every case plans its form;
  * a run call never takes the fused small-problem kernel, a bank-only run launches no SOURCE kernel, exactly the launches
    that leave partial results are marked, the plan ends with the merge over the runs;
  * the plan is a function of the arguments;
  * the flag combinations the header refuses raise, with the function's name in the message.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import attn_run_forms as rf  # noqa: E402

# read once per process by the library: a set one changes the plans the sweep describes (the documented planner overrides)
PLANNER_ENV = ("TOKENFLOW_ATTN_NSEG", "TOKENFLOW_SPLIT_OVER", "TOKENFLOW_FUSED_MAX_S")


def _ops():
    from tokenflow_amd import ops
    return ops


@pytest.fixture(scope="module")
def swept():
    ops = _ops()
    return [(key, kw, rf.plan(ops, kw)) for key, kw in rf.sweep()]


def test_every_reachable_run_form_has_a_gpu_case(swept):
    forms = {rf.form(t) for _, _, p in swept for t in p}
    uncovered = sorted(forms - set(rf.CASES))
    assert not uncovered, f"no case in tests/attn_run_forms.py runs {uncovered}"
    stale = sorted(set(rf.CASES) - forms)
    assert not stale, f"tests/attn_run_forms.py lists forms the sweep cannot reach: {stale}"


def test_every_case_plans_its_form():
    ops = _ops()
    for f, cases in rf.CASES.items():
        assert cases, f"{f}: no case"
        for c in cases:
            runs = c["runs"]
            assert sorted(x for f0, n in runs for x in range(f0, f0 + n)) == list(range(c["K"])), c
            assert runs[0][0] <= c["q_frame0"] and c["q_frame0"] + c["Kq"] <= runs[0][0] + runs[0][1], c
            got = rf.case_plans(ops, c)
            assert f in [rf.form(t) for p in got for t in p], f"{f}: case {c} plans {got}"


def test_every_streaming_family_has_a_run_form(swept):
    """The interleaved, one-tile and ping-pong kernels, ALL and DUAL, at every head dim they serve."""
    toks = {t for _, _, p in swept for t in p}
    for want in ("il<40,", "il<64,", "il<80,", "one<40,", "one<64,", "one<80,", "one<160,", "pp<64,"):
        assert any(t.startswith(want) and t.endswith(",run>") for t in toks), want
    for dh in (40, 64, 80):
        assert any(f",DUAL," in t and t.endswith(",run>") and f"<{dh}," in t for t in toks), dh


def test_run_plan_shape(swept):
    for key, kw, p in swept:
        assert p[0] == "vt_pack" and p[-1] == f"merge[runs={kw['n_runs']}]", (key, p)
        body = p[1:-1]
        assert body, (key, p)
        assert not any(t.startswith("fused[") for t in p), (key, p)          # no partial output in the fused kernel
        assert not any(t.startswith("merge[nseg") for t in p), (key, p)      # a run's partials wait for the merge over runs
        for t in body:
            # partial results <=> a bank launch; the source branch is final
            assert t.endswith(",run>") == (",SOURCE," not in t), (key, p)
        bank = [t for t in body if t.endswith(",run>")]
        assert len(bank) == 1 and body[0] == bank[0], (key, p)
        if kw["bank_only"]:
            assert len(body) == 1 and ",SOURCE," not in body[0], (key, p)
        else:
            # the source branch: inside the ALL launch, or a SOURCE launch behind the dual-V / ping-pong bank launch
            assert len(body) == 1 and ",ALL," in body[0] or (len(body) == 2 and ",SOURCE," in body[1]), (key, p)
        if not kw["hints"]:
            assert not any(t.startswith("il<") and ",3" in t.split(",", 4)[-1] for t in p), (key, p)   # mixed form: on the hint only


def test_source_launch_of_a_run_is_the_source_only_call_s(swept):
    """What computes the source branch in a run call is the kernel of ops.ext_attn(part='source', no_split=True,
    fused=False) on the same frames: SOURCE launches token for token, ALL launches as the same kernel in its ALL mode."""
    ops = _ops()
    import torch
    seen = set()
    for key, kw, p in swept:
        if kw["bank_only"]:
            continue
        sig = (kw["Kq"], kw["S"], kw["heads"], kw["dh"], kw["inject"], kw["fold_scale"], kw["hints"])
        if sig in seen:
            continue
        seen.add(sig)
        ref = ops.attn_plan(kw["Kq"], kw["Kq"], kw["S"], kw["heads"], kw["dh"], kw["inject"], part="source", no_split=True,
                            fused=False, fold_scale=kw["fold_scale"], hints=kw["hints"], dtype=torch.bfloat16)
        assert len(ref) == 2, ref
        body = p[1:-1]
        got = body[1] if len(body) == 2 else body[0].replace(",ALL,", ",SOURCE,").replace(",run>", ">")
        assert got == ref[1], (key, p, ref)


def test_plan_is_a_function_of_the_arguments():
    """Twice the same answer in one process, and the same in a fresh process whose environment sets every switch that is
    NOT a documented planner override."""
    ops = _ops()
    if any(e in os.environ for e in PLANNER_ENV):
        pytest.skip("planner overrides set in the environment")
    probe = [kw for i, (_, kw) in enumerate(rf.sweep()) if i % 97 == 0]
    here = [rf.plan(ops, kw) for kw in probe]
    assert here == [rf.plan(ops, kw) for kw in probe]
    code = ("import sys, json; sys.path.insert(0, %r)\n"
            "from tokenflow_amd import ops\nfrom tests import attn_run_forms as rf\n"
            "print(json.dumps([rf.plan(ops, kw) for i, (_, kw) in enumerate(rf.sweep()) if i %% 97 == 0]))\n" % ROOT)
    env = dict(os.environ, TOKENFLOW_ATTN_NO_SPLIT="1", TOKENFLOW_FOLD_SCALE="0", TOKENFLOW_SHARD_BANK_RUNS="1",
               TOKENFLOW_FP32_AS="f16")
    import json
    out = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout
    assert json.loads(out.strip().splitlines()[-1]) == here


def test_run_plan_rejects_bad_arguments():
    ops = _ops()
    from tokenflow_amd import _lib
    from tokenflow_amd._lib import TokenflowHipError
    for bad in (_lib.TF_ATTN_SOURCE_ONLY, _lib.TF_ATTN_FUSED, _lib.attn_hint(qw=2), _lib.attn_hint(kw=4),
                _lib.TF_ATTN_HINT_QB2, _lib.TF_ATTN_PRECISE_P, _lib.TF_ATTN_NO_PRECISE_P):
        with pytest.raises(TokenflowHipError, match="tf_ext_attn_run"):
            ops.attn_run_plan(5, 2, 2, 3, 256, 2, 40, False, hints=bad)
    with pytest.raises(TokenflowHipError, match="tf_ext_attn_run.*source branch"):
        ops.attn_run_plan(5, 2, 1, 3, 256, 2, 40, False)               # query frames do not fit the run
    assert ops.attn_run_plan(5, 2, 1, 3, 256, 2, 40, False, bank_only=True)
    with pytest.raises(TokenflowHipError, match="tf_ext_attn_run_plan.*head dim"):
        ops.attn_run_plan(5, 2, 2, 3, 256, 2, 48, False)
    with pytest.raises(TokenflowHipError, match="tf_ext_attn_run_plan"):
        ops.attn_run_plan(2, 3, 2, 1, 256, 2, 40, False)               # Kq > K
    with pytest.raises(TokenflowHipError, match="tf_ext_attn_run_plan.*runs"):
        ops.attn_run_plan(2, 1, 1, 3, 256, 2, 40, False)               # more runs than frames
    with pytest.raises(TokenflowHipError, match="tf_ext_attn_run: run of frames"):
        ops.attn_run_plan(5, 2, 6, 3, 256, 2, 40, False)               # run longer than the bank
    with pytest.raises(TokenflowHipError, match="tf_ext_attn_run: run of frames"):
        ops.attn_run_plan(5, 2, 0, 3, 256, 2, 40, False, bank_only=True)


def test_existing_plans_do_not_know_the_run_mark():
    """tf_ext_attn_plan emits the tokens it always did: the run mark appears in run plans only."""
    from tests import kernel_forms as kf
    ops = _ops()
    for _, kw in kf.bench_calls():
        assert not any("run" in t for t in kf.plan(ops, kw))
