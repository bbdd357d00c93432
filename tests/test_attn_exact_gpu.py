"""Exact-arithmetic attention tests: count every key, find every key (tests/attn_exact.py builds the inputs and the fp64
reference; tests/test_attn_exact_cpu.py shows on mutated references that these assertions fail on a subtly wrong kernel).

Every call of `attn_exact.GPU_CASES` -- every attention form of tests/kernel_forms.CASES, the frame-set, windowed, multi-edit
(with the four-bank shared-softmax form), run and segment calls -- has its launch plan asserted (16-bit and fp32 output) and
then runs, in bf16 and f16:

  * census zero and census flat negative: the output is the count c / N of the key list, known in closed form.
    fp32 output, zero: |out - c/N| <= 2^-20 c/N and exactly 0 where c = 0 -- everything before the normalisation is exact
    integer arithmetic; the normalisation is at most a reciprocal and a multiply, once more in a split or run merge: 4
    roundings of 2^-23 at most, doubled.  The smallest single-key signal, 1 / (N + 1) >= 2^-12.01, is 250 times that.
    fp32 output, flat negative: 2^-16 -- at most N / 32 tile-level accumulations round at 2^-24 each, 2^-17 at N = 4096,
    doubled.  16-bit output: the half-ulp of the output type at c/N (attn_exact.census_tolerance: in c/N's own binade, the
    figure a correctly rounded result reaches) plus 2^-16 c/N; the ones channel exactly 1.
  * roll-call: over the passes every key of every key list is aimed at by exactly one query; the output must decode to the
    aimed key for every (query, head), and max |out - V[target]| <= 2^-15 + half-ulp of the output type.  Where a bank branch
    injects and the pass aims across frames, the source branch (which sees its own frame only) is held to the ordinary
    attention bound against the fp64 reference.
  * every output is finite and the rows of branches the call does not own keep the sentinel they were filled with.

Measured on an MI355X: every census case meets its tolerance (fp32 output, zero: at most 6e-8 relative against 9.5e-7), every
roll-call decodes 100 % of its (query, head) pairs, and max |out - V[target]| is 0.  The roll-call found the one-tile, ping-pong
and four-bank forms at head dim 64 summing the denominator from the fp32 P beside a numerator of bf16 P (a one-hot output of
1 - 2^-8, 3.906e-3 off, in 32 bf16 cases); they now sum the rounded P.

The signed-error probe runs every attention form on its N(0,1) input with fp32 output: T = mean(sign(ref) (out - ref) /
(softmax.|V|)) against a CPU emulation that rounds P to nearest (T_rne) or truncates it with an fp32 denominator (T_trunc);
|T_rne| <= |T_trunc| / 8 is the precondition and |T_kernel| <= |T_trunc| / 4 the assertion.
"""
import pytest
import torch

from tests import attn_exact as ax
from tests import kernel_forms as kf
from tests.test_kernel_forms_gpu import _attn_inputs, _rnd
from tests.test_kernels_gpu import attn_bound, attn_ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
ROLL_ATOL = 2.0 ** -15


def _ops():
    from tokenflow_amd import ops
    return ops


def _launch(ops, case, mode, dtype, out_dtype, dq, dk, dv):
    """The plan of the call, asserted; then the call into a sentinel-filled `out`.  Returns the output on the CPU as
    [nbr, Kq, S, D] after checking that it is finite and that unowned branches are untouched."""
    spec = case.spec
    case.check_plan(case.plan(ops, dtype, out_dtype, **mode), dtype, **mode)
    out = torch.full((spec.nbr * spec.Kq, spec.S, spec.D), ax.SENTINEL, dtype=out_dtype, device="cuda")
    case.call(ops, dq, dk, dv, out, **mode)
    o = out.cpu().view(spec.nbr, spec.Kq, spec.S, spec.D)
    assert torch.isfinite(o.float()).all(), f"{case.name} {mode}"
    for b in range(spec.nbr):
        if b not in spec.owned:
            assert bool((o[b] == ax.SENTINEL).all()), f"{case.name} {mode}: branch {b} is not the call's to write"
    return o


def _census(case, dtype, kind):
    ops, spec = _ops(), case.spec
    v, ones = ax.census_v(spec)
    c, n = ax.census_expected(spec, v)
    q, k = ax.census_qk(spec, kind, case.seed)
    dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
    c4, n4 = c.view(spec.nbr, spec.Kq, 1, -1)[spec.owned], n.view(spec.nbr, spec.Kq, 1, 1)[spec.owned]
    for mode in case.modes:
        for out_dtype in (torch.float32, dtype):
            o = _launch(ops, case, mode, dtype, out_dtype, dq, dk, dv)[spec.owned]
            viol = ax.census_violation(o, c4, n4, kind, out_dtype)
            e = (c4.double() / n4.double()).expand_as(o)
            rel = ((o.double() - e).abs() / e.clamp_min(1e-300)).masked_fill(e == 0, 0)
            print(f"{case.name} {mode} census {kind} {dtype} -> {out_dtype}: worst |out - c/N| / (c/N) = {float(rel.max()):.3e}, "
                  f"{viol:.3g} of its tolerance")
            if viol > 1.0:
                err = torch.where(e == 0, (o != 0) * 1e30, (o.double() - e).abs() / ax.census_tolerance(e.clamp_min(1e-300), kind, out_dtype))
                b, f, s, ch = (int(x) for x in torch.unravel_index(err.argmax(), err.shape))
                raise AssertionError(f"{case.name} {mode} census {kind} {dtype} -> {out_dtype}: {viol:.3g} x the tolerance at branch "
                                     f"{spec.owned[b]} query frame {f} row {s} head {ch // spec.d} channel {ch % spec.d}: "
                                     f"got {float(o[b, f, s, ch])!r}, count {int(c4[b, f, 0, ch])} / {int(n4[b, f, 0, 0])}")
            if out_dtype != torch.float32:
                assert bool((o[..., ones] == 1).all()), f"{case.name} {mode} census {kind} {dtype}: the ones channel is not exactly 1"


def _rollcall(case, dtype):
    ops, spec = _ops(), case.spec
    k, gain, seed, leak = ax.rollcall_keys(spec, case.seed)
    assert leak <= ax.LEAK_MAX
    v = ax.rollcall_v(spec)
    dk, dv = k.to(dtype).cuda(), v.to(dtype).cuda()
    worst, n_pairs, n_expected = 0.0, 0, 0
    for r, own in ax.rollcall_passes(spec):
        frame, pos = ax.rollcall_aims(spec, r, own)
        q = ax.rollcall_q(spec, k, gain, frame, pos)
        tf, tp, code, exact = ax.rollcall_targets(spec, frame, pos)
        want = ax.rollcall_expected(spec, v, tf, tp).view(spec.nbr, spec.Kq, spec.S, spec.D)
        dq = q.to(dtype).cuda()
        src_ref = None
        n_expected += len(case.modes) * sum(exact[b] for b in spec.owned) * spec.Kq * spec.S * spec.H
        for mode in case.modes:
            o = _launch(ops, case, mode, dtype, dtype, dq, dk, dv).float()
            got = ax.rollcall_decode(spec, o)
            for b in spec.owned:
                what = f"{case.name} {mode} roll-call {dtype} pass {r}{' (own frame)' if own else ''} branch {b}"
                if not exact[b]:      # the source under a cross-frame aim of an injecting bank branch: the ordinary bound
                    if src_ref is None:
                        src_ref = ax.reference(spec.only([0]), q, k, v, want_abs=True)
                    ref, ref_abs = (t.view(spec.nbr, spec.Kq, spec.S, spec.D)[0].float() for t in src_ref)
                    over = float(((o[0] - ref).abs() - attn_bound(ref, ref_abs, dtype)).max())
                    assert over <= 0, f"{what}: exceeds the attention bound by {over:.3e}"
                    continue
                bad = got[b] != code[b]
                if bool(bad.any()):
                    f, s, h = (int(x) for x in torch.nonzero(bad)[0])
                    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} (query, head) pairs read another key; first: query "
                                         f"frame {f} row {s} head {h} aimed at frame {int(tf[b, f, s, h])} row {int(tp[b, f, s, h])} "
                                         f"(code {int(code[b, f, s, h])}), decoded code {int(got[b, f, s, h])}")
                n_pairs += bad.numel()
                err = float((o[b] - want[b]).abs().max())
                worst = max(worst, err)
                assert err <= ROLL_ATOL + ax.HALF_ULP[dtype], f"{what}: max |out - V[target]| = {err:.3e}"
    print(f"{case.name} roll-call {dtype}: gain {gain}, seed {seed}, leak bound {leak:.2e}, {n_pairs} (query, head) pairs decoded, "
          f"max |out - V[target]| {worst:.3e}")
    assert n_pairs == n_expected      # nothing left out


def _check(case, dtype, kind):
    if kind == "roll":
        _rollcall(case, dtype)
    else:
        _census(case, dtype, kind)


KINDS = ["zero", "flat", "roll"]


@pytest.mark.parametrize("name", list(ax.FORM_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_kernel_forms(name, dtype, kind):
    _check(ax.FORM_CASES[name], dtype, kind)


@pytest.mark.parametrize("name", list(ax.SET_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_frame_sets_and_windows(name, dtype, kind):
    _check(ax.SET_CASES[name], dtype, kind)


@pytest.mark.parametrize("name", list(ax.EDIT_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_edits(name, dtype, kind):
    _check(ax.EDIT_CASES[name], dtype, kind)


@pytest.mark.parametrize("name", list(ax.RUN_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_runs(name, dtype, kind):
    _check(ax.RUN_CASES[name], dtype, kind)


@pytest.mark.parametrize("name", list(ax.SEGMENT_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_segments(name, dtype, kind):
    _check(ax.SEGMENT_CASES[name], dtype, kind)


# -------------------------------------------------------------------------------------------------- signed-error probe
PROBE_CASES = [(f, i) for f, cs in kf.CASES.items() for i, c in enumerate(cs) if "dh" in c]


@pytest.mark.parametrize("form,i", PROBE_CASES, ids=[f"{f}-{i}" for f, i in PROBE_CASES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_signed_error_probe(form, i, dtype):
    ops = _ops()
    c = kf.CASES[form][i]
    case = ax.FORM_CASES[f"form-{form}-{i}"]
    spec = case.spec
    K, S, h, d = c["K"], c["S"], c["heads"], c["dh"]
    case.check_plan(case.plan(ops, dtype, torch.float32), dtype)
    q, k, v = (_rnd(dtype)(x) for x in _attn_inputs(K, S, h * d, h, "randn", seed=K * 1000 + S + d + 5))
    ref, ref_abs, _ = attn_ref(q, k, v, h, d ** -0.5, c["inject"], need_sigma=False)
    out = torch.zeros(3 * K, S, h * d, dtype=torch.float32, device="cuda")
    ops.ext_attn(q.to(dtype).cuda(), k.to(dtype).cuda(), v.to(dtype).cuda(), h, d ** -0.5, c["inject"], out=out, part=c["part"],
                 no_split=c["no_split"], fused=c["fused"], hints=c["hints"], fold_scale=c["fold_scale"])
    sel = lambda t: t.view(3, K, S, -1)[spec.owned]      # noqa: E731
    t_kernel = ax.signed_error(sel(out.cpu()), sel(ref), sel(ref_abs))
    t_rne, t_trunc = ax.signed_error_stats(spec, q, k, v, dtype)
    name = "bf16" if dtype == torch.bfloat16 else "f16"
    print(f"PROBE {form:32s} case {i} K{K} S{S} H{h} d{d} {name:4s} T_kernel {t_kernel:+.3e}  T_rne {t_rne:+.3e}  T_trunc {t_trunc:+.3e}  "
          f"|T_kernel| / |T_trunc| {abs(t_kernel) / abs(t_trunc):.3f}")
    assert abs(t_rne) <= abs(t_trunc) / 8, "precondition: rounding to nearest is not far enough inside the truncation bias"
    assert abs(t_kernel) <= abs(t_trunc) / 4, f"signed error {t_kernel:+.3e} against a truncation bias of {t_trunc:+.3e}"


def test_case_tables_are_those_of_the_frame_set_tests():
    """attn_exact keeps literal copies (it is imported by a CPU test and pulls in no GPU test module)."""
    from tests import test_frame_sets_gpu as fs
    assert fs.K_ATTN == ax.K_SETS and all(ax.SET_TABLES[t] == fs.TABLES[t] for t in ax.SET_TABLES)
    assert [tuple(c) for c in fs.ATTN_CASES] == ax.SET_SHAPES
    assert ax.WINDOWS_R1 == _ops().bank_windows(ax.K_SETS, 1)
