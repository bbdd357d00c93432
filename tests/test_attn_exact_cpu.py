"""The exact-arithmetic attention tests have teeth (no GPU): tests/attn_exact.py's fp64 reference is mutated the way a subtly
wrong kernel would be, and the assertions of tests/test_attn_exact_gpu.py are run against the mutant.

  * census (zero and flat negative; a plain bank and a scattered frame set, ragged and tile-multiple S): a phantom key with
    k = 0 and v = 0 or a garbage row, the row after a frame's last one taken twice, a key taken from a non-member frame, a key
    dropped with its neighbour doubled -- each must miss the fp32-output tolerance by a factor of at least 8, and the
    unmutated reference must meet it (which also checks the closed-form count against the reference);
  * roll-call: the leak bound holds for every case run on the GPU; every key is the target of exactly one query over the
    passes; a swap of two V rows and an off-by-one key index are decoded as wrong;
  * signed-error probe: P truncated instead of rounded (fp32 denominator) gives a T at least 8 times that of rounding to
    nearest, so the probe's limit |T_trunc| / 4 is missed by the truncating mutant and met with room by the correct one.
"""
import math

import pytest
import torch

from tests import attn_exact as ax

SCATTERED = [ax.members(m) for m in ax.SET_TABLES["scattered"]]
SPECS = {
    "bank-S72": ax.Spec(3, 2, 72, 2, 40),
    "bank-S128-inject": ax.Spec(3, 3, 128, 2, 40, inject=True),
    "scattered-S72-inject": ax.Spec(3, 6, 72, 2, 64, sets=SCATTERED, inject=True),
    "scattered-S128": ax.Spec(3, 6, 128, 1, 40, sets=SCATTERED),
    "edits-scattered-S45": ax.Spec(5, 6, 45, 2, 40, sets=SCATTERED, inject=ax.edit_inject(0b01, 2)),
}


# ------------------------------------------------------------------------------------------------------------ mutants
def _append(kmat, vmat, krow, vrow):
    return torch.cat([kmat, krow.unsqueeze(0)]), torch.cat([vmat, vrow.unsqueeze(0)])


def phantom_zero(spec, b, qi, kmat, vmat, k5, v5):
    return _append(kmat, vmat, torch.zeros_like(kmat[0]), torch.zeros_like(vmat[0]))


def phantom_garbage(spec, b, qi, kmat, vmat, k5, v5):
    return _append(kmat, vmat, torch.zeros_like(kmat[0]), torch.full_like(vmat[0], 5.0))


def row_after_last(spec, b, qi, kmat, vmat, k5, v5):
    """One key past the end of the last member frame: row 0 of the frame stored behind it."""
    nxt = (spec.key_frames(b, qi)[-1] + 1) % spec.K
    return _append(kmat, vmat, k5[spec.qk_branch(b), nxt, 0], v5[b, nxt, 0])


def nonmember_key(spec, b, qi, kmat, vmat, k5, v5):
    """Key 3 of the first member read at the same position of a frame outside the key list (where there is one)."""
    out = [f for f in range(spec.K) if f not in spec.key_frames(b, qi)]
    if not out:
        return kmat, vmat
    kmat, vmat = kmat.clone(), vmat.clone()
    kmat[3], vmat[3] = k5[spec.qk_branch(b), out[0], 3], v5[b, out[0], 3]
    return kmat, vmat


def drop_and_double(spec, b, qi, kmat, vmat, k5, v5):
    kmat, vmat = kmat.clone(), vmat.clone()
    kmat[5], vmat[5] = kmat[6], vmat[6]
    return kmat, vmat


MUTANTS = [phantom_zero, phantom_garbage, row_after_last, nonmember_key, drop_and_double]


@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("kind", ["zero", "flat"])
def test_census_catches_every_mutant(name, kind):
    spec = SPECS[name]
    v, ones = ax.census_v(spec)
    c, n = ax.census_expected(spec, v)
    q, k = ax.census_qk(spec, kind, seed=11)
    for t in (q, k, v):      # every value is exact in both 16-bit types
        assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)
    tol = ax.TOL_ZERO_F32 if kind == "zero" else ax.TOL_FLAT_F32
    clean = ax.reference(spec, q, k, v)
    assert ax.census_violation(clean, c, n, kind, torch.float32) <= 1.0
    assert bool((c[:, :, ones] == n).all())                       # the ones channels count every key
    if kind == "flat":                                            # the common score of a query: -5 .. -25 nats
        s = torch.einsum("qc,kc->qk", q[0, :, :spec.d].double(), k[0, :, :spec.d].double()) * spec.scale
        assert bool((s == s[:, :1]).all()) and -25.0 <= float(s.min()) and float(s.max()) <= -5.0
    for mutant in MUTANTS:
        got = ax.reference(spec, q, k, v, mutate=mutant)
        viol = ax.census_violation(got, c, n, kind, torch.float32)
        print(f"{name} {kind} {mutant.__name__}: misses the tolerance {tol:.2e} by a factor of {viol:.3g}")
        assert viol >= 8.0, f"{mutant.__name__} would pass"
    # the 16-bit tolerance is the half-ulp AT c / N (and the value itself meets it once rounded)
    for dtype in (torch.bfloat16, torch.float16):
        assert ax.census_violation(clean.to(dtype), c, n, kind, dtype) <= 1.0
        assert ax.census_violation(ax.reference(spec, q, k, v, mutate=phantom_garbage), c, n, kind, dtype) >= 8.0


def test_census_violation_flags_zero_channels_and_non_finite():
    spec = SPECS["scattered-S128"]
    v, _ = ax.census_v(spec)
    c, n = ax.census_expected(spec, v)
    out = (c.double() / n.double()).expand(-1, spec.S, -1).clone()
    assert ax.census_violation(out, c, n, "zero", torch.float32) == 0.0
    assert bool((c == 0).any())
    bad = out.clone()
    bad[(c == 0).expand_as(bad)] = 1e-30
    assert ax.census_violation(bad, c, n, "zero", torch.float32) == math.inf
    bad = out.clone()
    bad[0, 0, 0] = float("nan")
    assert ax.census_violation(bad, c, n, "zero", torch.float32) == math.inf


# ----------------------------------------------------------------------------------------------------------- roll-call
def test_leak_bound_of_every_gpu_case():
    gains = {}
    for name, case in ax.GPU_CASES.items():
        spec = case.spec
        k, gain, seed, leak = ax.rollcall_keys(spec, case.seed)      # raises if no seed meets the bound
        assert leak <= ax.LEAK_MAX and gain in (1, 2, 4, 8, 16, 32), name
        maxoff = ax._rollcall_keys(spec.nbr, spec.K, spec.S, spec.H, spec.d, seed)[1]
        worst = max(maxoff[spec.qk_branch(b)] for b in spec.owned)
        assert leak == ax.leak_bound(spec.n_max(), spec.scale, gain, spec.d, worst), name
        assert gain == 1 or ax.leak_bound(spec.n_max(), spec.scale, gain // 2, spec.d, worst) > ax.LEAK_MAX, name      # the smallest
        assert sum(b for _, b in ax._code_bits(spec)) <= spec.d, name
        gains.setdefault((spec.d, gain), []).append(name)
    print({k_: len(v_) for k_, v_ in sorted(gains.items())})


def _mismatches(spec, out, code, branches):
    got = ax.rollcall_decode(spec, out).view(spec.nbr, spec.Kq, spec.S, spec.H)
    return int(sum((got[b] != code[b]).sum() for b in branches))


@pytest.mark.parametrize("name", list(SPECS))
def test_rollcall_reads_every_key_once_and_decodes_faults(name):
    spec = SPECS[name]
    k, gain, _seed, leak = ax.rollcall_keys(spec, 5)
    v = ax.rollcall_v(spec)
    assert torch.equal(v.abs(), torch.ones_like(v)) and torch.equal(k.abs(), torch.ones_like(k))
    seen = {}
    for r, own in ax.rollcall_passes(spec):
        frame, pos = ax.rollcall_aims(spec, r, own)
        q = ax.rollcall_q(spec, k, gain, frame, pos)
        tf, tp, code, exact = ax.rollcall_targets(spec, frame, pos)
        want = ax.rollcall_expected(spec, v, tf, tp)
        assert torch.equal(ax.rollcall_decode(spec, want).view(code.shape), code)
        one_hot = [b for b in range(spec.nbr) if exact[b]]
        assert one_hot[-spec.nbr + 1:] == list(range(1, spec.nbr)) and (0 in one_hot) == (own or not spec.any_inject())
        ref = ax.reference(spec, q, k, v)
        assert _mismatches(spec, ref, code, one_hot) == 0
        err = (ref - want).view(spec.nbr, -1)[one_hot].abs().max()
        assert float(err) <= 2.0 * leak <= 2.0 ** -15
        # a swap of two V rows and a key index off by one are decoded as wrong
        def swap(s, b, qi, km, vm, k5, v5):      # the first two V rows of every frame of the key list
            idx = torch.arange(len(vm))
            idx[0::s.S], idx[1::s.S] = idx[1::s.S].clone(), idx[0::s.S].clone()
            return km, vm[idx]
        shift = lambda s, b, qi, km, vm, k5, v5: (torch.roll(km, 1, 0), vm)                      # noqa: E731
        assert _mismatches(spec, ax.reference(spec, q, k, v, mutate=swap), code, one_hot) >= 2 * spec.H
        assert _mismatches(spec, ax.reference(spec, q, k, v, mutate=shift), code, one_hot) >= spec.S
        if not own:
            for b in range(1, spec.nbr):
                for qi in range(spec.Kq):
                    if r < len(spec.sets[qi]):
                        for h in range(spec.H):
                            seen.setdefault((b, qi, h), []).append(tf[b, qi, :, h] * spec.S + tp[b, qi, :, h])
    for (b, qi, h), parts in seen.items():      # over the passes: every key of the set, each exactly once
        want = torch.cat([torch.arange(f * spec.S, (f + 1) * spec.S) for f in spec.sets[qi]])
        assert torch.equal(torch.cat(parts).sort().values, want), (b, qi, h)


# -------------------------------------------------------------------------------------------------- signed-error probe
@pytest.mark.parametrize("K,S,H,d,dtype", [(2, 200, 2, 40, torch.bfloat16), (3, 181, 2, 80, torch.bfloat16),
                                           (2, 200, 2, 64, torch.float16)])
def test_probe_separates_truncation_from_rounding(K, S, H, d, dtype):
    g = torch.Generator().manual_seed(K * 1000 + S + d + 5)
    q, k, v = (torch.randn(3 * K, S, H * d, generator=g).to(dtype).float() for _ in range(3))
    spec = ax.Spec(3, K, S, H, d)
    t_rne, t_trunc = ax.signed_error_stats(spec, q, k, v, dtype)
    print(f"K{K} S{S} d{d} {dtype}: T_rne {t_rne:.2e}  T_trunc {t_trunc:.2e}")
    assert t_trunc < 0                                   # a shrink
    assert abs(t_rne) <= abs(t_trunc) / 8                # the probe's precondition: rounding to nearest is far inside the limit
    assert abs(t_trunc) > abs(t_trunc) / 4               # ... and the truncating mutant misses |T| <= |T_trunc| / 4 (by 4x)
    ref, ref_abs = ax.reference(spec, q, k, v, want_abs=True)
    assert ax.signed_error(ref.float(), ref, ref_abs) == pytest.approx(0.0, abs=abs(t_trunc) / 64)      # fp32 rounding alone
