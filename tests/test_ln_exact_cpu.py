"""tests/ln_exact.py proves itself on the CPU: the family is exact in fp32 (the kernel's formula in plain torch fp32, in two
reduction orders, equals the fp64 reference bit for bit at every D of the GPU suite), and the reference distinguishes every
bug the GPU suite is there to catch (each mutant of the reference differs from it at every D)."""
import pytest
import torch

from tests import ln_exact as lx

ROWS = 37          # ragged against 16, 8 and 4 rows per workgroup
GROUP = 16         # rows per "trip" of the next_trip_rows mutant
W16 = {torch.bfloat16: torch.bfloat16, torch.float16: torch.float16, torch.float32: torch.bfloat16}


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_fp32_identities():
    """What the family rests on, as measured: the fma identities hold at every D; fl(D * fl(1/D)) == 1 and the exact mean for all
    |k| <= 127 hold everywhere but D = 776, where 22 values of k fail (the powers of two and those near +-127)."""
    for D in lx.DS:
        unit, fm = lx.identities(D)
        assert fm == {3.0: True, 15.0: True}, D
        ks = lx.allowed_k(D)
        if D == 776:
            bad = sorted(set(range(-127, 128)) - set(ks))
            assert not unit and len(bad) == 22 and all(-k in bad for k in bad), bad
            assert {1, 2, 4, 8, 16, 32, 64, 127} <= set(bad), bad
            assert lx.families(D) == ("eps3", "eps15")
        else:
            assert unit and len(ks) == 255 and lx.families(D) == lx.FAMILIES, D


def test_rows_one_trip_apart_differ():
    """The sign pattern of a row is a function of the digit sum of r: rows 4096 * m apart differ in s (so in y, which does not see
    k_r or a_r) at every D -- D = 8 with its 16 patterns included."""
    for D in (8, 72, 2048):
        for step in (8192, 16384, 32768):
            s0 = lx._pattern(64, D)[0]
            for m in (1, 2):
                assert bool((s0 != lx._pattern(64, D, row0=m * step)[0]).any(1).all()), (D, step, m)


@pytest.mark.parametrize("D", lx.DS)
def test_family_is_exact_in_fp32(D):
    """The kernel's formula in torch fp32, lane order and reversed order, equals the fp64 reference in every bit of y and of
    1/||y||: all input, output and weight forms, every family that exists at D."""
    for family in lx.families(D):
        fam = lx.make(D, ROWS, family)
        for which, in_dt, out_dt in (("both", torch.bfloat16, torch.bfloat16), ("both", torch.float32, torch.float16),
                                     ("both", torch.float16, torch.float32), (None, torch.float32, torch.bfloat16),
                                     ("gamma", torch.bfloat16, torch.float16), ("beta", torch.float16, torch.bfloat16)):
            g, b = lx.weights(D, family, which)
            want, ss = lx.reference(fam["x"], g, b, fam["eps"], out_dt)
            lx.assert_ss_exact(want, ss)
            inv = lx.inv_norm_expected(ss)
            wd = W16[in_dt] if which != "gamma" else torch.float32
            for order in ("lanes", "reversed"):
                got, got_inv = lx.emulate_fp32(fam["x"].to(in_dt), None if g is None else g.to(wd), None if b is None else b.to(wd),
                                               fam["eps"], out_dt, order)
                assert torch.equal(_bits(got), _bits(want)), (family, which, out_dt, order)
                assert torch.equal(_bits(got_inv), _bits(inv)), (family, which, out_dt, order)
        if family == "scaled":
            assert len(set(fam["a"].tolist())) == 5
    # something rounds in each 16-bit output type, or "rounded once" is not tested
    fam = lx.make(D, ROWS, lx.families(D)[0])
    g, b = lx.weights(D, fam["family"])
    y32 = lx.reference(fam["x"], g, b, fam["eps"], torch.float32)[0]
    for dt in (torch.bfloat16, torch.float16):
        assert bool((y32.to(dt).float() != y32).any()), dt


@pytest.mark.parametrize("D", lx.DS)
def test_add_split_is_exact(D):
    """x = a + b: exact parts, the sum equal to x off the stripe, a rounding sum on it (asserted inside split_add); the emulated
    norm of the rounded sum equals the reference off the stripe."""
    for family in lx.families(D):
        fam = lx.make(D, ROWS, family)
        g, b = lx.weights(D, family)
        for sum_dt in (torch.bfloat16, torch.float16, torch.float32):
            pa, pb, on = lx.split_add(fam, sum_dt)
            assert int(on.sum()) == (0 if sum_dt == torch.float32 else 5)
            total, want = lx.add_reference(pa, pb, sum_dt, g, b, fam["eps"], torch.float32)
            assert torch.equal(total.double()[~on], fam["x"][~on])
            got = lx.emulate_fp32(total, g, b, fam["eps"], torch.float32, "lanes")[0]
            assert torch.equal(got[~on], want[~on]) and torch.equal(want[~on], lx.reference(fam["x"], g, b, fam["eps"],
                                                                                             torch.float32)[0][~on])


@pytest.mark.parametrize("D", lx.DS)
def test_every_mutant_is_caught(D):
    """Each mutant of the reference differs from the reference in y (fp32 output: nothing hides in a rounding) or in the sum of
    squares behind 1/||y|| (bf16 output), in at least one element, at every D.  The eps mutants cannot show in the eps = 0
    family and are held to the other two, which exist at every D."""
    caught = {m: False for m in lx.MUTANTS + lx.ADD_MUTANTS}
    for family in lx.families(D):
        fam = lx.make(D, ROWS, family)
        g, b = lx.weights(D, family)
        want, _ = lx.reference(fam["x"], g, b, fam["eps"], torch.float32)
        for m in lx.MUTANTS:
            if m == "inv_from_unrounded" or (m.startswith("eps_") and family == "scaled"):
                continue
            if m == "weights_shifted_one_piece" and D == 8:      # a row of ONE piece has no other piece to take weights from
                caught[m] = True
                continue
            got, _ = lx.reference(fam["x"], g, b, fam["eps"], torch.float32, mutant=m, group=GROUP)
            assert not torch.equal(got, want), f"D={D} {family}: the reference does not see mutant {m}"
            caught[m] = True
        for out_dt in (torch.bfloat16, torch.float16):      # the inverse norm itself moves, not only its operand
            _, ss = lx.reference(fam["x"], g, b, fam["eps"], out_dt)
            _, got_ss = lx.reference(fam["x"], g, b, fam["eps"], out_dt, mutant="inv_from_unrounded")
            assert not torch.equal(lx.inv_norm_expected(ss), lx.inv_sqrt32(got_ss.float())), \
                f"D={D} {family} {out_dt}: 1/||y|| of the unrounded y equals that of the rounded one"
            caught["inv_from_unrounded"] = True
        for sum_dt in (torch.bfloat16, torch.float16):
            pa, pb, on = lx.split_add(fam, sum_dt)
            total, want = lx.add_reference(pa, pb, sum_dt, g, b, fam["eps"], torch.float32)
            _, got = lx.add_reference(pa, pb, sum_dt, g, b, fam["eps"], torch.float32, mutant="norm_sees_unrounded_sum")
            hit = bool((got != want)[on].any(1).all()) and torch.equal(got[~on], want[~on])
            assert hit, f"D={D} {family} {sum_dt}: a stripe row does not show the unrounded sum"
            caught["norm_sees_unrounded_sum"] = True
    assert all(caught.values()), (D, [m for m, c in caught.items() if not c])
