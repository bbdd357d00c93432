"""tf_layer_norm / tf_add_layer_norm on inputs whose fp32 arithmetic is exact (tests/ln_exact.py; proven on the CPU by
tests/test_ln_exact_cpu.py): every bit of every output element and of every 1/||y|| is decided, nothing hides in a tolerance.

  * boundaries: every lanes-per-row and pieces-per-lane switch of layer_norm_kernel (D = 384|392, 512|520, 768|776, 1024|1032)
    beside the model's widths, 37 rows; input bf16 / f16 / fp32 x output bf16 / f16 / fp32 x weights none / gamma / beta / both x
    weight dtype 16-bit / fp32 x the three eps families -- `ops.layer_norm` with its side output, and `ops.add_layer_norm`
    with a stripe of rows whose sum rounds in the 16-bit sum dtype;
  * second trips: shapes past the grid cap for 16, 32 and 64 lanes per row, 3 and 4 pieces per lane, plain (+ 1/||y||) and ADD,
    bf16 and fp32 input; every row has its own exact reference, so a row group prefetched for the wrong trip shows;
  * one non-exact check: the second-trip shapes on N(0,1) * 3 + 0.5 rows against torch's fp32 layer_norm with an fp32 output,
    where a D - 1 divisor is far outside the bound.

The references are fp64 on the device.  1/||y|| is held to bit equality with the IEEE fp32 square root and division of the
exact sum of squares (`lx.inv_sqrt32` on the CPU)."""
import pytest
import torch

from tests import ln_exact as lx
from tests.test_kernels_gpu import layer_norm_bound

pytestmark = pytest.mark.gpu

LN_GRID_CAP = 256 * 8      # layer_norm.hip:211 (launch_ln_lpr): blocks capped at 256 * TF_TUNE_LN_WGS_PER_CU, default 8 (:209)
DTS = (torch.bfloat16, torch.float16, torch.float32)
ROWS = 37                  # ragged against 16, 8 and 4 rows per workgroup
STRIDE_SHAPES = [(8, 2 * 32768 + 16 + 5), (384, 32768 + 37), (512, 32768 + 37), (520, 16384 + 19), (1024, 16384 + 19),
                 (1032, 8192 + 7), (2048, 2 * 8192 + 3)]


def _ops():
    from tokenflow_amd import ops
    return ops


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _trips(D, rows):
    """Trips of a wave's row loop: a workgroup of 4 waves holds 4 * 64 / lanes-per-row rows (layer_norm.hip:206)."""
    return -(-rows // (LN_GRID_CAP * 4 * (64 // lx.lanes_per_row(D))))


def _same(got, want, what, D):
    if not torch.equal(_bits(got), _bits(want)):
        bad = (_bits(got) != _bits(want)).nonzero()
        r, c = (int(v) for v in bad[0])
        pytest.fail(f"{what}: {bad.shape[0]} of {want.numel()} elements differ; first: row {r} column {c} (piece {c // 8}, lane "
                    f"{(c // 8) % lx.lanes_per_row(D)}, trip {_trips(D, r + 1) - 1}) got {float(got[r, c])} want {float(want[r, c])}; "
                    f"rows hit: {sorted(set(bad[:, 0].tolist()))[:8]}")


def _same_inv(inv, ss, what):
    want = lx.inv_norm_expected(ss)
    got = inv.cpu()
    if not torch.equal(_bits(got), _bits(want)):
        bad = (_bits(got) != _bits(want)).nonzero().flatten()
        r = int(bad[0])
        pytest.fail(f"{what}: 1/||y|| differs from the IEEE fp32 1/sqrt(ss) on {bad.numel()} of {want.numel()} rows; first: row "
                    f"{r} ss {float(ss[r])} got {float(got[r]).hex()} want {float(want[r]).hex()}")


def _w(t, dt):
    return None if t is None else t.to(dt)


# ----------------------------------------------------------------------------------------------------------- boundaries
@pytest.mark.parametrize("D", lx.DS)
def test_layer_norm_exact_at_every_boundary(D):
    ops = _ops()
    assert lx.families(D) == (lx.FAMILIES if D != 776 else ("eps3", "eps15"))
    n = 0
    for family in lx.families(D):
        fam = lx.make(D, ROWS, family, device="cuda")
        for which in (None, "gamma", "beta", "both"):
            g, b = lx.weights(D, family, which, device="cuda")
            refs = {dt: lx.reference(fam["x"], g, b, fam["eps"], dt) for dt in DTS}
            for want, ss in refs.values():
                lx.assert_ss_exact(want, ss)
            for in_dt in DTS:
                x = fam["x"].to(in_dt)
                w16 = in_dt if in_dt != torch.float32 else torch.float16
                for w_dt in ((w16, torch.float32) if which else (None,)):
                    for out_dt in DTS:
                        what = f"layer_norm D={D} {family} weights={which}/{w_dt} in={in_dt} out={out_dt}"
                        out, inv = ops.layer_norm(x, _w(g, w_dt), _w(b, w_dt), fam["eps"], out_dt, want_inv_norm=True)
                        _same(out, refs[out_dt][0], what, D)
                        _same_inv(inv, refs[out_dt][1], what)
                        n += 1
    assert n == len(lx.families(D)) * 3 * 3 * 7


def _stripe_vs_torch(out, total, on, g, b, eps, out_dt, what):
    """layer_norm_bound of torch's fp32 layer_norm (on the CPU, as test_layer_norm_vs_torch_fp32) on the stripe rows.  Called
    without beta only: the bound is relative to max(1, |y|), the error model of y = z * gamma, and says nothing about an element
    whose z * gamma cancels against an integer beta of up to 31."""
    assert b is None
    D = total.shape[-1]
    ref = torch.nn.functional.layer_norm(total[on].float().cpu(), (D,), None if g is None else g.float().cpu(), None, eps)
    err = (out[on].float().cpu() - ref).abs()
    bound = layer_norm_bound(ref, out_dt)
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


@pytest.mark.parametrize("D", lx.DS)
def test_add_layer_norm_exact_at_every_boundary(D):
    """a + b = the family's x off the stripe: the sum equals torch's `a + b` everywhere, the norm equals the exact reference off
    the stripe; on the stripe (the fp32 sum does not fit the 16-bit sum dtype) the norm must see the ROUNDED sum: bit equal to
    `ops.layer_norm(total)` and (without beta, see _stripe_vs_torch) within layer_norm_bound of torch's fp32 layer_norm of it."""
    ops = _ops()
    pairs = [(dt, dt) for dt in DTS] + [(torch.bfloat16, torch.float32), (torch.float32, torch.float16)]
    for family in lx.families(D):
        fam = lx.make(D, ROWS, family, device="cuda")
        splits = {dt: lx.split_add(fam, dt) for dt in DTS}
        for which in (None, "gamma", "beta", "both"):
            g, b = lx.weights(D, family, which, device="cuda")
            refs = {dt: lx.reference(fam["x"], g, b, fam["eps"], dt)[0] for dt in DTS}
            for a_dt, b_dt in pairs:
                sum_dt = torch.promote_types(a_dt, b_dt)
                pa, pb, on = splits[sum_dt]
                pa, pb = pa.to(a_dt), pb.to(b_dt)
                assert int(on.sum()) == (5 if sum_dt != torch.float32 else 0)
                for w_dt in ((torch.bfloat16, torch.float32) if which else (None,)):
                    for out_dt in DTS:
                        what = f"add_layer_norm D={D} {family} weights={which}/{w_dt} a={a_dt} b={b_dt} out={out_dt}"
                        total, out = ops.add_layer_norm(pa, pb, _w(g, w_dt), _w(b, w_dt), fam["eps"], out_dt)
                        want_total = pa + pb
                        assert total.dtype == sum_dt and torch.equal(_bits(total), _bits(want_total)), what
                        assert torch.equal(total[~on].double(), fam["x"][~on])
                        _same(out[~on], refs[out_dt][~on], what + " (rows off the stripe, renumbered)", D)
                        if bool(on.any()):
                            assert bool((total.double() != pa.double() + pb.double())[on].any(1).all()), what
                            sep = ops.layer_norm(want_total, _w(g, w_dt), _w(b, w_dt), fam["eps"], out_dt)[0]
                            assert torch.equal(_bits(out[on]), _bits(sep[on])), what
                            if b is None:
                                _stripe_vs_torch(out, want_total, on, g, b, fam["eps"], out_dt, what)


def test_single_weight_is_taken_as_given():
    """gamma alone and beta alone are accepted by `ops` (each pointer is staged on its own, ln_row.h): not a refusal to assert."""
    ops = _ops()
    fam = lx.make(320, ROWS, "eps3", device="cuda")
    for which in ("gamma", "beta"):
        g, b = lx.weights(320, "eps3", which, device="cuda")
        out, _ = ops.layer_norm(fam["x"].bfloat16(), _w(g, torch.float32), _w(b, torch.float32), 3.0, torch.float32)
        _same(out, lx.reference(fam["x"], g, b, 3.0, torch.float32)[0], which, 320)


# ---------------------------------------------------------------------------------------------------------- second trips
@pytest.mark.parametrize("D,rows", STRIDE_SHAPES)
@pytest.mark.parametrize("in_dt", [torch.bfloat16, torch.float32])
def test_layer_norm_exact_past_the_grid_cap(D, rows, in_dt):
    """Every wave takes a second trip (the one-deep prefetch pipeline of layer_norm_kernel), the last one with a ragged tail;
    plain with 1/||y||, and ADD (x and the residual both prefetched)."""
    ops = _ops()
    trips = _trips(D, rows)
    assert trips >= 2 and trips == (3 if D in (8, 2048) else 2), (D, rows, trips)
    family = "scaled" if in_dt == torch.bfloat16 else "eps15"
    out_dt = in_dt
    fam = lx.make(D, rows, family, device="cuda")
    per_trip = LN_GRID_CAP * 4 * (64 // lx.lanes_per_row(D))
    g, b = lx.weights(D, family, device="cuda")
    want, ss = lx.reference(fam["x"], g, b, fam["eps"], out_dt)
    # a row and the row one trip later differ in y: a prefetched group consumed on the wrong trip cannot pass
    assert bool((want[:rows - per_trip] != want[per_trip:]).any(1).all())
    lx.assert_ss_exact(want, ss)
    what = f"D={D} rows={rows} {family} in={in_dt}"
    gw, bw = g.float(), b.float()
    out, inv = ops.layer_norm(fam["x"].to(in_dt), gw, bw, fam["eps"], out_dt, want_inv_norm=True)
    _same(out, want, "layer_norm " + what, D)
    _same_inv(inv, ss, "layer_norm " + what)
    del out, inv
    pa, pb, on = lx.split_add(fam, in_dt)
    assert bool(on.any()) == (in_dt != torch.float32)
    pa, pb = pa.to(in_dt), pb.to(in_dt)
    total, out = ops.add_layer_norm(pa, pb, gw, bw, fam["eps"], out_dt)
    want_total = pa + pb
    assert torch.equal(_bits(total), _bits(want_total)), "add_layer_norm sum " + what
    _same(out[~on], want[~on], "add_layer_norm " + what, D)
    if bool(on.any()):
        sep = ops.layer_norm(want_total[on], gw, bw, fam["eps"], out_dt)[0]
        assert torch.equal(_bits(out[on]), _bits(sep)), "add_layer_norm stripe " + what
        del out, sep
        _, out = ops.add_layer_norm(pa, pb, gw, None, fam["eps"], out_dt)
        _same(out[~on], lx.reference(fam["x"], g, None, fam["eps"], out_dt)[0][~on], "add_layer_norm (gamma) " + what, D)
        _stripe_vs_torch(out, want_total, on, g, None, fam["eps"], out_dt, what)


@pytest.mark.parametrize("D,rows", STRIDE_SHAPES)
def test_layer_norm_vs_torch_fp32_past_the_grid_cap(D, rows):
    """The inputs and the bound of test_layer_norm_vs_torch_fp32 at the second-trip shapes, fp32 output: a D - 1 divisor is
    1 / (2 D) relative, 2.4e-4 at D = 2048, against a bound of 2e-6."""
    ops = _ops()
    assert _trips(D, rows) >= 2
    g = torch.Generator().manual_seed(rows * 7 + D)
    x = (torch.randn(rows, D, generator=g) * 3 + 0.5).bfloat16()
    w = 1 + 0.2 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    ref = torch.nn.functional.layer_norm(x.float(), (D,), w, b, 1e-5)
    out, inv = ops.layer_norm(x.cuda(), w.cuda(), b.cuda(), 1e-5, torch.float32, want_inv_norm=True)
    got = out.cpu()
    err = (got - ref).abs()
    bound = layer_norm_bound(ref, torch.float32)
    print(f"D={D} rows={rows}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    assert torch.allclose(inv.cpu(), 1.0 / got.double().norm(dim=-1).float(), rtol=2e-6, atol=0)
    ta, tb = x.cuda(), (torch.randn(rows, D, generator=g) + 0.3).cuda()
    total, out2 = ops.add_layer_norm(ta, tb, w.cuda(), b.cuda(), 1e-5, torch.float32)
    assert torch.equal(total, ta + tb)
    ref2 = torch.nn.functional.layer_norm(total.cpu(), (D,), w, b, 1e-5)
    err2 = (out2.cpu() - ref2).abs()
    assert bool((err2 <= layer_norm_bound(ref2, torch.float32)).all()), float((err2 - layer_norm_bound(ref2, torch.float32)).max())
