"""Inputs on which the fp32 arithmetic of the row LayerNorm (csrc/ln_row.h) is EXACT, and its reference.

A row is x[r, c] = a_r * (k_r + s[r, c]):

  * s is +-1 with exactly D/2 of each sign: the first half of the columns spells a row code in bits (`_pattern`), the second
    half is its complement.  There are 2^min(D/2, 20) such patterns; the row code is the digit sum of r in that base, so rows
    one grid-stride trip apart (a multiple of 4096 rows) carry different patterns at every D;
  * a_r is a power of two (1 in the eps families, 2^-2 .. 2^2 in the "scaled" family);
  * k_r is an integer with |k_r| + 1 <= 128: every value is exact in bf16, f16 and fp32.

Then the row sum is the integer a_r * D * k_r, every deviation from the mean is +-a_r, the sum of squares is D * a_r^2, and no
partial sum of either rounds: the reduction order does not matter.  eps makes rstd a power of two:

  family "eps3"   : a_r = 1, eps = 3   -> fma(D, fl(1/D), 3) = 4,   rstd = 1/2
  family "eps15"  : a_r = 1, eps = 15  -> fma(D, fl(1/D), 15) = 16, rstd = 1/4
  family "scaled" : eps = 0, a_r = 2^e -> fl(D a^2 * fl(1/D)) = a^2, rstd = 2^-e

These are properties of fp32 at the given D, not theorems: `identities(D)` evaluates them in fp32 on the CPU, `allowed_k(D)`
keeps the k whose mean fl(fl(D k) * fl(1/D)) is k, and `make` asserts what it emits (D = 776: 22 values of k fail and
fl(D * fl(1/D)) != 1, so the "scaled" family does not exist there -- `families(D)`).

gamma and beta are column-coded integers exact in every weight dtype (`weights`), chosen so that the fp32 y is an integer (a
multiple of 1/4 without gamma), that some elements round in bf16 (|y| in 256 .. 512) and in f16 (|y| > 2048), and that the sum
of squares of the ROUNDED row stays below 2^24 in units of its lowest bit: the side output 1/||y|| is then one IEEE square root
and one IEEE division of an exact operand (`inv_norm_expected`, `inv_sqrt32`).

The reference (`reference`, `add_reference`) is the same formula in fp64 -- exact on these inputs -- rounded once with
`.to(out_dtype)`; its `mutant=` argument plants the bugs tests/test_ln_exact_cpu.py proves the family catches."""
import torch

DS = (8, 72, 320, 384, 392, 512, 520, 640, 768, 776, 1024, 1032, 1280, 1536, 2048)
EPS = {"eps3": 3.0, "eps15": 15.0, "scaled": 0.0}
FAMILIES = tuple(EPS)
MUTANTS = ("eps_dropped", "eps_over_d", "unbiased", "stats_miss_last_piece", "weights_shifted_one_piece", "next_trip_rows",
           "inv_from_unrounded", "gamma_without_beta", "beta_without_gamma")
ADD_MUTANTS = ("norm_sees_unrounded_sum",)

_F32 = torch.float32


def fma32(a, b, c):
    """fp32 fma(a, b, c) of fp32 tensors: the product is exact in fp64 (24 + 24 bits); the one fp64 rounding of the sum is
    harmless where it is used (the sum is exact, or further than 2^-29 relative from an fp32 tie)."""
    return (a.double() * b.double() + torch.as_tensor(c, dtype=torch.float64)).to(_F32)


def identities(D):
    """(fl(D * fl(1/D)) == 1, {eps: fma(D, fl(1/D), eps) == eps + 1}) in fp32 on the CPU."""
    d = torch.tensor(float(D), dtype=_F32)
    inv_d = torch.tensor(1.0, dtype=_F32) / d
    unit = bool(d * inv_d == 1.0)
    return unit, {eps: bool(fma32(d, inv_d, eps) == eps + 1.0) for eps in (3.0, 15.0)}


def allowed_k(D):
    """The k in -127 .. 127 whose fp32 mean is exact: fl(fl(D k) * fl(1/D)) == k."""
    k = torch.arange(-127, 128, dtype=_F32)
    inv_d = torch.tensor(1.0, dtype=_F32) / torch.tensor(float(D), dtype=_F32)
    ok = (k * float(D)) * inv_d == k
    return [int(v) for v in k[ok]]


def families(D):
    """The families that exist at D (every identity they rest on holds)."""
    unit, fm = identities(D)
    return tuple(f for f in FAMILIES if (unit if f == "scaled" else fm[EPS[f]]))


def lanes_per_row(D):
    """ln_lanes_per_row of csrc/ln_row.h."""
    return 16 if D <= 512 else 32 if D <= 1024 else 64


def _pattern(rows, D, row0=0, device="cpu"):
    """s [rows, D] of +-1 (int64) and the pattern count."""
    h = D // 2
    B = min(h, 20)
    npat = 1 << B
    r = torch.arange(row0, row0 + rows, dtype=torch.int64, device=device)
    code, t = torch.zeros_like(r), r.clone()
    while bool((t > 0).any()):          # digit sum of r in base npat: rows a multiple of npat apart differ
        code += t % npat
        t //= npat
    code %= npat
    c = torch.arange(h, dtype=torch.int64, device=device)
    bit = ((code[:, None] >> (c % B)[None]) & 1) ^ ((c // B) & 1)[None]
    half = 1 - 2 * bit
    return torch.cat([half, -half], dim=1), npat


def make(D, rows, family, row0=0, device="cpu"):
    """dict(x = fp64 [rows, D] of values exact in bf16 / f16 / fp32, k, a, eps) on `device`; preconditions asserted (the fp32
    identities on the CPU, whatever the device)."""
    assert D % 8 == 0 and family in families(D), (D, family)
    ks = allowed_k(D)
    assert len(ks) >= 200, (D, len(ks))
    s, npat = _pattern(rows, D, row0, device)
    assert bool((s.sum(1) == 0).all()) and bool((s.abs() == 1).all())
    r = torch.arange(row0, row0 + rows, dtype=torch.int64, device=device)
    k = torch.tensor(ks, dtype=torch.int64, device=device)[(r // npat + 5 * (r % npat)) % len(ks)]
    a = torch.ones(rows, dtype=torch.float64, device=device) if family != "scaled" else 2.0 ** ((r % 5) - 2).double()
    x = a[:, None] * (k[:, None] + s).double()
    assert int((k.abs() + 1).max()) <= 128
    for dt in (torch.bfloat16, torch.float16, _F32):
        assert torch.equal(x.to(dt).double(), x), f"precondition: the family is not exact in {dt}"
    # the three fp32 identities for exactly what was emitted, in fp32 on the CPU
    inv_d = torch.tensor(1.0, dtype=_F32) / torch.tensor(float(D), dtype=_F32)
    tot, ac, kc = x.sum(1).cpu(), a.cpu(), k.cpu()
    assert torch.equal(tot.to(_F32).double(), tot) and torch.equal(tot, ac * kc * D)
    assert torch.equal((tot.to(_F32) * inv_d).double(), ac * kc), "precondition: the fp32 mean is not a_r * k_r"
    q = (ac * ac * D).to(_F32)
    assert torch.equal(q.double(), ac * ac * D)
    var = fma32(q, inv_d, EPS[family])
    assert torch.equal(var.double(), ac * ac + EPS[family]), "precondition: the fp32 variance + eps is not a power of two"
    rstd = inv_sqrt32(var)
    assert torch.equal(rstd.double() * ac, torch.full_like(ac, {"eps3": 0.5, "eps15": 0.25, "scaled": 1.0}[family]))
    return {"x": x, "k": k, "a": a, "eps": EPS[family], "family": family}


def weights(D, family, which="both", device="cpu"):
    """(gamma, beta) as fp64 [D] or None, exact in bf16 / f16 / fp32.  a_r * rstd * gamma_c is 1 + c % 7, 268 on every 64th
    column, 2048 on columns 5 and D - 3; beta_c is c % 63 - 31, and 33 / 35 on those two columns."""
    c = torch.arange(D, dtype=torch.int64, device=device)
    m = 1 + c % 7
    m[c % 64 == 9] = 268
    beta = c % 63 - 31
    for col, bv in ((5, 33), (D - 3, 35)):
        m[col], beta[col] = 2048, bv
    gamma = (m * {"eps3": 2, "eps15": 4, "scaled": 1}[family]).double()
    beta = beta.double()
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(gamma.to(dt).double(), gamma) and torch.equal(beta.to(dt).double(), beta)
    return (gamma if which in ("both", "gamma") else None), (beta if which in ("both", "beta") else None)


def reference(x, gamma, beta, eps, out_dtype, mutant=None, group=None):
    """(y rounded once to out_dtype, fp64 sum of squares of the rounded rows) by the kernel's formula in fp64.  x, gamma, beta:
    fp64 (or anything exactly convertible), on any device.  `mutant` plants one bug (MUTANTS); `group` = rows per trip."""
    x = x.double()
    D = x.shape[-1]
    g = torch.ones(D, dtype=torch.float64, device=x.device) if gamma is None else gamma.double()
    b = torch.zeros(D, dtype=torch.float64, device=x.device) if beta is None else beta.double()
    if mutant == "next_trip_rows" and x.shape[0] > group:
        x = torch.cat([x[group:], x[x.shape[0] - group:]])
    if mutant == "weights_shifted_one_piece":
        g, b = g.roll(8), b.roll(8)
    if mutant == "gamma_without_beta":
        b = torch.zeros_like(b)
    if mutant == "beta_without_gamma":
        g = torch.ones_like(g)
    xs = x[:, :-8] if mutant == "stats_miss_last_piece" else x
    # divisors as TENSORS: torch divides a device tensor by a Python scalar as a multiplication by its rounded reciprocal
    d = torch.full((1,), float(D), dtype=torch.float64, device=x.device)
    mean = torch.div(xs.sum(-1, keepdim=True), d)
    c = xs - mean
    q = (c * c).sum(-1, keepdim=True)
    e = {"eps_dropped": 0.0, "eps_over_d": eps / D}.get(mutant, eps)
    var = torch.div(q, d - 1 if mutant == "unbiased" else d) + e
    rstd = torch.div(torch.ones_like(var), var.sqrt())
    y = (x - mean) * rstd * g + b
    out = y.to(out_dtype)
    ss = ((y if mutant == "inv_from_unrounded" else out.double()) ** 2).sum(-1)
    return out, ss


def assert_ss_exact(out, ss):
    """The sum of squares of the rounded rows is exact in fp32 in ANY order: every element is a multiple of u = 1, 1/2 or 1/4
    and ss / u^2 < 2^24."""
    o = out.double()
    u = 1.0 if bool((o == o.round()).all()) else 0.5 if bool((2 * o == (2 * o).round()).all()) else 0.25
    assert bool((o / u == (o / u).round()).all()), "precondition: a rounded output is not a multiple of 1/4"
    assert float(ss.max()) / (u * u) < 2 ** 24, f"precondition: sum of squares {float(ss.max())} / {u}^2 reaches 2^24"


def inv_sqrt32(s32):
    """fl32(1 / fl32(sqrt(s))) of an fp32 tensor -- one IEEE square root, one IEEE division -- evaluated in fp64 and rounded:
    a square root or a quotient of fp32 operands rounded to 53 bits and then to 24 is the correctly rounded fp32 result
    (53 >= 2 * 24 + 2), so this is the IEEE value whatever instructions the host's fp32 `1.0 / x.sqrt()` is built from."""
    assert s32.dtype == _F32
    r = s32.double().sqrt().to(_F32).double()
    return torch.div(torch.ones_like(r), r).to(_F32)


def inv_norm_expected(ss):
    """The IEEE fp32 1 / sqrt(ss) of the exact sum of squares (`inv_sqrt32`), on the CPU."""
    s32 = ss.cpu().to(_F32)
    assert torch.equal(s32.double(), ss.cpu().double())
    return inv_sqrt32(s32)


def split_add(fam, sum_dtype, stripe=8):
    """x = a + b for the ADD form: b[r, c] = a_r * ((r + c) % 5 - 2), a = x - b, both exact in every dtype.  Where the sum is
    stored in 16 bit, every `stripe`-th row (r % stripe == 3) has a[r, c] = a_r * big on every third column, big = 512 (bf16) or
    4096 (f16), where the dtype's spacing is 4: the fp32 sum a_r * (big + t), t = +-1, +-2, is exact and does not fit the sum
    dtype.  Returns (a, b, bool mask of the stripe rows)."""
    x, ar = fam["x"], fam["a"]
    rows, D = x.shape
    dev = x.device
    r, c = torch.arange(rows, device=dev)[:, None], torch.arange(D, device=dev)[None]
    b = ar[:, None] * ((r + c) % 5 - 2).double()
    a = x - b
    on = torch.zeros(rows, dtype=torch.bool, device=dev)
    if sum_dtype != _F32:
        big = 512.0 if sum_dtype == torch.bfloat16 else 4096.0
        on = (torch.arange(rows, device=dev) % stripe) == 3
        a = torch.where(on[:, None] & (c % 3 == 0), ar[:, None] * big, a)
        tot = a + b
        assert torch.equal(tot.to(_F32).double(), tot)
        assert bool((tot.to(sum_dtype).double() != tot)[on].any(1).all()), "precondition: a stripe row does not round"
        assert torch.equal(tot[~on].to(sum_dtype).double(), tot[~on])
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(a.to(dt).double(), a) and torch.equal(b.to(dt).double(), b), f"precondition: a / b not exact in {dt}"
    assert torch.equal((a + b)[~on], x[~on])
    return a, b, on


def add_reference(a, b, sum_dtype, gamma, beta, eps, out_dtype, mutant=None):
    """(a + b rounded to sum_dtype, LayerNorm of THAT tensor by `reference`); the mutant normalises the unrounded sum."""
    tot = a.double() + b.double()
    total = tot.to(sum_dtype)
    return total, reference(tot if mutant == "norm_sees_unrounded_sum" else total, gamma, beta, eps, out_dtype)[0]


# ------------------------------------------------------------------------------------------ the kernel's formula in plain fp32
def emulate_fp32(x, gamma, beta, eps, out_dtype, order):
    """layer_norm_kernel's arithmetic with torch fp32 ops on the CPU -> (out, fp32 inv_norm).  order "lanes": the kernel's own
    (lane lr of the LPR sharing a row sums its pieces lr + LPR*j element by element, then the xor butterfly); order
    "reversed": eight accumulators (one per element of a 16-byte piece) walking the pieces from the last to the first, then
    added up from the last to the first."""
    x = x.to(_F32)
    rows, D = x.shape
    g = torch.ones(D, dtype=_F32) if gamma is None else gamma.to(_F32)
    b = torch.zeros(D, dtype=_F32) if beta is None else beta.to(_F32)
    inv_d = torch.tensor(1.0, dtype=_F32) / torch.tensor(float(D), dtype=_F32)

    def row_sum(v, fused_square):      # v [rows, D] -> [rows]
        lpr, pieces = lanes_per_row(D), D // 8
        if order == "reversed":
            acc = torch.zeros(rows, 8, dtype=_F32)
            for p in range(pieces - 1, -1, -1):
                t = v[:, p * 8:p * 8 + 8]
                acc = fma32(t, t, acc) if fused_square else acc + t
            tot = torch.zeros(rows, dtype=_F32)
            for i in range(7, -1, -1):
                tot = tot + acc[:, i]
            return tot
        np_ = -(-pieces // lpr)
        pad = torch.zeros(rows, np_ * lpr * 8, dtype=_F32)      # a lane without piece j adds nothing: + 0 is exact
        pad[:, :D] = v
        pad = pad.view(rows, np_, lpr, 8)
        lane = torch.zeros(rows, lpr, dtype=_F32)
        for j in range(np_):
            for i in range(8):
                t = pad[:, j, :, i]
                lane = fma32(t, t, lane) if fused_square else lane + t
        o = lpr // 2
        idx = torch.arange(lpr)
        while o:
            lane = lane + lane[:, idx ^ o]
            o //= 2
        assert bool((lane == lane[:, :1]).all())
        return lane[:, 0]

    mean = (row_sum(x, False) * inv_d)[:, None]
    c = x - mean
    rstd = inv_sqrt32(fma32(row_sum(c, True), inv_d, eps))[:, None]
    y = fma32(c * rstd, g[None], b[None])
    out = y.to(out_dtype)
    return out, inv_sqrt32(row_sum(out.to(_F32), True))
