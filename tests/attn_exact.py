"""Inputs that make the attention kernels' arithmetic exact, and the plain fp64 reference they are held to.

The attention bound of tests/test_kernels_gpu.py allows the worst case of rounding every probability, about one key's
weight.  The inputs built here leave the kernels nothing to round, so the tolerance drops to fp32 rounding and a single
key too many, a key read from the wrong place or a bias of 0.2 % stands far above it:

  * census "zero": q = 0, so every score is 0 and every P exactly 1; the output is a COUNT,
    out[c] = (sum of V[:, c] over the key list) / (number of keys), with small integers in V that say which keys were
    counted (a ones channel, the branch, the frame, the 64-key tile, the position inside the tile, j mod R);
  * census "flat negative": every key is the same vector u and q_i = -a_i u, so all scores of a query are bit-identical and
    lie between -5 and -25 nats: the output is the same count, and a zero-padded phantom key (score 0) destroys it;
  * roll-call: Rademacher keys, every query `gain` times the key it is aimed at, V the binary code of (branch, head, frame,
    position) as +-1 per channel: the softmax is one-hot up to a leak <= 2^-16 (asserted from the Gram matrix of the keys)
    and the output decodes by sign to the key that was read.  Over the passes every key of every query frame's key list is
    the target of exactly one query of that frame.

A `Spec` is the geometry of one call: per (branch, query frame) the explicit list of key frames.  `reference` is fp64 softmax
attention over those lists; the census expectation is written in closed form from V alone (`census_expected`).  GPU_CASES
lists the calls of tests/test_attn_exact_gpu.py; tests/test_attn_exact_cpu.py proves on mutated references that the
assertions have teeth.  Every value built here is exactly representable in bf16 and in f16.
"""
import functools
import math

import torch

from tests import attn_run_forms as rf
from tests import kernel_forms as kf

SENTINEL = 7.0
LEAK_MAX = 2.0 ** -16
HALF_ULP = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12, torch.float32: 2.0 ** -24}
# derived tolerances (relative to the count c / N; see the issue text repeated in tests/test_attn_exact_gpu.py)
TOL_ZERO_F32 = 2.0 ** -20
TOL_FLAT_F32 = 2.0 ** -16


class Spec:
    """Geometry of one attention call.  Branch 0 is the source (it attends to its own frame), branches 1 .. nbr-1 are bank
    branches: query frame qi attends to the frames `sets[qi]` of its own branch's V, in ascending order, with the k of
    its own branch or, where inject[b], with the source's q and k."""

    def __init__(self, nbr, K, S, H, d, sets=None, inject=False, qframes=None, owned=None):
        self.nbr, self.K, self.S, self.H, self.d = nbr, K, S, H, d
        self.qframes = list(range(K)) if qframes is None else list(qframes)
        self.Kq = len(self.qframes)
        self.sets = [sorted(s) for s in (sets if sets is not None else [range(K)] * self.Kq)]
        inj = [inject] * (nbr - 1) if isinstance(inject, bool) else list(inject)
        self.inject = [False] + [bool(x) for x in inj]
        self.owned = list(range(nbr)) if owned is None else list(owned)
        assert len(self.sets) == self.Kq and len(self.inject) == nbr
        assert all(f in s for f, s in zip(self.qframes, self.sets)), "a set holds its own frame"

    @property
    def D(self):
        return self.H * self.d

    @property
    def scale(self):
        return self.d ** -0.5

    def key_frames(self, b, qi):
        return [self.qframes[qi]] if b == 0 else self.sets[qi]

    def qk_branch(self, b):
        return 0 if self.inject[b] else b

    def any_inject(self):
        return any(self.inject[b] for b in self.owned)

    def n_max(self):
        return max(len(s) for s in self.sets) * self.S

    def only(self, branches):
        return Spec(self.nbr, self.K, self.S, self.H, self.d, self.sets, self.inject[1:], self.qframes, list(branches))


def edit_inject(mask, E):
    """Per bank branch [uncond_1, cond_1, uncond_2, ...] the injection flag of its edit."""
    return [bool((mask >> (b // 2)) & 1) for b in range(2 * E)]


# ------------------------------------------------------------------------------------------------------ fp64 reference
def reference(spec, q, k, v, mutate=None, want_abs=False):
    """fp64 softmax attention over the explicit key lists.  q [nbr*Kq,S,D], k, v [nbr*K,S,D] -> out [nbr*Kq,S,D] (float64;
    rows of branches the spec does not own hold SENTINEL), and softmax.|V| with want_abs.
    mutate(spec, b, qi, kmat, vmat, k5, v5) -> (kmat, vmat): a fault injected into the key list [n, H, d] of (b, qi)."""
    nbr, K, Kq, S, H, d = spec.nbr, spec.K, spec.Kq, spec.S, spec.H, spec.d
    q5 = q.double().view(nbr, Kq, S, H, d)
    k5, v5 = k.double().view(nbr, K, S, H, d), v.double().view(nbr, K, S, H, d)
    out = torch.full((nbr, Kq, S, H, d), SENTINEL, dtype=torch.float64)
    out_abs = torch.full_like(out, SENTINEL)
    for b in spec.owned:
        qb = spec.qk_branch(b)
        for qi in range(Kq):
            fr = torch.as_tensor(spec.key_frames(b, qi))
            kmat, vmat = k5[qb, fr].reshape(-1, H, d), v5[b, fr].reshape(-1, H, d)
            if mutate is not None:
                kmat, vmat = mutate(spec, b, qi, kmat, vmat, k5, v5)
            p = torch.softmax(torch.einsum("qhc,khc->hqk", q5[qb, qi], kmat) * spec.scale, dim=-1)
            out[b, qi] = torch.einsum("hqk,khc->qhc", p, vmat)
            if want_abs:
                out_abs[b, qi] = torch.einsum("hqk,khc->qhc", p, vmat.abs())
    out = out.view(nbr * Kq, S, H * d)
    return (out, out_abs.view(nbr * Kq, S, H * d)) if want_abs else out


# ------------------------------------------------------------------------------------------------------------- census
def _quantised_randn(shape, g):
    """N(0,1) rounded to sixteenths and clipped to +-4: at most 7 significant bits, exact in bf16 and in f16."""
    return (torch.randn(shape, generator=g) * 16).round().clamp(-64, 64) / 16


def census_v(spec):
    """V [nbr*K,S,D] of small integers and the mask [D] of the ones channels.  Per head the d channels hold, rotated by
    5 * head: 1 | branch + 1 | K frame indicators | indicators of the 64-key tile | pos % 64 | indicators of pos mod R in
    the R channels that remain."""
    nbr, K, S, H, d = spec.nbr, spec.K, spec.S, spec.H, spec.d
    pos = torch.arange(S).view(1, 1, S).expand(nbr, K, S)
    frame = torch.arange(K).view(1, K, 1).expand(nbr, K, S)
    branch = torch.arange(nbr).view(nbr, 1, 1).expand(nbr, K, S)
    feats = [torch.ones(nbr, K, S, dtype=torch.long), branch + 1]
    feats += [(frame == f).long() for f in range(K)]
    feats += [(pos // 64 == t).long() for t in range((S + 63) // 64)]
    feats += [pos % 64]
    R = d - len(feats)
    assert R >= 0, f"census: {len(feats)} channels do not fit head dim {d} (K {K}, S {S})"
    feats += [(pos % R == r).long() for r in range(R)]
    F = torch.stack(feats, dim=-1)                                          # [nbr, K, S, d]
    rot = (torch.arange(d).view(1, d) + 5 * torch.arange(H).view(H, 1)) % d  # channel c of head h holds feature rot[h, c]
    v = F[..., rot]                                                         # [nbr, K, S, H, d]
    assert int(v.max()) <= 64
    return v.reshape(nbr * K, S, H * d).float(), (rot == 0).reshape(H * d)


def census_expected(spec, v):
    """The count in closed form: (c, N), c [nbr*Kq, 1, D] int64 = sum of V over the key list, N [nbr*Kq, 1, 1] its length.
    The output of a census call is c / N in every query row."""
    nbr, K, Kq, S = spec.nbr, spec.K, spec.Kq, spec.S
    v4 = v.long().view(nbr, K, S, -1)
    c = torch.zeros(nbr, Kq, 1, v4.shape[-1], dtype=torch.long)
    n = torch.ones(nbr, Kq, 1, 1, dtype=torch.long)
    for b in range(nbr):
        for qi in range(Kq):
            fr = torch.as_tensor(spec.key_frames(b, qi))
            c[b, qi, 0] = v4[b, fr].sum((0, 1))
            n[b, qi] = len(fr) * S
    assert int(c.max()) < 2 ** 24
    return c.view(nbr * Kq, 1, -1), n.view(nbr * Kq, 1, 1)


def flat_multipliers(d):
    """Four distinct multipliers a (eighths: bf16- and f16-exact) whose common score -a sqrt(d) is about -6, -12, -18, -24."""
    a = [max(1, round(8 * t / math.sqrt(d))) / 8 for t in (6.0, 12.0, 18.0, 24.0)]
    assert len(set(a)) == 4 and all(5.0 <= x * math.sqrt(d) <= 25.0 for x in a), a
    return a


def census_qk(spec, kind, seed):
    """q [nbr*Kq,S,D], k [nbr*K,S,D] of the census family `kind` ("zero" | "flat")."""
    nbr, K, Kq, S, H, d = spec.nbr, spec.K, spec.Kq, spec.S, spec.H, spec.d
    g = torch.Generator().manual_seed(seed)
    if kind == "zero":
        return torch.zeros(nbr * Kq, S, H * d), _quantised_randn((nbr * K, S, H * d), g)
    assert kind == "flat"
    u = (torch.randint(0, 2, (H, d), generator=g) * 2 - 1).float()
    a = torch.tensor(flat_multipliers(d))
    ai = a[(torch.arange(S).view(S, 1) + torch.arange(H).view(1, H)) % 4]        # [S, H]
    q = (-ai.view(1, S, H, 1) * u.view(1, 1, H, d)).expand(nbr * Kq, S, H, d)
    k = u.view(1, 1, H, d).expand(nbr * K, S, H, d)
    return q.reshape(nbr * Kq, S, H * d).contiguous(), k.reshape(nbr * K, S, H * d).contiguous()


def census_tolerance(e, kind, out_dtype):
    """The absolute tolerance on an output whose exact value is e = c / N (a tensor).
    fp32 output: 2^-20 e (zero) / 2^-16 e (flat negative).  16-bit output: the half-ulp of the output type AT e plus
    2^-16 e.  The half-ulp is taken in e's own binade, 2^(floor(log2 e) - 8) in bf16 and 2^(floor(log2 e) - 11) in f16: it is
    between 2^-9 e and 2^-8 e (2^-12 e and 2^-11 e), and a correctly rounded result reaches it -- 11 / 576 rounds to the bf16
    value 0.01904296875, 2.8e-3 = 1.44 * 2^-9 of it away -- so no smaller figure can be asserted of a 16-bit output."""
    if out_dtype == torch.float32:
        return (TOL_ZERO_F32 if kind == "zero" else TOL_FLAT_F32) * e
    _, ex = torch.frexp(e)                      # e = m 2^ex, 0.5 <= m < 1: floor(log2 e) = ex - 1
    return torch.ldexp(torch.ones_like(e), ex - (9 if out_dtype == torch.bfloat16 else 12)) + 2.0 ** -16 * e


def census_violation(out, c, n, kind, out_dtype):
    """max |out - c/N| / census_tolerance over the channels with c > 0; inf if a channel with c = 0 is not exactly 0 or a
    value is not finite.  <= 1 passes."""
    out = out.double()
    if not bool(torch.isfinite(out).all()):
        return math.inf
    zero = (c == 0).expand_as(out)
    if bool((out[zero] != 0).any()):
        return math.inf
    e = (c.double() / n.double()).expand_as(out)[~zero]
    return float(((out[~zero] - e).abs() / census_tolerance(e, kind, out_dtype)).max())


# ----------------------------------------------------------------------------------------------------------- roll-call
@functools.lru_cache(maxsize=4)
def _rollcall_keys(nbr, K, S, H, d, seed):
    """Rademacher keys [nbr*K,S,D] and, per branch, the largest off-diagonal entry of the Gram matrix of that branch's K*S
    keys over the heads (every key list of the branch is a subset of them)."""
    g = torch.Generator().manual_seed(seed)
    k = (torch.randint(0, 2, (nbr, K, S, H, d), generator=g) * 2 - 1).float()
    maxoff = []
    for b in range(nbr):
        worst = -d
        for h in range(H):
            kk = k[b, :, :, h].reshape(K * S, d)
            gram = kk @ kk.T
            gram.fill_diagonal_(-d)
            worst = max(worst, int(gram.max()))
        maxoff.append(worst)
    return k.reshape(nbr * K, S, H * d), tuple(maxoff)


def leak_bound(n, scale, gain, d, maxoff):
    return n * math.exp(-scale * gain * (d - maxoff))


def rollcall_keys(spec, seed0):
    """(k, gain, seed, leak): the first seed >= seed0 whose keys meet the leak bound with a gain <= 32, and the smallest
    power-of-two gain that meets it."""
    used = sorted({spec.qk_branch(b) for b in spec.owned})
    for seed in range(seed0, seed0 + 8):
        k, maxoff = _rollcall_keys(spec.nbr, spec.K, spec.S, spec.H, spec.d, seed)
        worst = max(maxoff[b] for b in used)
        for gain in (1, 2, 4, 8, 16, 32):
            leak = leak_bound(spec.n_max(), spec.scale, gain, spec.d, worst)
            if leak <= LEAK_MAX:
                return k, gain, seed, leak
    raise AssertionError("roll-call: no seed meets the leak bound")


def _code_bits(spec):
    """[(field, bits)] of the code carried by V, lowest bit first."""
    nb = lambda n: max(1, (n - 1).bit_length())      # noqa: E731
    return [("pos", nb(spec.S)), ("frame", nb(spec.K)), ("head", nb(spec.H)), ("branch", nb(spec.nbr))]


def rollcall_code(spec, branch, head, frame, pos):
    code, shift = 0, 0
    for (name, bits), val in zip(_code_bits(spec), (pos, frame, head, branch)):
        code = code + (val << shift)
        shift += bits
    return code


def rollcall_v(spec):
    """V [nbr*K,S,D] of +-1: channel c of a head holds bit (c mod nbits) of the code of (branch, head, frame, position)."""
    nbr, K, S, H, d = spec.nbr, spec.K, spec.S, spec.H, spec.d
    nbits = sum(b for _, b in _code_bits(spec))
    assert nbits <= d, f"roll-call: a {nbits}-bit code does not fit head dim {d}"
    code = rollcall_code(spec, torch.arange(nbr).view(nbr, 1, 1, 1), torch.arange(H).view(1, 1, 1, H),
                         torch.arange(K).view(1, K, 1, 1), torch.arange(S).view(1, 1, S, 1))        # [nbr, K, S, H]
    bit = (code.unsqueeze(-1) >> (torch.arange(d) % nbits)) & 1
    return (bit * 2 - 1).float().reshape(nbr * K, S, H * d)


def rollcall_decode(spec, out):
    """out [.., S, D] -> the code read from the signs of the first nbits channels of every head, [.., S, H]."""
    nbits = sum(b for _, b in _code_bits(spec))
    o = out.reshape(*out.shape[:-1], spec.H, spec.d)[..., :nbits]
    return ((o > 0).long() << torch.arange(nbits)).sum(-1)


def _coprime(a, n):
    while math.gcd(a, n) != 1:
        a += 1
    return a


def rollcall_passes(spec):
    """The cross-frame passes (one per member of the largest set) and, under injection, one pass aimed inside the own frame."""
    m = max(len(s) for s in spec.sets)
    return [(r, False) for r in range(m)] + ([(0, True)] if spec.any_inject() else [])


def rollcall_aims(spec, r, own):
    """Aim of every q row: (frame, pos) as [nbr, Kq, S, H] each, by the branch that OWNS the q.
    Bank q rows (and, where a bank branch injects, the source's) aim through the bijection idx = (a (i + r S) + b0) mod (m S) on
    the key list of their frame's set, m its members: over r = 0 .. m-1 every key is the target of exactly one query.  The
    source's q aims through a bijection on its own frame when no branch injects, and every q does in the `own` pass.
    (a, b0) differ per head and branch; gcd(a, m S) = 1."""
    nbr, Kq, S, H = spec.nbr, spec.Kq, spec.S, spec.H
    frame = torch.empty(nbr, Kq, S, H, dtype=torch.long)
    pos = torch.empty_like(frame)
    i = torch.arange(S)
    for b in range(nbr):
        inside = own or (b == 0 and not spec.any_inject())
        for qi in range(Kq):
            members = [spec.qframes[qi]] if inside else spec.sets[qi]
            n = len(members) * S
            mem = torch.as_tensor(members)
            for h in range(H):
                a, b0 = _coprime(2 * (3 * h + 5 * b) + 3, n), 17 * h + 29 * b + 3
                idx = (a * (i + (r % len(members)) * S + (r if inside else 0)) + b0) % n
                frame[b, qi, :, h], pos[b, qi, :, h] = mem[idx // S], idx % S
    return frame, pos


def rollcall_q(spec, k, gain, frame, pos):
    """q [nbr*Kq,S,D]: every row `gain` times the key it is aimed at (the keys of the branch whose k that q meets)."""
    nbr, K, Kq, S, H, d = spec.nbr, spec.K, spec.Kq, spec.S, spec.H, spec.d
    k5 = k.view(nbr, K, S, H, d)
    hh = torch.arange(H).view(1, 1, H).expand(Kq, S, H)
    # the q of a bank branch that injects is never read; it is aimed like its own keys all the same
    q = torch.stack([k5[b][frame[b], pos[b], hh] for b in range(nbr)])
    return (gain * q).reshape(nbr * Kq, S, H * d)


def rollcall_targets(spec, frame, pos):
    """Per OUTPUT branch the aimed (frame, pos) [nbr, Kq, S, H], the expected code, and which branches are one-hot (`exact`):
    the source branch is not where a bank branch injects and the pass aims across frames."""
    src = [spec.qk_branch(b) for b in range(spec.nbr)]
    tf, tp = frame[src], pos[src]
    code = rollcall_code(spec, torch.arange(spec.nbr).view(-1, 1, 1, 1), torch.arange(spec.H).view(1, 1, 1, -1), tf, tp)
    own = torch.as_tensor(spec.qframes).view(1, -1, 1, 1)
    exact = [b != 0 or bool((tf[0] == own).all()) for b in range(spec.nbr)]
    return tf, tp, code, exact


def rollcall_expected(spec, v, tf, tp):
    """V of the aimed key for every output row: [nbr*Kq, S, D]."""
    nbr, K, Kq, S, H, d = spec.nbr, spec.K, spec.Kq, spec.S, spec.H, spec.d
    v5 = v.view(nbr, K, S, H, d)
    hh = torch.arange(H).view(1, 1, H).expand(Kq, S, H)
    return torch.stack([v5[b][tf[b], tp[b], hh] for b in range(nbr)]).reshape(nbr * Kq, S, H * d)


# -------------------------------------------------------------------------------------------------- signed-error probe
def _round16(p, dtype, truncate):
    """fp64 probabilities -> the values of `dtype`, rounded to nearest or truncated towards zero (p >= 0)."""
    p32 = p.float()
    if not truncate:
        return p32.to(dtype).double()
    if dtype == torch.bfloat16:
        return (p32.view(torch.int32) & -65536).view(torch.float32).double()
    h = p32.half()
    over = h.float() > p32
    h = torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)
    return h.double()


def signed_error_stats(spec, q, k, v, dtype):
    """(T_rne, T_trunc) of a CPU emulation on (q, k, v): fp64 softmax, P rounded to `dtype` to nearest (numerator and
    denominator from the rounded P) or truncated with the denominator summed from the fp32 P;
    T = mean(sign(ref) (out - ref) / (softmax.|V|)) over the owned branches, ref the fp64 result."""
    nbr, K, Kq, S, H, d = spec.nbr, spec.K, spec.Kq, spec.S, spec.H, spec.d
    q5 = q.double().view(nbr, Kq, S, H, d)
    k5, v5 = k.double().view(nbr, K, S, H, d), v.double().view(nbr, K, S, H, d)
    tot, cnt = [0.0, 0.0], 0
    for b in spec.owned:
        qb = spec.qk_branch(b)
        for qi in range(Kq):
            fr = torch.as_tensor(spec.key_frames(b, qi))
            kmat, vmat = k5[qb, fr].reshape(-1, H, d), v5[b, fr].reshape(-1, H, d)
            for h in range(H):      # head by head: the [S, n] score matrix of the largest case is 32 MB in fp64
                s = (q5[qb, qi, :, h] @ kmat[:, h].T) * spec.scale
                e = torch.exp(s - s.amax(-1, keepdim=True))
                vh = vmat[:, h]
                ref = (e @ vh) / e.sum(-1, keepdim=True)
                ref_abs = (e @ vh.abs()) / e.sum(-1, keepdim=True)
                for m, trunc in enumerate((False, True)):
                    p = _round16(e, dtype, trunc)
                    den = e.float().sum(-1, keepdim=True, dtype=torch.float32).double() if trunc else p.sum(-1, keepdim=True)
                    tot[m] += float((torch.sign(ref) * ((p @ vh) / den - ref) / ref_abs).sum())
                cnt += ref.numel()
    return tot[0] / cnt, tot[1] / cnt


def signed_error(out32, ref, ref_abs):
    return float((torch.sign(ref) * (out32.double() - ref.double()) / ref_abs.double()).mean())


# ------------------------------------------------------------------------------------------------ the calls under test
def mask(*frames):
    m = 0
    for f in frames:
        m |= 1 << f
    return m


def members(m):
    return [j for j in range(64) if (m >> j) & 1]


K_SETS = 6
# the frame-set tables and shapes of tests/test_frame_sets_gpu.py (kept literal: this module needs no GPU package import)
SET_TABLES = {
    "scattered": [mask(0), mask(1, 3, 5), mask(0, 2, 4), mask(0, 3), mask(1, 2, 4, 5), mask(0, 5)],
    "R1+a0a5": [mask(0, 1, 5), mask(0, 1, 2, 5), mask(0, 1, 2, 3, 5), mask(0, 2, 3, 4, 5), mask(0, 3, 4, 5), mask(0, 4, 5)],
}
WINDOWS_R1 = [(max(0, i - 1), min(K_SETS - 1, i + 1) - max(0, i - 1) + 1) for i in range(K_SETS)]
SET_SHAPES = [      # (S, H, Dh, kwargs, form of the set launch under no_split)
    (48, 2, 40, {}, "fused"),
    (192, 2, 160, {}, "fused"),
    (320, 2, 64, {"fused": False}, "one<64"),
    (512, 2, 40, {"fused": False, "hints": kf.HINT_MIX}, "il<40"),
    (576, 2, 64, {"fused": False}, "il<64"),
    (520, 2, 64, {"fused": False}, "pp<64"),
    (320, 2, 80, {}, "il<80"),
    (128, 2, 160, {"fused": False}, "one<160"),
]
EDIT_SHAPES = [(48, 2, 40, {}), (320, 2, 64, {"fused": False}), (520, 2, 64, {"fused": False}), (320, 2, 80, {})]
MV4_SHAPES = [(45, 2, 40, {"multi_v": True}), (320, 2, 40, {"multi_v": True}), (45, 2, 64, {"multi_v64": True}),
              (320, 2, 64, {"multi_v64": True})]
RUN_SHAPES = [(200, 2, 40, {}), (256, 2, 80, {}), (576, 2, 64, {}), (515, 1, 64, {"no_split": True})]
SEGMENTS = (2, 3)
SEG_SHAPES = [(181, 2, 80, {}), (181, 2, 80, {"fused": False})]


def _table_sets(table):
    if table == "win1":
        return [list(range(lo, lo + n)) for lo, n in WINDOWS_R1]
    return [members(m) for m in SET_TABLES[table]]


class Case:
    """One call under test: `spec`, `modes` (the keyword sets it runs under, e.g. no_split on / off), `call(ops, q, k, v, out,
    **mode)` and `plan(ops, dtype, out_dtype, **mode)` (the launch plan, asserted by `check_plan`)."""

    def __init__(self, name, spec, call, plan, check_plan, modes=({},), seed=0):
        self.name, self.spec, self.call, self.plan, self.check_plan, self.modes, self.seed = name, spec, call, plan, check_plan, modes, seed


def _form_cases():
    for form, cs in kf.CASES.items():
        for i, c in enumerate(cs):
            if "dh" not in c:
                continue
            K, S, H, d = c["K"], c["S"], c["heads"], c["dh"]
            owned = {"all": [0, 1, 2], "bank": [1, 2], "source": [0]}[c["part"]]
            spec = Spec(3, K, S, H, d, inject=c["inject"], owned=owned)

            def call(ops, q, k, v, out, c=c):
                ops.ext_attn(q, k, v, c["heads"], c["dh"] ** -0.5, c["inject"], out=out, part=c["part"], no_split=c["no_split"],
                             fused=c["fused"], hints=c["hints"], fold_scale=c["fold_scale"])

            def plan(ops, dtype, out_dtype, c=c):
                return [kf.form(t) for t in kf.plan(ops, dict(c, dtype=dtype, out_f32=out_dtype == torch.float32))]

            def check(p, dtype, form=form):
                want = form.replace("prec=1", "prec=0") if dtype == torch.float16 else form      # hi + lo P is a bf16 form
                assert want in p, (want, p)
            yield Case(f"form-{form}-{i}", spec, call, plan, check, seed=K * 1000 + S + d)


def _set_cases():
    NS = ({"no_split": False}, {"no_split": True})
    for table in ("scattered", "R1+a0a5", "win1"):
        sets = _table_sets(table)
        for S, H, d, kw, form in SET_SHAPES:
            for inject in (False, True):
                spec = Spec(3, K_SETS, S, H, d, sets=sets, inject=inject)

                def call(ops, q, k, v, out, no_split, table=table, H=H, d=d, kw=kw, inject=inject):
                    if table == "win1":
                        ops.ext_attn_windows(q, k, v, H, d ** -0.5, inject, WINDOWS_R1, no_split=no_split, out=out, **kw)
                    else:
                        ops.ext_attn_frame_sets(q, k, v, H, d ** -0.5, inject, SET_TABLES[table], no_split=no_split, out=out, **kw)

                def plan(ops, dtype, out_dtype, no_split, table=table, S=S, H=H, d=d, kw=kw, inject=inject):
                    if table == "win1":
                        return ops.attn_windows_plan(K_SETS, WINDOWS_R1, S, H, d, inject, dtype=dtype, out_dtype=out_dtype,
                                                     no_split=no_split, **kw)
                    return ops.attn_frame_sets_plan(K_SETS, SET_TABLES[table], S, H, d, inject, dtype=dtype, out_dtype=out_dtype,
                                                    no_split=no_split, **kw)

                def check(p, dtype, no_split, form=form, inject=inject, mark="win" if table == "win1" else "set"):
                    marked = [t for t in p if t.endswith("," + mark) or t.endswith("," + mark + "]")]
                    assert marked, p
                    if no_split:      # (injection at Dh 64, ragged S: the DUAL one-tile form)
                        want = "one<64" if inject and form == "pp<64" else form
                        assert len(marked) == 1 and marked[0].startswith(want), p
                yield Case(f"{table}-S{S}-d{d}-{form.strip('<')}-inj{inject:d}", spec, call, plan, check, NS, seed=S + d)


def _edit_cases():
    E, nbr = 2, 5
    NS = ({"no_split": False}, {"no_split": True})
    variants = [("edits", 3, None), ("set_edits", K_SETS, "scattered"), ("set_edits", K_SETS, "R1+a0a5"), ("win_edits", K_SETS, "win1")]
    shapes = [(s, m, False) for s in EDIT_SHAPES for m in (0b00, 0b11, 0b01)] + [(s, 0b11, True) for s in MV4_SHAPES]
    for op, K, table in variants:
        sets = None if table is None else _table_sets(table)
        for (S, H, d, kw), emask, mv4 in shapes:
            spec = Spec(nbr, K, S, H, d, sets=sets, inject=edit_inject(emask, E))
            kw = dict(kw, fused=False) if mv4 else dict(kw, multi_v=False)

            def call(ops, q, k, v, out, no_split, op=op, table=table, H=H, d=d, kw=kw, emask=emask):
                a = (q, k, v, H, d ** -0.5, False, E)
                if op == "edits":
                    ops.ext_attn_edits(*a, out=out, inject_mask=emask, no_split=no_split, **kw)
                elif op == "win_edits":
                    ops.ext_attn_windows_edits(*a, WINDOWS_R1, inject_mask=emask, no_split=no_split, out=out, **kw)
                else:
                    ops.ext_attn_frame_sets_edits(*a, SET_TABLES[table], inject_mask=emask, no_split=no_split, out=out, **kw)

            def plan(ops, dtype, out_dtype, no_split, op=op, table=table, K=K, S=S, H=H, d=d, kw=kw, emask=emask):
                if op == "edits":
                    return ops.attn_edits_plan(K, K, S, H, d, False, E, dtype=dtype, out_dtype=out_dtype, no_split=no_split,
                                               inject_mask=emask, **kw)
                if op == "win_edits":
                    return ops.attn_windows_edits_plan(K, WINDOWS_R1, S, H, d, E, emask, dtype=dtype, out_dtype=out_dtype,
                                                       no_split=no_split, **kw)
                return ops.attn_frame_sets_edits_plan(K, SET_TABLES[table], S, H, d, E, emask, dtype=dtype, out_dtype=out_dtype,
                                                      no_split=no_split, **kw)

            def check(p, dtype, no_split, mv4=mv4, d=d, mark={"edits": "", "win_edits": ",win", "set_edits": ",set"}[op]):
                assert p, p
                if mv4:
                    token = ("one<40,1,4,MV4,2,fq0>" if d == 40 else "one<64,1,8,MV4,2,fq1>") + mark
                    assert [t for t in p if "MV4" in t] == [token] and p.count("vt_pack") == 1, p
                else:
                    assert not any("MV4" in t for t in p), p
            name = f"{op}{'-' + table if table else ''}-S{S}-d{d}-mask{emask:02b}{'-mv4' if mv4 else ''}"
            yield Case(name, spec, call, plan, check, NS, seed=S + d + emask)


def _run_cases():
    g = rf.BASE
    for S, H, d, kw in RUN_SHAPES:
        for inject in (False, True):
            spec = Spec(3, g["K"], S, H, d, sets=[range(g["K"])] * g["Kq"], inject=inject,
                        qframes=range(g["q_frame0"], g["q_frame0"] + g["Kq"]))

            def call(ops, q, k, v, out, H=H, d=d, kw=kw, inject=inject):
                ops.ext_attn_runs(q, k, v, H, d ** -0.5, inject, g["runs"], q_frame0=g["q_frame0"], out=out, **kw)

            def plan(ops, dtype, out_dtype, S=S, H=H, d=d, kw=kw, inject=inject):
                return [ops.attn_run_plan(g["K"], g["Kq"], n, len(g["runs"]), S, H, d, inject, dtype=dtype, bank_only=r != 0,
                                          out_dtype=out_dtype, **kw) for r, (_f0, n) in enumerate(g["runs"])]

            def check(p, dtype):
                assert len(p) == 3 and all(any(t.endswith(",run>") for t in rp) and rp[-1] == "merge[runs=3]" for rp in p), p
            yield Case(f"runs-S{S}-d{d}-inj{inject:d}{'-ns' if kw else ''}", spec, call, plan, check, seed=S + d)


def _segment_cases():
    K = sum(SEGMENTS)
    sets, f0 = [], 0
    for n in SEGMENTS:
        sets += [list(range(f0, f0 + n))] * n
        f0 += n
    for S, H, d, kw in SEG_SHAPES:
        for inject in (False, True):
            spec = Spec(3, K, S, H, d, sets=sets, inject=inject)

            def call(ops, q, k, v, out, no_split, H=H, d=d, kw=kw, inject=inject):
                ops.ext_attn_segments(q, k, v, H, d ** -0.5, inject, SEGMENTS, out=out, no_split=no_split, **kw)

            def plan(ops, dtype, out_dtype, no_split, S=S, H=H, d=d, kw=kw, inject=inject):
                return ops.attn_segments_plan(K, SEGMENTS, S, H, d, inject, dtype=dtype, out_dtype=out_dtype, no_split=no_split, **kw)

            def check(p, dtype, no_split, kw=kw):
                assert p and (kw or any(t.startswith("fused[") and "sets=2" in t for t in p)), p
            yield Case(f"segments-S{S}-d{d}-inj{inject:d}{'-streaming' if kw else ''}", spec, call, plan, check,
                       ({"no_split": False}, {"no_split": True}), seed=S + d)


FORM_CASES = {c.name: c for c in _form_cases()}
SET_CASES = {c.name: c for c in _set_cases()}
EDIT_CASES = {c.name: c for c in _edit_cases()}
RUN_CASES = {c.name: c for c in _run_cases()}
SEGMENT_CASES = {c.name: c for c in _segment_cases()}
GPU_CASES = {**FORM_CASES, **SET_CASES, **EDIT_CASES, **RUN_CASES, **SEGMENT_CASES}
