"""The NN search on pivots whose row norms differ (tests/nn_families.py; tests/test_nn_norms_cpu.py shows that the
unit-norm pivots of the other oracle comparisons cannot see `inv_norm` at all, and that this family can).

  * every NN form of tests/kernel_forms.py, bf16 and f16, against the fp32 oracle on the spread family: tie-aware equal at
    NN_TAU, indices in [0, S), `ops.pivot_inv_norm` within rtol 1e-5 of 1 / ||row||, fewer than 1 % oracle near-ties among
    the checked rows (precondition).  In the same run: EXACT ties between rows of different norm (the second row of every
    `_tie_pairs` pair is 2 ** j times the first, j in {-3, 1, 2}; its inverse norm must be 2 ** -j times the first's bit
    for bit, the scores are then bit-identical and the first index must win), and, where S is not a multiple of the
    form's pivot tile, a guard behind the ragged tile: the first 256 rows of every keyframe slot behind slot 0 are scaled
    by 2 ** -8 (a cosine does not notice), so the inverse norms stored directly behind a searched keyframe's S entries
    are 256 times larger and a padded copy of row S - 1 that read one of them would win every target with a positive dot
    product with row S - 1;
  * per form family (plain, [split], [chunks]): scaling the pivot rows by 2 ** j, j per row, leaves every index unchanged
    bit for bit on iid targets, near-ties included;
  * per form family: targets whose cosines are ALL negative (the -inf start of the running maximum; a padded row whose
    score were 0 would win);
  * one block through the hooks with a `norm1` that has outlier channels: the pivots' inverse norms from the LayerNorm's
    side output against the stored rows (rtol 2e-6), the indices of the hook's own propagation call against the oracle.
"""
import re

import pytest
import torch

import tokenflow_utils as tfu
from oracle import golden_cases as gc
from oracle import tokenflow_oracle as orc
from tests import fake_diffusers as fd
from tests import kernel_forms as kf
from tests import nn_families as nf
from tests.test_kernel_forms_gpu import (DTYPES, NN_CASES, _check_nn, _plant, _rows_chunk, _rows_single, _sampled,
                                         _tie_pairs)
from tests.test_kernels_gpu import NN_TAU

pytestmark = pytest.mark.gpu

# pivot rows per tile of every kernel family (csrc/nn_search.hip: `tm` of the form descriptions)
PIVOT_TILE = {"rb": 32, "rbs<TJ=2>": 32, "rbs<TJ=4>": 32, "glds": 256, "wide": 128, "bk64": 128, "bk128": 128, "deep": 64}
TIE_EXPONENTS = (-3, 1, 2)
GUARD_ROWS, GUARD_SCALE = 256, 2.0 ** -8
HOOK_SEED = 15          # chosen on the CPU: the pivots' row norms span a ratio of 5.2 (bf16 and f16)


def _ops():
    from tokenflow_amd import ops
    return ops


def _family(token):
    return re.sub(r"\[.*", "", token)


def _kernel_family(ops, c):
    """The family of the search kernel a case launches (its plan's first token; `finalize` follows it)."""
    return _family(kf.plan(ops, c)[0])


def _ragged(ops, c):
    return c["S"] % PIVOT_TILE[_kernel_family(ops, c)] != 0


def _size(c):
    return c["n_tgt"] * c["C"] * c["S"] * c["D"] * c["P"]


def _slots(c):
    """(K, searched slots): C = 1 searches slot 1 (and 0 for P = 2) of three; a run of C chunks searches slots 0 .. C - 1 of
    C + 1, so that every searched keyframe has another one's inverse norms directly behind its own."""
    if c["C"] == 1:
        return 3, ([1, 0] if c["P"] == 2 else [1])
    return c["C"] + 1, list(range(c["C"]))


def _inputs(c, dtype, seed, guard):
    """Spread pivots and iid targets of the case.  Cases checked on every target draw from a CPU generator: the same inputs
    on every machine, so the preconditions (exact scalings, the near-tie cap) were verified on the CPU and cannot depend on
    the GPU's generator.  The largest (sampled) cases draw on the GPU; thousands of their rows are checked."""
    K, _ = _slots(c)
    g = torch.Generator(device="cuda" if _sampled(c) else "cpu").manual_seed(seed)
    piv, gamma, beta = nf.spread_pivots(K, c["S"], c["D"], dtype, g)
    tgt = nf.spread_targets(c["C"] * c["n_tgt"], c["D"], dtype, g, gamma, beta)
    piv, tgt = piv.cuda(), tgt.cuda()
    if guard:
        piv[1:, :GUARD_ROWS] = (piv[1:, :GUARD_ROWS].float() * GUARD_SCALE).to(dtype)
    return piv, tgt


def _scaled_ties(piv, slots):
    """Second row of every `_tie_pairs` pair := 2 ** j times the first, exactly (asserted).  For j < 0 the first row is first
    put on the grid where the scaling is exact (only elements near the f16 subnormal range move).  -> {slot: [(a, b, j)]}"""
    S, dtype = piv.shape[1], piv.dtype
    ties = {}
    for slot in slots:
        ties[slot] = []
        for t, (a, b) in enumerate(_tie_pairs(S)):
            j = TIE_EXPONENTS[t % len(TIE_EXPONENTS)]
            first = piv[slot, a].float()
            if j < 0:
                first = (first * 2.0 ** j).to(dtype).float() * 2.0 ** -j
            dup = (first * 2.0 ** j).to(dtype)
            piv[slot, a] = first.to(dtype)
            piv[slot, b] = dup
            assert torch.equal(piv[slot, a].float(), first) and torch.equal(dup.float(), first * 2.0 ** j)
            ties[slot].append((a, b, j))
    return ties


def _check_inv(ops, piv, ties):
    """tf_pivot_inv_norm against 1 / ||row|| (fp64 of the stored rows), rtol 1e-5; and the scaled duplicates' inverse norms:
    1.0f / sqrtf(s) is exact under a scaling of s by 4 ** j."""
    inv = ops.pivot_inv_norm(piv)
    ref = 1.0 / piv.double().norm(dim=-1)
    rel = ((inv.double() - ref).abs() / ref).max()
    assert float(rel) <= 1e-5, f"pivot_inv_norm: relative error {float(rel):.3e}"
    for slot, pairs in ties.items():
        for a, b, j in pairs:
            want = inv[slot, a] * 2.0 ** -j
            assert torch.equal(inv[slot, b], want), \
                f"slot {slot}: inv_norm of row {b} (= 2^{j} * row {a}) is {float(inv[slot, b])!r}, not {float(want)!r}"
    return inv


def _search(ops, c, piv, tgt, inv):
    """The case's search: C = 1 -> ops.nn_search [P, n_tgt]; C > 1 -> ops.propagate_chunks (first_single), the indices read
    back through an index-coded keyframe cache (row j of every slot holds j; w = 1 selects the first keyframe's index,
    w = 0 the second's) -> [2, C, n_tgt]."""
    K, slots = _slots(c)
    n_tgt, S, D, C = c["n_tgt"], c["S"], c["D"], c["C"]
    if C == 1:
        return ops.nn_search(tgt, piv, inv, slots).long()
    n = n_tgt // S
    kf_out = torch.arange(S, dtype=torch.float32, device="cuda").view(1, S, 1).expand(3 * K, S, D).contiguous()
    res = []
    for wv in (1.0, 0.0):
        w = torch.full((n,), wv, device="cuda")
        out = ops.propagate_chunks(tgt, piv, inv, kf_out, w, n, C, 0, True, None, torch.float32)
        res.append(out.view(3, C, n_tgt, D)[0, :, :, 0].round().long())
    return torch.stack(res)


def _near_ties(sim, dups):
    """(rows whose oracle top-2 gap is <= NN_TAU, smallest gap), the exact duplicates apart: they tie by construction and the
    planted targets pin their order."""
    s = sim.clone()
    if dups:
        s[:, dups] = -float("inf")
    return nf.near_tie_rows(s, NN_TAU)


def _check_case(c, res, tgt, piv, ties, plants, what, negative=False):
    """Every searched (chunk, slot) of the case against the fp32 oracle, then the precondition that keeps the tie-aware
    comparison honest: fewer than 1 % of the checked rows are oracle near-ties.
    plants: {chunk: {position among the planted targets at the chunk's end: index}}"""
    _, slots = _slots(c)
    n_tgt, C = c["n_tgt"], c["C"]
    sampled = _sampled(c)
    seen = []

    def one(got, rows, slot, planted, tag):
        sim = _check_nn(got, tgt, piv, slot, rows.cuda(), planted)
        if negative:
            assert float(sim.max()) < 0, f"{tag}: precondition, every cosine negative (max {float(sim.max()):.3e})"
        seen.append((len(rows),) + _near_ties(sim, [b for _a, b, _j in ties.get(slot, [])]))

    if C == 1:
        rows = _rows_single(n_tgt, sampled)
        for p, slot in enumerate(slots):
            pl = {len(rows) - len(plants[0]) + t: a for t, a in plants[0].items()} if p == 0 and plants else {}
            one(res[p][rows.cuda()], rows, slot, pl, f"{what} slot {slot}")
    for j in range(C if C > 1 else 0):
        rows = _rows_chunk(j, n_tgt, sampled)
        loc = (rows - j * n_tgt).cuda()
        for w_i, slot in ((0, j), (1, j - 1)):
            if slot < 0:
                continue          # chunk 0 of the video: one keyframe
            pl = {len(rows) - len(plants[j]) + t: a for t, a in plants[j].items()} if w_i == 0 and plants else {}
            one(res[w_i][j][loc], rows, slot, pl, f"{what} chunk {j} slot {slot}")
    n_rows, n_ties, min_gap = sum(r for r, _, _ in seen), sum(t for _, t, _ in seen), min(g_ for _, _, g_ in seen)
    print(f"{what}: {n_rows} rows checked, {n_ties} oracle near-ties (min top-2 gap {min_gap:.1e})")
    assert n_ties < 0.01 * n_rows, f"{what}: {n_ties} oracle near-ties among {n_rows} checked rows"


# ------------------------------------------------------------------ every form against the oracle
@pytest.mark.parametrize("form,i", NN_CASES, ids=[f"{f}-{i}" for f, i in NN_CASES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nn_form_vs_oracle_on_spread_norms(form, i, dtype):
    ops = _ops()
    c = kf.CASES[form][i]
    assert form in [kf.form(t) for t in kf.plan(ops, c)]
    n_tgt, S, C = c["n_tgt"], c["S"], c["C"]
    _, slots = _slots(c)
    guard = _ragged(ops, c)
    piv, tgt = _inputs(c, dtype, seed=n_tgt + S + c["D"] + C, guard=guard)
    ties = _scaled_ties(piv, slots)
    npl = len(_tie_pairs(S))
    if C == 1:      # the planted targets sit in the ragged last target panel, where there is one
        plants = {0: _plant(tgt, piv, slots[0], n_tgt - npl, S)}
    else:           # chunk j matches slot j first: its planted targets at the end of the chunk
        plants = {j: _plant(tgt, piv, j, (j + 1) * n_tgt - npl, S) for j in range(C)}
    inv = _check_inv(ops, piv, ties)
    if guard:       # what sits behind a searched keyframe's S inverse norms is 256 times larger than it would be
        ref = 1.0 / (piv[1:, :GUARD_ROWS].double() / GUARD_SCALE).norm(dim=-1)
        assert bool((inv[1:, :GUARD_ROWS].double() > 200.0 * ref).all())
    res = _search(ops, c, piv, tgt, inv)
    _check_case(c, res, tgt, piv, ties, plants, f"{form} case {i} {dtype} guard={guard}")


def test_every_nn_form_and_family_is_covered():
    """A form added to the table cannot skip the family: the parametrisation above is the table's, every family has its pivot
    tile here, and the per-family tests below cover every family."""
    nn_forms = {f for f, cs in kf.CASES.items() if any("n_tgt" in c for c in cs)}
    assert {f for f, _ in NN_CASES} == nn_forms
    assert all(len([1 for f_, _ in NN_CASES if f_ == f]) == len(kf.CASES[f]) for f in nn_forms)
    fams = {_family(f) for f in nn_forms} - {"finalize"}
    assert fams == set(PIVOT_TILE)
    assert {_family(f) for f in SCALING_FORMS} == fams and {f for f, _ in NEGATIVE_CASES} == fams


# ------------------------------------------------------------------ bit-exact scaling invariance
def _smallest(form):
    return min(kf.CASES[form], key=_size)


SCALING_FORMS = [fam + v for fam in PIVOT_TILE for v in ("", "[split]", "[chunks]") if fam + v in kf.CASES]


@pytest.mark.parametrize("form", SCALING_FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_scaling_pivot_rows_by_powers_of_two_changes_no_index(form, dtype):
    ops = _ops()
    c = _smallest(form)
    assert form in [kf.form(t) for t in kf.plan(ops, c)]
    piv, tgt = _inputs(c, dtype, seed=_size(c) % 9973, guard=False)
    piv = ((piv.float() * 2.0 ** -3).to(dtype).float() * 2.0 ** 3).to(dtype)     # the grid on which 2 ** -3 is exact
    g = torch.Generator(device="cuda").manual_seed(7)
    j = torch.randint(-3, 4, (piv.shape[0], piv.shape[1], 1), generator=g, device="cuda").float()
    scaled = (piv.float() * torch.exp2(j)).to(dtype)
    assert torch.equal(scaled.float(), piv.float() * torch.exp2(j)), "precondition: the scaling is exact in the dtype"
    inv, inv_s = ops.pivot_inv_norm(piv), ops.pivot_inv_norm(scaled)
    assert torch.equal(inv_s, inv * torch.exp2(-j[..., 0])), "inv_norm is not exactly covariant with a 2 ** j row scale"
    base = _search(ops, c, piv, tgt, inv)
    got = _search(ops, c, scaled, tgt, inv_s)
    assert int(base.min()) >= 0 and int(base.max()) < c["S"]
    n_diff = int((base != got).sum())
    assert n_diff == 0, f"{form} {dtype}: {n_diff} of {base.numel()} indices change under a 2 ** j scaling of the pivot rows"


# ------------------------------------------------------------------ negative cosines
def _negative_case(fam):
    """The smallest case of the family whose last pivot tile is ragged (a padded row must not win), else the smallest."""
    cases = [c for f, cs in kf.CASES.items() if _family(f) == fam for c in cs]
    ragged = [c for c in cases if c["S"] % PIVOT_TILE[fam]]
    return min(ragged or cases, key=_size)


NEGATIVE_CASES = [(fam, _negative_case(fam)) for fam in PIVOT_TILE]


@pytest.mark.parametrize("fam,c", NEGATIVE_CASES, ids=[f for f, _ in NEGATIVE_CASES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_cosines_negative(fam, c, dtype):
    """Pivots |y| (every element >= 0), targets -|y'|: every cosine is negative, the oracle's index is the least negative
    one.  The running maximum starts at -inf, and a padded copy of row S - 1 never scores above the real rows."""
    ops = _ops()
    assert _kernel_family(ops, c) == fam
    guard = _ragged(ops, c)
    piv, tgt = _inputs(c, dtype, seed=_size(c) % 9973 + 3, guard=guard)      # seeds verified on the CPU (near-tie cap)
    piv, tgt = piv.abs(), -tgt.abs()
    inv = _check_inv(ops, piv, {})
    res = _search(ops, c, piv, tgt, inv)
    _check_case(c, res, tgt, piv, {}, {}, f"{fam} negative {dtype}", negative=True)


# ------------------------------------------------------------------ the hooks, with a norm1 that has outlier channels
@pytest.mark.parametrize("fp32_as", DTYPES)
def test_hooks_norm1_with_outlier_channels(monkeypatch, fp32_as):
    """One block: the pivotal pass, then the pass of chunk 1 (K = 3, n = 2, S = 48).  norm1 has gains 1 + 0.3 * randn with four
    channels 16 times larger and a bias 0.3 * randn, as a trained SD block has outlier channels: the stored pivots' row norms
    span a ratio >= 4.  In the hook's own propagation call: the inverse norms (norm1's side output) against the STORED rows,
    and the indices (decoded through an index-coded cache) against the oracle."""
    ops = _ops()
    monkeypatch.setattr(ops, "FP32_AS", fp32_as)
    K, n, S, bi = 3, 2, 48, 1
    cfg = gc.BLOCKS_CFG
    torch.manual_seed(cfg["seed"])
    pipe = fd.FakePipeline(dims=cfg["dims"], heads=cfg["heads"], cross_dim=cfg["cross_dim"]).eval()
    blk = pipe.unet.up_blocks[2].attentions[0].transformer_blocks[0]
    D = blk.norm1.normalized_shape[0]
    g = torch.Generator().manual_seed(HOOK_SEED)
    with torch.no_grad():
        gain = 1.0 + 0.3 * torch.randn(D, generator=g)
        gain[torch.randperm(D, generator=g)[:4]] *= 16.0
        blk.norm1.weight.copy_(gain)
        blk.norm1.bias.copy_(0.3 * torch.randn(D, generator=g))
    pipe = pipe.cuda()
    tfu.register_extended_attention_pnp(pipe, [801])
    tfu.set_tokenflow(pipe.unet)
    tfu.register_time(pipe, 801)
    x_piv, enc_piv = torch.randn(3 * K, S, D, generator=g).cuda(), torch.randn(3 * K, 7, cfg["cross_dim"], generator=g).cuda()
    # video-like source branch of the chunk: permuted tokens of keyframe 1 plus noise
    src = x_piv.view(3, K, S, D)[0, bi][torch.randperm(S, generator=g).cuda()][None].repeat(n, 1, 1)
    src = src + 0.3 * torch.randn(n, S, D, generator=g).cuda()
    x_ch = torch.cat([src, torch.randn(2 * n, S, D, generator=g).cuda()])
    enc_ch = torch.randn(3 * n, 7, cfg["cross_dim"], generator=g).cuda()
    seen = []
    real = ops.propagate

    def spy(tgt, piv, inv, kf_ids, kf_out, w, n_, residual, out_dtype, norm=None):
        assert piv.dtype == fp32_as and piv.shape == (K, S, D) and list(kf_ids) == [bi, bi - 1]
        pc = piv.float().cpu()
        norms = pc.norm(dim=-1)
        ratio = float(norms.max() / norms.min())
        assert ratio >= 4.0, f"precondition: row norms of the pivots span a ratio of {ratio:.2f}"
        ref = 1.0 / piv.double().norm(dim=-1)
        rel = float(((inv.double() - ref).abs() / ref).max())
        assert rel <= 2e-6, f"inverse norms of the stored pivots: relative error {rel:.3e}"
        code = torch.zeros(3, K, S, D, dtype=torch.float32, device="cuda")
        rows = torch.arange(S, dtype=torch.float32, device="cuda")
        code[:, kf_ids[0], :, 0] = rows
        code[:, kf_ids[1], :, 1] = rows
        out = real(tgt, piv, inv, kf_ids, code.view(3 * K, S, D), w, n_, None, torch.float32).view(3, n_, S, D)
        got = [(out[0, :, :, 0] / w.view(n_, 1)).reshape(-1).round().long().cpu(),
               (out[0, :, :, 1] / (1 - w).view(n_, 1)).reshape(-1).round().long().cpu()]
        ref_idx, sim = orc.nn_search(tgt.float().cpu().view(n_, S, D), pc, bi)
        n_diff = 0
        for r, s, g_ in zip(ref_idx, sim.chunk(2, dim=1), got):
            assert int(g_.min()) >= 0 and int(g_.max()) < S
            diff, bad = orc.nn_mismatch_tie_aware(s, r, g_, NN_TAU)
            assert bad == 0, f"{bad} of {n_ * S} rows differ from the oracle beyond a near-tie"
            n_diff += diff
        seen.append((ratio, rel, n_diff))
        return real(tgt, piv, inv, kf_ids, kf_out, w, n_, residual, out_dtype, norm=norm)
    monkeypatch.setattr(ops, "propagate", spy)

    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        blk(x_piv, encoder_hidden_states=enc_piv)
        tfu.register_pivotal(pipe, False)
        tfu.register_batch_idx(pipe, bi)
        out = blk(x_ch, encoder_hidden_states=enc_ch)
    assert len(seen) == 1 and torch.isfinite(out.float()).all()
    print(f"hooks {fp32_as}: pivot norm ratio {seen[0][0]:.2f}, inv_norm rel err {seen[0][1]:.2e}, "
          f"{seen[0][2]} indices differ from the oracle (all within a near-tie)")

