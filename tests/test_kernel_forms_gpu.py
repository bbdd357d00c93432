"""Every kernel form the attention and NN-search dispatchers can pick (tests/kernel_forms.py), each run on a case whose
launch plan is asserted first (ops.attn_plan / ops.nn_plan: the library's own record of the launches), then checked
against a plain reference:

  * attention: the CPU oracle (oracle.ext_attn_core) under the bound of tests/test_kernels_gpu.py, on N(0,1) inputs,
    on peaked ones (planted keys of gain 12 in late tiles: the deferred shift moves, O is rescaled) and, for the forms
    with the Cauchy-Schwarz score bound (Dh = 40 / 64), on a strongly negative first tile; bf16 and f16;
  * the mixed-MFMA-shape form (Dh = 40, DMA 3) on its own set: one-pass / split / source-beside-dual-V against the
    oracle, the fp32 output, the bank / source parts, strided views and query-frame subsets bit for bit, and one
    unhinted launch of >= 1024 workgroups against an fp64 reference computed on the GPU;
  * NN search: every (or, for the largest launches, every sampled) target against the fp32 oracle, tie-aware
    (NN_TAU), exact-duplicate pivot pairs at every merge distance the kernels have (one lane's rows, the lanes of a
    tile, pivot tiles, splits -- the first index must win), one keyframe of identical rows (every index 0).
"""
import pytest
import torch

from oracle import tokenflow_oracle as orc
from tests import kernel_forms as kf
from tests.test_kernels_gpu import NN_TAU, assert_attn_close, attn_bound, attn_ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _ops():
    from tokenflow_amd import ops
    return ops


def _rnd(dtype):
    return orc.bf16_round if dtype == torch.bfloat16 else (lambda x: x.half().float())


def _attn_inputs(K, S, D, h, kind, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(3 * K, S, D, generator=g) for _ in range(3))
    if kind == "peaked":      # planted keys aligned with their queries, many of them in the last 64-key tile of a frame
        s_ = torch.arange(0, S, 5)
        k[:, (s_ * 3 + S - 60) % S] = q[:, s_] * 12.0
    elif kind == "negfirst":  # every score of the first 64-key tile ~ -110 (exp2 of the shift difference overflows fp32)
        d = D // h
        u = torch.nn.functional.normalize(torch.randn(h, d, generator=g), dim=-1)
        amp = (110.0 * d ** 0.5) ** 0.5
        q = (amp * u.view(1, 1, h, d) + 0.05 * q.view(3 * K, S, h, d)).reshape(3 * K, S, D)
        kv = k.view(3 * K, S, h, d)
        kv[:, :64] = -amp * u.view(1, 1, h, d) + 0.05 * kv[:, :64]
    return q, k, v


def _branches(part):
    return {"all": [0, 1, 2], "bank": [1, 2], "source": [0]}[part]


ATTN_CASES = [(f, i) for f, cs in kf.CASES.items() for i, c in enumerate(cs) if "dh" in c]
NN_CASES = [(f, i) for f, cs in kf.CASES.items() for i, c in enumerate(cs) if "n_tgt" in c]


@pytest.mark.parametrize("form,i", ATTN_CASES, ids=[f"{f}-{i}" for f, i in ATTN_CASES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_form_vs_oracle(form, i, dtype):
    ops = _ops()
    c = dict(kf.CASES[form][i])
    want = form.replace("prec=1", "prec=0") if dtype == torch.float16 else form   # hi + lo P is a bf16 form
    assert want in [kf.form(t) for t in kf.plan(ops, dict(c, dtype=dtype))]
    K, Kq, S, h, d = c["K"], c["Kq"], c["S"], c["heads"], c["dh"]
    assert Kq == K
    kinds = ["randn", "peaked"] + (["negfirst"] if d in (40, 64) and S >= 128 else [])
    for kind in kinds:
        q, k, v = (_rnd(dtype)(x) for x in _attn_inputs(K, S, h * d, h, kind, seed=K * 1000 + S + d + len(kind)))
        refs = attn_ref(q, k, v, h, d ** -0.5, c["inject"], need_sigma=c["fold_scale"])
        out = torch.zeros(3 * K, S, h * d, dtype=dtype, device="cuda")
        ops.ext_attn(q.to(dtype).cuda(), k.to(dtype).cuda(), v.to(dtype).cuda(), h, d ** -0.5, c["inject"], out=out,
                     part=c["part"], no_split=c["no_split"], fused=c["fused"], hints=c["hints"],
                     fold_scale=c["fold_scale"])
        br = _branches(c["part"])
        o = out.view(3, K, S, -1)[br].reshape(-1, S, h * d)
        sel = [r.view(3, K, S, -1)[br].reshape(-1, S, h * d) if r is not None else None for r in refs]
        assert torch.isfinite(o.float()).all(), f"{form} {kind}"
        assert_attn_close(o, sel, f"{form} case {i} {kind} {dtype}", dtype=dtype, folded=c["fold_scale"])


# ------------------------------------------------------------------ the mixed-MFMA-shape form (Dh = 40, DMA 3)
MIX_SHAPES = [(4, 1024, 8), (2, 256, 2)]


def _mix_plan(ops, K, S, h, inject, no_split, **kw):
    p = ops.attn_plan(K, K, S, h, 40, inject, no_split=no_split, fused=False, hints=kf.HINT_MIX, **kw)
    assert ("il<40,8,SOURCE,4,3>" if inject else "il<40,8,ALL,4,3>") in p, p
    return p


@pytest.mark.parametrize("K,S,h", MIX_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["randn", "peaked"])
def test_mixed_form_vs_oracle(K, S, h, dtype, kind):
    """One-pass and split MODE_ALL; under injection MODE_SOURCE beside the dual-V kernel."""
    ops = _ops()
    d = 40
    q, k, v = (_rnd(dtype)(x) for x in _attn_inputs(K, S, h * d, h, kind, seed=7 * S + K))
    dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
    for inject in (False, True):
        refs = attn_ref(q, k, v, h, d ** -0.5, inject, need_sigma=False)
        for no_split in (True, False):
            _mix_plan(ops, K, S, h, inject, no_split, dtype=dtype)
            out = ops.ext_attn(dq, dk, dv, h, d ** -0.5, inject, fused=False, no_split=no_split, hints=kf.HINT_MIX)
            assert torch.isfinite(out.float()).all()
            assert_attn_close(out, refs, f"mixed K{K} S{S} {kind} {dtype} inject={inject} no_split={no_split}", dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_form_fp32_output(dtype):
    """TF_ATTN_OUT_F32 in the mixed form: within 1e-3 of the oracle at S >= 576, and the 16-bit call is exactly its
    rounding."""
    ops = _ops()
    K, S, h, d = 2, 576, 2, 40
    q, k, v = (_rnd(dtype)(x) for x in _attn_inputs(K, S, h * d, h, "randn", seed=99))
    dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
    for inject in (False, True):
        ref = attn_ref(q, k, v, h, d ** -0.5, inject, need_sigma=False)[0]
        for no_split in (True, False):
            _mix_plan(ops, K, S, h, inject, no_split, dtype=dtype, out_dtype=torch.float32)
            o32 = ops.ext_attn(dq, dk, dv, h, d ** -0.5, inject, fused=False, no_split=no_split, hints=kf.HINT_MIX,
                               out_dtype=torch.float32)
            out = ops.ext_attn(dq, dk, dv, h, d ** -0.5, inject, fused=False, no_split=no_split, hints=kf.HINT_MIX)
            assert float((o32.cpu() - ref).abs().max()) < 1e-3
            assert torch.equal(o32.to(dtype), out)


@pytest.mark.parametrize("inject", [False, True])
def test_mixed_form_parts_views_and_query_subsets(inject):
    """part="bank" + part="source" reproduce the full call, strided views equal the dense call, and a q_frame0 subset
    (one-pass: the kernel choice is then a function of the shape) equals the matching slice -- all bit for bit."""
    ops = _ops()
    K, S, h, d = 4, 1024, 8, 40
    D = h * d
    g = torch.Generator(device="cuda").manual_seed(5)
    qkv = torch.randn(3 * K, S, 3 * D, generator=g, device="cuda").bfloat16()
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    for no_split in (True, False):
        kw = dict(fused=False, no_split=no_split, hints=kf.HINT_MIX)
        _mix_plan(ops, K, S, h, inject, no_split)
        full = ops.ext_attn(q.contiguous(), k.contiguous(), v.contiguous(), h, d ** -0.5, inject, **kw)
        out = torch.full_like(full, 7.0)
        ops.ext_attn(q, k, v, h, d ** -0.5, inject, out=out, part="bank", **kw)
        ops.ext_attn(q, k, v, h, d ** -0.5, inject, out=out, part="source", **kw)
        assert torch.equal(out, full)
        assert "il<40,8,SOURCE,4,3>" in ops.attn_plan(K, K, S, h, d, inject, part="source", **kw)
        # strided 4-D views of the fused projection (token stride 3D)
        vo = torch.empty(3, K, S, D, dtype=torch.bfloat16, device="cuda")
        ops.ext_attn_views(q.view(3, K, S, D), k.view(3, K, S, D), v.view(3, K, S, D), vo, h, d ** -0.5, inject,
                           **kw)
        assert torch.equal(vo.view(3 * K, S, D), full)
        if no_split:
            for f0, nq in ((1, 2), (3, 1)):
                assert ("il<40,8,SOURCE,4,3>" if inject else "il<40,8,ALL,4,3>") in ops.attn_plan(K, nq, S, h, d, inject,
                                                                                                  **kw)
                qs = q.view(3, K, S, D)[:, f0:f0 + nq].reshape(3 * nq, S, D)
                sub = ops.ext_attn(qs, k.contiguous(), v.contiguous(), h, d ** -0.5, inject, q_frame0=f0, **kw)
                assert torch.equal(sub.view(3, nq, S, D), full.view(3, K, S, D)[:, f0:f0 + nq])


def test_mixed_form_is_the_default_of_large_launches_fp64():
    """An unhinted launch of >= 1024 eight-wave workgroups (K = 8, S = 2048, 8 heads: 3 * 8 * 8 * 8 = 1536) takes the
    mixed form by default; every row on peaked inputs against an fp64 reference computed on the GPU (plain matmul +
    softmax in double, frame by frame)."""
    ops = _ops()
    K, S, h, d = 8, 2048, 8, 40
    D = h * d
    assert ops.attn_plan(K, K, S, h, d, False, no_split=False, fused=None) == ["vt_pack", "il<40,8,ALL,4,3>"]
    q, k, v = (orc.bf16_round(x) for x in _attn_inputs(K, S, D, h, "peaked", seed=2048))
    dq, dk, dv = (t.bfloat16().cuda() for t in (q, k, v))
    out = ops.ext_attn(dq, dk, dv, h, d ** -0.5, False, no_split=False, fused=None).view(3, K, S, h, d)
    q4, k4, v4 = (t.cuda().double().view(3, K, S, h, d) for t in (q, k, v))
    worst = -1.0
    for b in range(3):
        keys = k4[b] if b == 0 else k4[b].reshape(1, K * S, h, d).expand(K, K * S, h, d)
        vals = v4[b] if b == 0 else v4[b].reshape(1, K * S, h, d).expand(K, K * S, h, d)
        for f in range(K):
            p = torch.softmax(torch.einsum("qhc,khc->hqk", q4[b, f], keys[f]) * d ** -0.5, dim=-1)
            ref = torch.einsum("hqk,khc->qhc", p, vals[f])
            ref_abs = torch.einsum("hqk,khc->qhc", p, vals[f].abs())
            err = (out[b, f].double() - ref).abs()
            worst = max(worst, float((err - attn_bound(ref, ref_abs)).max()))
    assert worst <= 0, f"exceeds the bound by {worst:.3e}"


# ------------------------------------------------------------------ NN search
def _tie_pairs(S):
    """(first, duplicate) pivot pairs: adjacent rows (one lane's rows / neighbouring lanes), 8 / 16 / 32 apart (the lanes
    of the __shfl_xor merge, a 32-pivot tile), 64 / 128 / 256 apart (pivot tiles of every form), across the middle and
    across the whole range (different splits whenever the range is split)."""
    pairs = []
    for a, dist in ((1, 1), (3, 8), (4, 16), (9, 32), (12, 64), (17, 128), (21, 256), (S // 2 - 1, 1), (6, S - 2)):
        if a + dist < S and a > 0:
            pairs.append((a, a + dist))
    used = set()
    return [(a, b) for a, b in pairs if not (a in used or b in used or used.update((a, b)))]


def _nn_inputs(K, n_all, S, D, dtype, seed, same_slot):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ln = torch.nn.functional.layer_norm
    piv = ln(torch.randn(K, S, D, generator=g, device="cuda"), (D,))
    for a, b in _tie_pairs(S):
        piv[:, b] = piv[:, a]
    if same_slot is not None:
        piv[same_slot] = piv[same_slot, 0:1]          # a keyframe of identical rows: every index 0
    tgt = ln(torch.randn(n_all, D, generator=g, device="cuda"), (D,))
    return piv.to(dtype), tgt.to(dtype)


def _check_nn(idx, tgt, piv, slot, rows, planted):
    """idx [rows] for targets `rows` against keyframe `slot`: tie-aware against the fp32 oracle; planted rows exact.
    Returns the oracle's similarity matrix of the checked rows."""
    t = tgt[rows].float().cpu()
    sim = orc.batch_cosine_sim(t, piv[slot].float().cpu())
    got = idx.cpu().long()
    assert int(got.min()) >= 0 and int(got.max()) < piv.shape[1]
    diff, bad = orc.nn_mismatch_tie_aware(sim, sim.argmax(-1), got, NN_TAU)
    assert bad == 0, f"slot {slot}: {bad} of {len(rows)} rows differ beyond a near-tie ({diff} differ at all)"
    for r, want in planted.items():
        assert int(got[r]) == want, f"slot {slot}: planted target {r} -> {int(got[r])}, the first index is {want}"
    return sim


def _sampled(c):
    """The largest launches are checked on sampled targets (the oracle's similarity matrix is on the CPU)."""
    return c["n_tgt"] * c["C"] * c["S"] * c["D"] * c["P"] > 4e10


def _rows_single(n_tgt, sampled):
    """The checked targets of a C = 1 case: all of them, or 2048 random ones and the last 512 (ragged panel, planted rows)."""
    if not sampled:
        return torch.arange(n_tgt)
    return torch.cat([torch.randint(0, n_tgt - 512, (2048,), generator=torch.Generator().manual_seed(1)),
                      torch.arange(n_tgt - 512, n_tgt)])


def _rows_chunk(j, n_tgt, sampled):
    """The checked targets of chunk j of a C > 1 case: all of them, or 512 random ones and the last 512."""
    if not sampled:
        return torch.arange(j * n_tgt, (j + 1) * n_tgt)
    return torch.cat([torch.randint(j * n_tgt, (j + 1) * n_tgt - 512, (512,), generator=torch.Generator().manual_seed(j)),
                      torch.arange((j + 1) * n_tgt - 512, (j + 1) * n_tgt)])


def _plant(tgt, piv, slot, rows_base, S):
    """Targets equal to the first row of each duplicate pair of keyframe `slot` -> {position in the checked rows: index}."""
    planted = {}
    for j, (a, _b) in enumerate(_tie_pairs(S)):
        tgt[rows_base + j] = piv[slot, a]
        planted[j] = a
    return planted


@pytest.mark.parametrize("form,i", NN_CASES, ids=[f"{f}-{i}" for f, i in NN_CASES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nn_form_vs_oracle(form, i, dtype):
    ops = _ops()
    c = kf.CASES[form][i]
    assert form in [kf.form(t) for t in kf.plan(ops, c)]
    n_tgt, S, D, P, C = c["n_tgt"], c["S"], c["D"], c["P"], c["C"]
    sampled = _sampled(c)
    npl = len(_tie_pairs(S))
    if C == 1:
        K = 2
        piv, tgt = _nn_inputs(K, n_tgt, S, D, dtype, seed=n_tgt + S + D, same_slot=0)
        ids = [1, 0] if P == 2 else [1]
        planted = _plant(tgt, piv, 1, n_tgt - npl, S)          # the ragged last target panel, where there is one
        idx = ops.nn_search(tgt, piv, ops.pivot_inv_norm(piv), ids)
        rows = _rows_single(n_tgt, sampled)
        base = len(rows) - npl
        _check_nn(idx[0][rows.cuda()], tgt, piv, 1, rows.cuda(), {base + j: a for j, a in planted.items()})
        if P == 2:
            assert bool((idx[1] == 0).all()), "identical keyframe: every index must be 0"
        else:
            idx0 = ops.nn_search(tgt, piv, ops.pivot_inv_norm(piv), [0])
            assert bool((idx0 == 0).all()), "identical keyframe: every index must be 0"
        return
    # C > 1: tf_nn_gather_blend_chunks (first_single); the indices are read back through the gather: kf_out row j of
    # every slot holds the value j, w = 1 selects the first keyframe's index, w = 0 the second's
    K, n, same = C, n_tgt // S, C - 2
    piv, tgt = _nn_inputs(K, C * n_tgt, S, D, dtype, seed=n_tgt + S + D + C, same_slot=same)
    # chunk j matches slot j first (its planted targets at the end of the chunk), then slot j - 1
    plants = {j: _plant(tgt, piv, j, (j + 1) * n_tgt - npl, S) for j in range(C) if j != same}
    inv = ops.pivot_inv_norm(piv)
    kf_out = torch.arange(S, dtype=torch.float32, device="cuda").view(1, S, 1).expand(3 * K, S, D).contiguous()
    res = {}
    for wv in (1.0, 0.0):
        w = torch.full((n,), wv, device="cuda")
        out = ops.propagate_chunks(tgt, piv, inv, kf_out, w, n, C, 0, True, None, torch.float32)
        res[wv] = out.view(3, C, n_tgt, D)[0, :, :, 0].round().long()
    for j in range(C):
        rows = _rows_chunk(j, n_tgt, sampled)
        loc = (rows - j * n_tgt).cuda()
        base = len(rows) - npl
        for wv, slot in ((1.0, j), (0.0, j - 1)):
            if slot < 0:
                continue          # chunk 0 of the video: one keyframe
            if slot == same:
                assert bool((res[wv][j] == 0).all()), f"chunk {j}: identical keyframe, every index must be 0"
            else:
                pl = {base + t: a for t, a in plants[j].items()} if wv == 1.0 else {}
                _check_nn(res[wv][j][loc], tgt, piv, slot, rows.cuda(), pl)
