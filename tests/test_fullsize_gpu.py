"""Parity at BASELINE.json's full sizes (cfg2: 40 frames, 512x512, SD1.5, K=8 keyframes, n=5;
cfg4 geometry for the NN search) through size-independent properties and oracle checks on
sampled rows -- the full score matrices the oracle would need do not fit anywhere
(4 GiB per head and branch at cfg2 level 0).  Needs an MI355X.

Stated tolerance for the attention at these shapes: per-token deviation < 1e-3 (north star),
inputs N(0,1) rounded to bf16, oracle fed the same rounded values -- except where the bf16
OUTPUT format itself cannot represent the reference to 1e-3: bf16 has 8 significand bits, so an
output of magnitude |o| carries a rounding error up to 2^-8*|o| (> 1e-3 once |o| > 0.256; this
happens on the short source-branch problems of the 16x16 level, S = 256 keys, where the
probabilities are also few enough that their own bf16 rounding does not average out).  The
asserted bound is therefore, per element,
    |out - ref| < max(1e-3, 2e-4 + 2^-8*|ref| + 2^-8*(softmax . |V|))
(the second argument is the bound of tests/test_kernels_gpu.py), and plain 1e-3 on the two
levels that carry 97 % of the work."""
import pytest
import torch

from oracle import tokenflow_oracle as orc

pytestmark = pytest.mark.gpu


def _ops():
    from tokenflow_amd import ops
    return ops


def _oracle_rows(q, k, v, K, S, h, d, b, f, head, rows, inject):
    """fp32 oracle for a few query rows of one (branch, frame, head): tokenflow_utils.py:173-179."""
    D = h * d
    qv, kv, vv = (t.view(3, K, S, h, d) for t in (q, k, v))
    bq = 0 if (inject and b > 0) else b
    qr = qv[bq, f, rows, head].float()                                   # [R, d]
    if b == 0:
        kk, vals = kv[0, f, :, head].float(), vv[0, f, :, head].float()  # own S keys
    else:
        kk, vals = kv[bq, :, :, head].reshape(K * S, d).float(), vv[b, :, :, head].reshape(K * S, d).float()
    p = torch.softmax(qr @ kk.T * d ** -0.5, dim=-1)
    return p @ vals, p @ vals.abs()                                      # [R, d] each


@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("inject", [False, True])
def test_ext_attn_cfg2_sampled_rows(level, inject):
    """BASELINE config 2 at full size, every level: north_star's "max per-token deviation < 1e-3" as the PLAIN number on
    the fp32 output (TF_ATTN_OUT_F32) -- no clamp, no relative term -- and, on the bf16 output, that plus what any bf16
    tensor is off by: half an ulp of the reference value."""
    ops = _ops()
    K, h = 8, 8
    S, D = [(4096, 320), (1024, 640), (256, 1280), (64, 1280)][level]
    d = D // h
    g = torch.Generator(device="cuda").manual_seed(100 + level)
    q, k, v = (torch.randn(3 * K, S, D, generator=g, device="cuda").bfloat16() for _ in range(3))
    out = ops.ext_attn(q, k, v, h, d ** -0.5, inject)
    out32 = ops.ext_attn(q, k, v, h, d ** -0.5, inject, out_dtype=torch.float32)
    torch.cuda.synchronize()
    qc, kc, vc = q.cpu(), k.cpu(), v.cpu()
    oc, oc32 = out.float().cpu().view(3, K, S, h, d), out32.cpu().view(3, K, S, h, d)
    rows = torch.tensor(sorted({0, 1, 31, 32, 63, min(64, S - 1), min(127, S - 1), min(128, S - 1), S // 2 + 5,
                                max(S - 129, 0), S - 2, S - 1}))
    worst32, worst16_excess = 0.0, -1.0
    for b, f, head in [(0, 0, 0), (0, K - 1, h - 1), (1, 0, 3), (1, K - 1, 0), (2, 3, h - 1), (2, K - 2, 5)]:
        ref, ref_abs = _oracle_rows(qc, kc, vc, K, S, h, d, b, f, head, rows, inject)
        worst32 = max(worst32, float((oc32[b, f, rows, head] - ref).abs().max()))
        half_ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 8)
        worst16_excess = max(worst16_excess, float(((oc[b, f, rows, head] - ref).abs() - (1e-3 + half_ulp)).max()))
    assert worst32 < 1e-3, f"level {level} inject {inject}: max per-token deviation (fp32 output) {worst32:.3e}"
    assert worst16_excess < 0, f"level {level} inject {inject}: bf16 output beyond 1e-3 + half an ulp of the reference"


@pytest.mark.parametrize("S", [1000, 1024])
def test_ext_attn_injection_equals_aliased_inputs(S):
    """inject=True against running without injection on tensors whose uncond/cond q and k were overwritten by the
    source branch's (what the reference does in place, 124-130).  S = 1000: both calls run the same kernel family
    (shared-softmax dual form / plain form: same tile order, same running maximum) and must agree bit for bit.
    S = 1024: the call without injection takes the half-tile interleaved kernel, whose softmax reference point moves
    per 32 keys instead of 64 -- P is then rounded against a different shift, so the two are independent roundings of
    the same result: EACH is within 2e-4 + 2^-8 |ref| of it (the attention bound of tests/test_kernels_gpu.py; its
    P-rounding term averages out over 8192 keys), hence they differ by at most twice that: 2 x 2e-4 = the 4e-4 asserted
    (up to round 3 both calls ran ONE kernel family at S = 1024 too and the absolute term was a single 2e-4; round 4's
    lagged reference point made the interleaved kernel's shift differ from the dual kernel's)."""
    ops = _ops()
    K, h, d = 8, 8, 80
    g = torch.Generator(device="cuda").manual_seed(7)
    q, k, v = (torch.randn(3 * K, S, h * d, generator=g, device="cuda").bfloat16() for _ in range(3))
    a = ops.ext_attn(q, k, v, h, d ** -0.5, True)
    q2, k2 = q.clone(), k.clone()
    q2[K:2 * K], q2[2 * K:], k2[K:2 * K], k2[2 * K:] = q[:K], q[:K], k[:K], k[:K]
    b = ops.ext_attn(q2, k2, v, h, d ** -0.5, False)
    if S % 64:
        assert torch.equal(a, b)
    else:
        af, bf = a.float(), b.float()
        assert bool(((af - bf).abs() <= 2.0 ** -7 * bf.abs() + 4e-4).all())
        assert float((af - bf).abs().max()) < 1e-3


@pytest.mark.parametrize("S,h,d", [(4096, 8, 40), (4096, 5, 64)])
def test_ext_attn_rows_sum_to_one(S, h, d):
    """V = 1 everywhere => every output element is sum(P)/sum(P) = 1 (exact when the denominator
    comes from the same MFMA as the numerator, within 2^-7 otherwise)."""
    ops = _ops()
    K = 4
    g = torch.Generator(device="cuda").manual_seed(3)
    q, k = (torch.randn(3 * K, S, h * d, generator=g, device="cuda").bfloat16() for _ in range(2))
    out = ops.ext_attn(q, k, torch.ones_like(q), h, d ** -0.5, False).float()
    assert float((out - 1).abs().max()) <= (0.0 if d % 32 else 2.0 ** -7)


def _videolike(K, n, S, D, chunk, g):
    ln = torch.nn.functional.layer_norm
    piv = ln(torch.randn(K, S, D, generator=g, device="cuda"), (D,)).bfloat16()
    perm = torch.stack([torch.randperm(S, generator=g, device="cuda") for _ in range(n)])
    tgt = (piv[chunk].float()[perm.reshape(-1)] + 0.1 * torch.randn(n * S, D, generator=g, device="cuda")).bfloat16()
    return piv, tgt, perm.reshape(-1)


def test_nn_search_cfg2_level0_full_oracle():
    """Full-size chunk (20480 targets x 2 keyframes x 4096 pivots, D=320) against the fp32 oracle."""
    ops = _ops()
    K, n, S, D, c = 8, 5, 4096, 320, 3
    g = torch.Generator(device="cuda").manual_seed(11)
    piv, tgt, perm = _videolike(K, n, S, D, c, g)
    idx = ops.nn_search(tgt, piv, ops.pivot_inv_norm(piv), [c, c - 1]).cpu()
    assert torch.equal(idx[0].long(), perm.cpu())            # keyframe c: the planted permutation
    ref_idx, sim = orc.nn_search(tgt.float().cpu().view(n, S, D), piv.float().cpu(), c)
    n_bad = 0
    for p, (r, s) in enumerate(zip(ref_idx, sim.chunk(2, dim=1))):
        _, bad = orc.nn_mismatch_tie_aware(s, r, idx[p], 1e-5)
        n_bad += bad
    assert n_bad == 0


def test_nn_search_cfg4_level0_planted_and_sampled():
    """cfg4 geometry (S=9216, n=8: 73728 targets, 5 GiB similarity matrix in the reference):
    planted permutation for keyframe c, sampled target rows against the oracle for keyframe c-1."""
    ops = _ops()
    K, n, S, D, c = 3, 8, 9216, 320, 2
    g = torch.Generator(device="cuda").manual_seed(13)
    piv, tgt, perm = _videolike(K, n, S, D, c, g)
    idx = ops.nn_search(tgt, piv, ops.pivot_inv_norm(piv), [c, c - 1]).cpu()
    assert torch.equal(idx[0].long(), perm.cpu())
    rows = torch.randint(0, n * S, (512,), generator=torch.Generator().manual_seed(1))
    sim = orc.batch_cosine_sim(tgt[rows.cuda()].float().cpu(), piv[c - 1].float().cpu())
    _, bad = orc.nn_mismatch_tie_aware(sim, sim.argmax(-1), idx[1][rows], 1e-5)
    assert bad == 0


def _iid(K, n, S, D, g):
    """SURVEY 8(d) flavour (i): pivots AND targets are LayerNorm(N(0,1)) rows, independent -- the worst case for an
    argmax (the best and the second-best pivot of a target are a few 1e-3 apart, near-ties at the 1e-6 level occur)."""
    ln = torch.nn.functional.layer_norm
    piv = ln(torch.randn(K, S, D, generator=g, device="cuda"), (D,)).bfloat16()
    tgt = ln(torch.randn(n * S, D, generator=g, device="cuda"), (D,)).bfloat16()
    return piv, tgt


def _iid_rates(idx, tgt, piv, ids, rows=None):
    """(targets checked, raw index-diff count, beyond-tie count at tau = 1e-5) against the fp32 oracle
    (util.py:61-69 + the argmax of tokenflow_utils.py:335-343), per keyframe of `ids`."""
    total = diff = bad = 0
    t = tgt.float().cpu() if rows is None else tgt[rows.cuda()].float().cpu()
    for p_, kf in enumerate(ids):
        sim = orc.batch_cosine_sim(t, piv[kf].float().cpu())
        got = idx[p_] if rows is None else idx[p_][rows]
        a, b = orc.nn_mismatch_tie_aware(sim, sim.argmax(-1), got, 1e-5)
        total, diff, bad = total + sim.shape[0], diff + a, bad + b
    return total, diff, bad


def test_nn_search_cfg2_level0_iid_full_oracle():
    """The iid flavour at FULL size: one cfg2 level-0 chunk, 20 480 targets x 2 keyframes x 4 096 pivots, D = 320,
    every target against the fp32 oracle.  An accumulation-order difference between the MFMA contraction and torch's
    fp32 matmul may flip an argmax only inside a near-tie: beyond-tie rate (oracle similarity gap > 1e-5) must be 0;
    the raw index-diff rate is printed (the bench reports it as `nn_index_diff_rate_iid`)."""
    ops = _ops()
    K, n, S, D, c = 8, 5, 4096, 320, 3
    piv, tgt = _iid(K, n, S, D, torch.Generator(device="cuda").manual_seed(21))
    idx = ops.nn_search(tgt, piv, ops.pivot_inv_norm(piv), [c, c - 1]).cpu()
    total, diff, bad = _iid_rates(idx, tgt, piv, [c, c - 1])
    print(f"cfg2 L0 iid: {total} (target, keyframe) pairs, index differs on {diff} ({diff / total:.2e}), beyond tie {bad}")
    assert total == 2 * n * S and bad == 0
    assert diff <= 1e-3 * total


def test_nn_search_cfg4_level0_iid_sampled_rows():
    """cfg4 level 0 (S = 9 216, n = 8: 73 728 targets per chunk), iid flavour, 4 096 sampled targets x 2 keyframes
    against the fp32 oracle."""
    ops = _ops()
    K, n, S, D, c = 3, 8, 9216, 320, 2
    piv, tgt = _iid(K, n, S, D, torch.Generator(device="cuda").manual_seed(23))
    idx = ops.nn_search(tgt, piv, ops.pivot_inv_norm(piv), [c, c - 1]).cpu()
    rows = torch.randperm(n * S, generator=torch.Generator().manual_seed(2))[:4096]
    total, diff, bad = _iid_rates(idx, tgt, piv, [c, c - 1], rows)
    print(f"cfg4 L0 iid: {total} pairs, index differs on {diff} ({diff / total:.2e}), beyond tie {bad}")
    assert bad == 0 and diff <= 1e-3 * total


@pytest.mark.parametrize("S,D", [(1024, 640), (256, 1280), (64, 1280)])
def test_nn_search_coarse_levels_iid_full_oracle(S, D):
    """The other kernels of the search family (D >= 640: LDS-staged panels; few workgroups: deep-contraction form) on
    iid rows at the cfg2 sizes of levels 1-3, every target against the oracle."""
    ops = _ops()
    K, n, c = 8, 5, 5
    piv, tgt = _iid(K, n, S, D, torch.Generator(device="cuda").manual_seed(S + D))
    idx = ops.nn_search(tgt, piv, ops.pivot_inv_norm(piv), [c, c - 1]).cpu()
    total, diff, bad = _iid_rates(idx, tgt, piv, [c, c - 1])
    print(f"S={S} D={D} iid: {total} pairs, index differs on {diff} ({diff / total:.2e}), beyond tie {bad}")
    assert bad == 0 and diff <= 1e-3 * total


@pytest.mark.parametrize("n,S,D,ids,flavour", [
    (10, 1024, 640, [3, 2], "iid"),        # 40 panels x 2 keyframes x 4 pivot tiles
    (9, 1020, 640, [1, 0], "iid"),         # ragged: last pivot tile 252 rows, last target panel 220 rows
    (40, 512, 1280, [2, 1], "iid"),        # D = 1280: 20 D chunks per tile
    (20, 1024, 640, [0], "videolike"),     # one keyframe (chunk 0 of a video), planted permutation
    (3, 2304, 640, [1, 0], "iid"),         # cfg4 level 1 geometry: 9 pivot tiles
])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_nn_search_lds_dma_kernel(n, S, D, ids, flavour, dtype):
    """Shapes that take `nn_search_glds_kernel` (D % 64 == 0, D >= 512, chip-filling grid: the LDS-DMA staged
    256 x 256 tiles), every target against the fp32 oracle, tie-aware; the video-like case also against its planted
    permutation; one exact-duplicate pivot pair per keyframe: the first index must win (torch.argmax's rule)."""
    ops = _ops()
    K = max(ids) + 2
    g = torch.Generator(device="cuda").manual_seed(n * S + D)
    ln = torch.nn.functional.layer_norm
    piv = ln(torch.randn(K, S, D, generator=g, device="cuda"), (D,)).to(dtype)
    if flavour == "videolike":
        perm = torch.stack([torch.randperm(S, generator=g, device="cuda") for _ in range(n)]).reshape(-1)
        tgt = (piv[ids[0]].float()[perm] + 0.1 * torch.randn(n * S, D, generator=g, device="cuda")).to(dtype)
    else:
        tgt = ln(torch.randn(n * S, D, generator=g, device="cuda"), (D,)).to(dtype)
        piv[:, S - 7] = piv[:, 5]          # exact duplicates: row 5 must win over row S - 7 wherever they are the maximum
        tgt[:64] = piv[ids[0], 5].float().to(dtype)     # ... which they are for these targets
    idx = ops.nn_search(tgt, piv, ops.pivot_inv_norm(piv), ids).cpu()
    if flavour == "videolike":
        assert torch.equal(idx[0].long(), perm.cpu())
    else:
        assert bool((idx[0][:64] == 5).all())
    total, diff, bad = _iid_rates(idx, tgt, piv, ids)
    print(f"n={n} S={S} D={D} {flavour} {str(dtype)[6:]}: {total} pairs, index differs on {diff}, beyond tie {bad}")
    assert bad == 0 and diff <= 1e-3 * total


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_nn_search_two_target_tile_kernel_ragged(dtype):
    """A D = 320 search that takes `nn_search_rbs_kernel` with four target tiles (rbs<TJ=4>: two 32-target tiles per wave, >= 1024 workgroups of
    256 targets, >= 24 pivot tiles per workgroup) with a RAGGED last target panel (65 856 = 257.25 panels) and a pivot range
    split over two workgroups (49 tiles -> 25 + 24): every row of the last two panels and 2 048 sampled rows against the fp32
    oracle, tie-aware; exact-duplicate pivots: the first index wins; and bit-identical to the one-tile kernel
    (TF_NN_RB2_MIN_WGS is read once per process, so the comparison is against the per-frame calls, which are too small
    for the two-tile kernel)."""
    ops = _ops()
    n, S, D, ids = 42, 1568, 320, [1, 0]
    g = torch.Generator(device="cuda").manual_seed(4242)
    ln = torch.nn.functional.layer_norm
    piv = ln(torch.randn(2, S, D, generator=g, device="cuda"), (D,)).to(dtype)
    tgt = ln(torch.randn(n * S, D, generator=g, device="cuda"), (D,)).to(dtype)
    assert ops.nn_plan(n * S, S, D, 2) == ["rbs<TJ=4>[splits=2]", "finalize"]
    piv[:, S - 9] = piv[:, 11]
    tgt[-64:] = piv[1, 11].float().to(dtype)            # in the ragged last panel
    inv = ops.pivot_inv_norm(piv)
    idx = ops.nn_search(tgt, piv, inv, ids).cpu()
    assert bool((idx[0][-64:] == 11).all())
    rows = torch.cat([torch.arange(n * S - 512, n * S),
                      torch.randint(0, n * S, (2048,), generator=torch.Generator().manual_seed(3))])
    total, diff, bad = _iid_rates(idx, tgt, piv, ids, rows)
    print(f"two-tile kernel, ragged, {str(dtype)[6:]}: {total} pairs, index differs on {diff}, beyond tie {bad}")
    assert bad == 0 and diff <= 1e-3 * total
    # one frame at a time: 1 568 targets -> 7 panels, far below the two-tile kernel's grid: the one-tile kernel
    for f in (0, 17, n - 1):
        one = ops.nn_search(tgt[f * S:(f + 1) * S], piv, inv, ids).cpu()
        assert torch.equal(one, idx[:, f * S:(f + 1) * S])


@pytest.mark.parametrize("P", [1, 2])
def test_gather_blend_cfg2_level0_bit_exact(P):
    ops = _ops()
    K, n, S, D = 8, 5, 4096, 320
    g = torch.Generator().manual_seed(5)
    kf_out = torch.randn(3 * K, S, D, generator=g).bfloat16()
    res = torch.randn(3 * n, S, D, generator=g).bfloat16()
    c = 4 if P == 2 else 0
    idx = [torch.randint(0, S, (n * S,), generator=g) for _ in range(P)]
    ref = orc.gather_blend(kf_out, idx, c, n, residual=res)
    out = ops.gather_blend(kf_out.cuda(), torch.stack(idx).int().cuda(),
                           orc.blend_weights(n, 1).cuda() if P == 2 else None, orc.keyframe_ids(c), n,
                           res.cuda(), ref.dtype)
    assert out.dtype == ref.dtype and torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("in_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,D", [(98304, 320), (5120, 640), (1280, 1280)])
def test_fused_layer_norm_is_the_autocast_value(rows, D, in_dtype):
    """Pin for fusing the block's LayerNorms: under autocast torch evaluates layer_norm in fp32 and the Linear that
    consumes it rounds its input to bf16 -- that rounded tensor is what `ops.layer_norm(..., bf16)` must produce.
    Equal everywhere except where the two fp32 evaluations (different summation order) fall on opposite sides of
    a bf16 rounding boundary: at most one bf16 ulp (or the fp32 noise floor, 4e-6) apart, on < 0.05 % of the elements."""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(D)
    x = (torch.randn(rows, D, generator=g, device="cuda") * 2 + 0.3).to(in_dtype)
    ln = torch.nn.LayerNorm(D).cuda()
    with torch.no_grad():
        ln.weight.copy_(1 + 0.2 * torch.randn(D, generator=g, device="cuda"))
        ln.bias.copy_(0.1 * torch.randn(D, generator=g, device="cuda"))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ref32 = ln(x)
        assert ref32.dtype == torch.float32                      # autocast policy: layer_norm runs and returns fp32
        want = ref32.to(torch.bfloat16)                           # what the next Linear's autocast cast produces
        got, _ = ops.layer_norm(x, ln.weight, ln.bias, ln.eps, torch.bfloat16)
    diff = (got.float() - want.float()).abs()
    # one bf16 ulp (<= 2^-7 |x|); where normalised term and bias cancel to |y| << 1 the two fp32 evaluations differ by
    # their ABSOLUTE rounding noise (~1e-6 at these magnitudes), which can be many ulps of the tiny result
    ulp = 2.0 ** -7 * want.float().abs() + 4e-6
    assert bool((diff <= ulp).all()), float((diff - ulp).max())
    assert float((diff > 0).float().mean()) < 5e-4


def test_hooks_16bit_block_uses_fused_norm_and_matches_module_norm():
    """A 16-bit block takes the fused LayerNorm producer (row f2) for norm1 -- the producer of the attention input
    and of the NN-search rows, which also yields the pivots' inverse norms -- and for norm2 / norm3, whose consumers
    are Linear layers (the value is pinned by test_fused_layer_norm_is_the_autocast_value).  The block outputs stay
    within 4 bf16 ulps of the output range of the same hooks with the module LayerNorms."""
    import tokenflow_utils as tfu
    from tests import fake_diffusers as fd
    from tokenflow_amd import hooks

    torch.manual_seed(0)
    blk = fd.BasicTransformerBlock(320, 8, cross_dim=32).eval()
    holder = torch.nn.Module()
    holder.unet = torch.nn.Module()
    holder.unet.blk = blk
    holder.cuda().bfloat16()
    blk.attn1.forward = hooks._make_sa_forward(blk.attn1, pnp=True)
    hooks._set_schedule(blk.attn1, [5])
    blk.attn1.t = 5
    tfu.set_tokenflow(holder)
    K, n, S = 3, 2, 192
    g = torch.Generator().manual_seed(1)
    x_piv = torch.randn(3 * K, S, 320, generator=g).cuda().bfloat16()
    enc, enc_n = (torch.randn(3 * m, 7, 32, generator=g).cuda().bfloat16() for m in (K, n))
    perm = torch.randperm(S, generator=g)
    src = x_piv.view(3, K, S, 320)[0, 1][perm][None].repeat(n, 1, 1)
    chunk = torch.cat([src, torch.randn(2 * n, S, 320, generator=g).cuda().bfloat16()])

    def run():   # under autocast, as the reference runs its UNet passes (run_tokenflow_pnp.py:220)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            tfu.register_pivotal(holder, True)
            a = blk(x_piv, encoder_hidden_states=enc)
            inv = blk._tf_pivot_inv_norm.clone()
            tfu.register_pivotal(holder, False)
            tfu.register_batch_idx(holder, 1)
            b = blk(chunk, encoder_hidden_states=enc_n)
        return a.float(), b.float(), inv

    calls, add_calls = [], []
    real, real_add = hooks.ops.layer_norm, hooks.ops.add_layer_norm
    hooks.ops.layer_norm = lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1]
    hooks.ops.add_layer_norm = lambda *a, **k: (add_calls.append(a[0].shape), real_add(*a, **k))[1]
    try:
        fused = run()
    finally:
        hooks.ops.layer_norm, hooks.ops.add_layer_norm = real, real_add
    # norm1, norm2, norm3 in both passes: a norm that follows a residual add takes the add with it
    # (pivotal: norm2, norm3; propagation: norm3 -- its self-attention residual is added by the gather kernel, which
    # also emits norm2 of the propagation pass from its epilogue unless TOKENFLOW_FUSED_GATHER_NORM=0)
    assert len(calls) == (2 if hooks.FUSE_GATHER_NORM else 3) and len(add_calls) == 3
    keep = hooks._fused_norm_dtype
    hooks._fused_norm_dtype = lambda mod, x, in_dtype=None: None
    try:
        plain = run()
    finally:
        hooks._fused_norm_dtype = keep
    assert torch.allclose(fused[2], plain[2], rtol=1e-5)
    for f, p in zip(fused[:2], plain[:2]):
        assert f.shape == p.shape and float((f - p).abs().max()) <= 2.0 ** -6 * float(p.abs().max())


# ---------------------------------------------------------------------------------------------------------------
# Size-independent properties at BASELINE's full sizes (no oracle needed: the whole output is checked).

@pytest.mark.parametrize("cfg", ["cfg2_l0", "cfg2_l1", "cfg5_l0"])
@pytest.mark.parametrize("inject", [False, True])
def test_ext_attn_is_exactly_linear_in_a_power_of_two_of_v(cfg, inject):
    """softmax(q k^T) (2 v) = 2 softmax(q k^T) v, and doubling commutes with every rounding on the way (bf16 inputs,
    fp32 accumulation, bf16 P and output): the two launches must agree BIT FOR BIT on every one of the 3*K*S*D
    outputs -- at full size, whichever kernel form (interleaved, dual, ping-pong, split) the shape selects."""
    ops = _ops()
    K, S, h, d = {"cfg2_l0": (8, 4096, 8, 40), "cfg2_l1": (8, 1024, 8, 80), "cfg5_l0": (25, 4096, 5, 64)}[cfg]
    if cfg == "cfg5_l0":
        if inject:
            pytest.skip("the SDEdit variant has no injection")
        K = 13                                  # 13 keyframes: past the reference's K > 12 frame loop, a third of the time
    D = h * d
    g = torch.Generator(device="cuda").manual_seed(77)
    q, k, v = (torch.randn(3 * K, S, D, generator=g, device="cuda").bfloat16() for _ in range(3))
    a = ops.ext_attn(q, k, v, h, d ** -0.5, inject)
    b = ops.ext_attn(q, k, v * 2, h, d ** -0.5, inject)
    assert torch.equal(a * 2, b)
    assert bool(torch.isfinite(a.float()).all())


def test_nn_search_is_invariant_to_power_of_two_pivot_scaling():
    """cos(x, 2^j y) = cos(x, y): scaling pivot rows by powers of two scales the fp32 dot products and the inverse
    norms exactly, so every score -- hence every index -- is bit-identical (cfg2 level 0, one full chunk)."""
    ops = _ops()
    K, n, S, D, c = 8, 5, 4096, 320, 3
    g = torch.Generator(device="cuda").manual_seed(12)
    piv, tgt, _ = _videolike(K, n, S, D, c, g)
    idx = ops.nn_search(tgt, piv, ops.pivot_inv_norm(piv), [c, c - 1])
    j = torch.randint(-3, 4, (K, S, 1), generator=g, device="cuda").float()
    piv2 = (piv.float() * torch.exp2(j)).bfloat16()
    assert torch.equal(piv2.float(), piv.float() * torch.exp2(j))          # exact in bf16
    idx2 = ops.nn_search(tgt, piv2, ops.pivot_inv_norm(piv2), [c, c - 1])
    assert torch.equal(idx, idx2)
    tgt2 = (tgt.float() * 4).bfloat16()                                     # and to a positive factor on the targets
    assert torch.equal(ops.nn_search(tgt2, piv, ops.pivot_inv_norm(piv), [c, c - 1]), idx)
