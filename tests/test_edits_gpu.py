"""Multi-edit batches on the GPU: E edits of one source video in one pass, B = 1 + 2E branches
[source | uncond_1 | cond_1 | ... | uncond_E | cond_E] (tests/edit_forms.py has the definition and the helpers).

  * propagation, feature injection, attention without injection, attention under injection with the four-bank form
    off: every branch BIT-IDENTICAL to the single-edit call on [source | uncond_e | cond_e] (the bank / source parts
    for the attention);
  * attention under injection with the four-bank form on (plan token one<40,1,4,MV4,2,fq0>, asserted first): every
    edit against the oracle on [source | uncond_e | cond_e] under the project's attention bound.  Every branch carries
    its own random V, so a launch that read another edit's bank -- or skipped the O rescale of banks 2-4 on the
    peaked / negative-first-tile inputs -- lands far outside the bound: `test_multi_v_vs_oracle_per_edit` is the
    assertion that catches a wrong V bank;
  * the config-1 hook harness over the HIP ops with E = 2.
"""
import pytest
import torch

from oracle import tokenflow_oracle as orc
from tests import edit_forms as ef
from tests import nn_families as nf
from tests.test_kernels_gpu import assert_attn_close, attn_bound, attn_ref

pytestmark = pytest.mark.gpu

MV4 = "one<40,1,4,MV4,2,fq0>"
DTYPES = [torch.bfloat16, torch.float16]


def _ops():
    from tokenflow_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------------- propagation
PROP_SHAPES = [(4, 2, 1024, 320), (8, 5, 4096, 320), (3, 2, 45, 1280)]     # cfg1 level 0, cfg2 level 0, ragged (K, n, S, D)


def _prop_inputs(K, n, S, D, C, E, res_dtype, seed):
    B = 1 + 2 * E
    g = torch.Generator(device="cuda").manual_seed(seed)
    ln = torch.nn.LayerNorm(D, elementwise_affine=False)
    piv = nf.spread_pivots(K, S, D, torch.bfloat16, g)[0]      # row norms differ: a misplaced inv_norm changes the indices
    tgt = ln(torch.randn(C * n * S, D, generator=g, device="cuda")).bfloat16()
    kf = torch.randn(B * K, S, D, generator=g, device="cuda").bfloat16()
    res = torch.randn(B * C * n, S, D, generator=g, device="cuda").to(res_dtype)
    return tgt, piv, kf, res


@pytest.mark.parametrize("K,n,S,D", PROP_SHAPES)
@pytest.mark.parametrize("E", [2, 3])
@pytest.mark.parametrize("first", [False, True])
def test_propagate_chunks_edits_bit_identical(K, n, S, D, E, first):
    """A run of chunks (C = K or K - 1) and one chunk alone (C = 1), fp32 and 16-bit output, with and without the fused
    norm: every branch equals the single-edit `propagate_chunks` / `propagate` on [source | uncond_e | cond_e] bit for
    bit, and the plan shows ONE search."""
    ops = _ops()
    inv = None
    gamma, beta = torch.randn(D, device="cuda").bfloat16(), torch.randn(D, device="cuda").bfloat16()
    for C in (K - (0 if first else 1), 1):
        slot0 = 0 if first else 1
        tgt, piv, kf, res = _prop_inputs(K, n, S, D, C, E, torch.bfloat16, seed=S + C + E)
        inv = ops.pivot_inv_norm(piv)
        w = orc.blend_weights(n, 1).cuda()
        single = C == 1 and first
        search = [t for t in ops.nn_plan(n * S, S, D, 1 if single else 2, C) if t != "finalize"]
        assert ops.propagate_edits_plan(n, C, S, D, first, E) == search + [f"gather[branches={1 + 2 * E}]"]
        out_dtypes = [torch.bfloat16] if single else [torch.float32, torch.bfloat16]
        for out_dtype in out_dtypes:
            norm_ok = out_dtype == (torch.bfloat16 if single else torch.float32)
            for norm in ([None, (gamma, beta, 1e-5, torch.bfloat16)] if norm_ok else [None]):
                got = ops.propagate_chunks_edits(tgt, piv, inv, kf, w, n, C, slot0, first, res, out_dtype, E, norm=norm)
                for e in range(E):
                    ref = ops.propagate_chunks(tgt, piv, inv, ef.edit_slice(kf, e, E), w, n, C, slot0, first,
                                               ef.edit_slice(res, e, E), out_dtype, norm=norm)
                    what = f"C={C} out={out_dtype} norm={norm is not None} edit {e}"
                    if norm is None:
                        assert torch.equal(ef.edit_slice(got, e, E), ref), what
                    else:
                        assert torch.equal(ef.edit_slice(got[0], e, E), ref[0]), what
                        assert torch.equal(ef.edit_slice(got[1], e, E), ref[1]), what + " (norm)"


@pytest.mark.parametrize("res_dtype,out_dtype", [(torch.float32, torch.float32), (torch.float16, torch.float16)])
def test_propagate_chunks_edits_other_dtypes(res_dtype, out_dtype):
    """f16 cached outputs and fp32 residuals through the same entry point."""
    ops = _ops()
    K, n, S, D, E, C = 4, 2, 256, 640, 3, 3
    tgt, piv, kf, res = _prop_inputs(K, n, S, D, C, E, res_dtype, seed=5)
    tgt, piv, kf = tgt.half(), piv.half(), kf.half()
    inv, w = ops.pivot_inv_norm(piv), orc.blend_weights(n, 1).cuda()
    got = ops.propagate_chunks_edits(tgt, piv, inv, kf, w, n, C, 1, False, res, out_dtype, E)
    for e in range(E):
        ref = ops.propagate_chunks(tgt, piv, inv, ef.edit_slice(kf, e, E), w, n, C, 1, False, ef.edit_slice(res, e, E),
                                   out_dtype)
        assert torch.equal(ef.edit_slice(got, e, E), ref)


@pytest.mark.parametrize("E", [1, 2, 3, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inject_copy_edits_exact(E, dtype):
    ops = _ops()
    B, n = 1 + 2 * E, 2
    x = torch.randn(B * n, 1280, 8, 8, device="cuda").to(dtype)
    want = x.clone()
    for b in range(1, B):
        want[b * n:(b + 1) * n] = x[:n]
    got = ops.inject_copy_edits_(x.clone(), E)
    assert torch.equal(got, want)
    for e in range(E):
        assert torch.equal(ef.edit_slice(got, e, E), orc.conv_inject_(ef.edit_slice(x, e, E).clone()))


# --------------------------------------------------------------------------------------------------------- attention
def _parts_reference(ops, q, k, v, K, h, d, inject, E, out_dtype, **kw):
    """The composition's definition: per edit `ext_attn_views(part="bank")` on views of that edit's slabs, and the source
    branch through `part="source"`, written into one [B*K,S,D] tensor."""
    B, S, D = 1 + 2 * E, q.shape[1], q.shape[2]
    q4, k4, v4 = (t.view(B, K, S, D) for t in (q, k, v))
    ref = torch.full((B, K, S, D), 7.0, dtype=out_dtype, device=q.device)
    for e in range(E):
        lo = 1 + 2 * e
        if inject:
            ops.ext_attn_views(q4[0:1], k4[0:1], v4[lo:lo + 2], ref[lo:lo + 2], h, d ** -0.5, True, "bank",
                               branch0=(0, 0, 1, 1), **kw)
        else:
            ops.ext_attn_views(q4[lo:lo + 2], k4[lo:lo + 2], v4[lo:lo + 2], ref[lo:lo + 2], h, d ** -0.5, False, "bank",
                               branch0=(1, 1, 1, 1), **kw)
    ops.ext_attn_views(q4[0:1], k4[0:1], v4[0:1], ref[0:1], h, d ** -0.5, inject, "source", branch0=(0, 0, 0, 0), **kw)
    return ref.view(B * K, S, D)


# (K, S, heads, dh): streaming at cfg2 level 0, the split form on a small grid, the fused small-problem kernel
COMPOSE_SHAPES = [(8, 4096, 8, 40), (4, 1024, 8, 40), (4, 256, 8, 40), (4, 1024, 8, 64), (3, 45, 8, 40)]


@pytest.mark.parametrize("K,S,h,d", COMPOSE_SHAPES)
@pytest.mark.parametrize("E", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_without_injection_equals_the_parts(K, S, h, d, E, dtype):
    ops = _ops()
    B, D = 1 + 2 * E, h * d
    g = torch.Generator(device="cuda").manual_seed(K + S + E)
    q, k, v = (torch.randn(B * K, S, D, generator=g, device="cuda").to(dtype) for _ in range(3))
    plan = ops.attn_edits_plan(K, K, S, h, d, False, E, dtype=dtype)
    assert plan.count("vt_pack") <= 1 and MV4 not in plan
    got = ops.ext_attn_edits(q, k, v, h, d ** -0.5, False, E)
    ref = _parts_reference(ops, q, k, v, K, h, d, False, E, dtype)
    assert torch.equal(got, ref)
    if S == 1024 and d == 40:   # fp32 output of the composition
        got32 = ops.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, out_dtype=torch.float32)
        assert torch.equal(got32, _parts_reference(ops, q, k, v, K, h, d, False, E, torch.float32))


@pytest.mark.parametrize("K,S,h,d", COMPOSE_SHAPES + [(2, 320, 2, 80), (2, 72, 1, 160)])
@pytest.mark.parametrize("E", [2, 3])
def test_attention_with_injection_composition_equals_the_parts(K, S, h, d, E):
    """The DUAL composition (what runs by default, and under multi_v=False): bit for bit the bank / source parts."""
    ops = _ops()
    B, D = 1 + 2 * E, h * d
    g = torch.Generator(device="cuda").manual_seed(K + S + E + 1)
    q, k, v = (torch.randn(B * K, S, D, generator=g, device="cuda").bfloat16() for _ in range(3))
    ref = _parts_reference(ops, q, k, v, K, h, d, True, E, torch.bfloat16)
    for multi_v in (False, None):
        if multi_v is None and MV4 in ops.attn_edits_plan(K, K, S, h, d, True, E):
            continue            # a shape class whose measured default is the four-bank form: held to the oracle below
        assert MV4 not in ops.attn_edits_plan(K, K, S, h, d, True, E, multi_v=multi_v)
        assert torch.equal(ops.ext_attn_edits(q, k, v, h, d ** -0.5, True, E, multi_v=multi_v), ref)


def _edit_attn_inputs(N, S, D, h, kind, seed):
    """The three input families of tests/test_kernel_forms_gpu.py for N = B*K frames: N(0,1); peaked (planted keys of
    gain 12, many in the last 64-key tile of a frame: the deferred shift moves, O is rescaled); a strongly negative
    first tile (every score of the first 64 keys ~ -110)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(N, S, D, generator=g) for _ in range(3))
    if kind == "peaked":
        s_ = torch.arange(0, S, 5)
        k[:, (s_ * 3 + S - 60) % S] = q[:, s_] * 12.0
    elif kind == "negfirst":
        d = D // h
        u = torch.nn.functional.normalize(torch.randn(h, d, generator=g), dim=-1)
        amp = (110.0 * d ** 0.5) ** 0.5
        q = (amp * u.view(1, 1, h, d) + 0.05 * q.view(N, S, h, d)).reshape(N, S, D)
        kv = k.view(N, S, h, d)
        kv[:, :64] = -amp * u.view(1, 1, h, d) + 0.05 * kv[:, :64]
    return q, k, v


# cfg2 level 0, cfg1 level 0 (a small grid: the composition would split), ragged frames
MV_SHAPES = [(8, 4096, 8), (4, 1024, 8), (4, 45, 8), (3, 77, 8)]


@pytest.mark.parametrize("K,S,h", MV_SHAPES)
@pytest.mark.parametrize("E", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_multi_v_vs_oracle_per_edit(K, S, h, E, dtype):
    """The four-bank form (pairs of edits: QK^T and the softmax once, four P.V products), forced on.  Plan first; then
    every edit against the oracle on [source | uncond_e | cond_e] under the attention bound, on the three input
    families; the fp32 output; and multi_v=False reproduces the DUAL composition bit for bit.
    (The oracle's own code runs on the device tensors at the level-0 size: 4 TFLOP per call are minutes on the host.)"""
    ops = _ops()
    d = 40
    B, D = 1 + 2 * E, h * d
    plan = ops.attn_edits_plan(K, K, S, h, d, True, E, dtype=dtype, multi_v=True)
    assert plan.count(MV4) == E // 2 and plan.count("vt_pack") == 1, plan
    assert sum(1 for t in plan if ",DUAL," in t) == E % 2, plan
    rnd = orc.bf16_round if dtype == torch.bfloat16 else (lambda x: x.half().float())
    odev = "cuda" if K * S > 8192 else "cpu"
    kinds = ["randn", "peaked", "negfirst"]
    for kind in kinds:
        q, k, v = (rnd(x) for x in _edit_attn_inputs(B * K, S, D, h, kind, seed=K * 1000 + S + E + len(kind)))
        dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
        got = ops.ext_attn_edits(dq, dk, dv, h, d ** -0.5, True, E, multi_v=True)
        assert torch.isfinite(got.float()).all(), kind
        got32 = ops.ext_attn_edits(dq, dk, dv, h, d ** -0.5, True, E, multi_v=True, out_dtype=torch.float32)
        assert got32.dtype == torch.float32 and torch.equal(got32.to(dtype), got), kind
        for e in range(E):
            refs = attn_ref(*(ef.edit_slice(t, e, E).to(odev) for t in (q, k, v)), h, d ** -0.5, True, need_sigma=False)
            what = f"multi-V K{K} S{S} E{E} {kind} {dtype} edit {e}"
            err = assert_attn_close(ef.edit_slice(got, e, E), refs, what, dtype=dtype)
            assert_attn_close(ef.edit_slice(got32, e, E), refs, what + " fp32 out", dtype=dtype)
            print(f"{what}: max abs err {err:.3e} (bound max {float(attn_bound(refs[0], refs[1], dtype).max()):.3e})")
        if kind == "randn":
            off = ops.ext_attn_edits(dq, dk, dv, h, d ** -0.5, True, E, multi_v=False)
            assert torch.equal(off, _parts_reference(ops, dq, dk, dv, K, h, d, True, E, dtype))


def test_multi_v_does_not_exist_outside_its_form():
    """Head dims other than 40, no injection, the folded scale, one edit: the hint selects nothing, the composition runs."""
    ops = _ops()
    K, S, h, E = 2, 320, 2, 2
    for d, inject, fold in [(64, True, False), (40, False, False), (40, True, True)]:
        assert MV4 not in ops.attn_edits_plan(K, K, S, h, d, inject, E, multi_v=True, fold_scale=fold)
        g = torch.Generator(device="cuda").manual_seed(d)
        q, k, v = (torch.randn(5 * K, S, h * d, generator=g, device="cuda").bfloat16() for _ in range(3))
        a = ops.ext_attn_edits(q, k, v, h, d ** -0.5, inject, E, multi_v=True, fold_scale=fold)
        b = ops.ext_attn_edits(q, k, v, h, d ** -0.5, inject, E, multi_v=False, fold_scale=fold)
        assert torch.equal(a, b)
    q, k, v = (torch.randn(3 * K, S, h * 40, device="cuda").bfloat16() for _ in range(3))
    assert torch.equal(ops.ext_attn_edits(q, k, v, h, 40 ** -0.5, True, 1, multi_v=True), ops.ext_attn(q, k, v, h, 40 ** -0.5, True))


# ------------------------------------------------------------------------------------------------------------- hooks
def test_hooks_multi_edit_cfg1_on_gpu(monkeypatch):
    """The harness of tests/test_edits_hooks_cpu.py over the HIP ops, E = 2, one step per injection state.  Per-op
    checks at the kernel tolerances of tests/test_kernels_gpu.py (attention: the bound; propagation: bit-exact,
    tie-aware on the indices; feature copy: bit-exact): THESE are the binding checks.  Block outputs against the
    single-edit pipeline are a coarse end-to-end guard on top of them, not a derived bound: the multi-edit attention is
    the composition of the parts (or the four-bank form) and the single-edit pipeline's the one-call form, so the two
    differ by kernel error carried through to_out, the residual, the norms and the feed-forward (random-init stand-ins
    of gain <= 1).  test_cfg1_end_to_end_public_installers holds the single-edit path within 1.5 x the block's
    attention bound of the rounding-matched host computation on that informal argument; two such results are taken to
    lie within 3 x of each other here.  A wrong branch or bank moves a block output by O(1), far outside it."""
    ops = _ops()

    def check_attn(out3, q3, k3, v3, heads, scale, inject, what):
        refs = attn_ref(q3.cuda(), k3.cuda(), v3.cuda(), heads, scale, inject, need_sigma=False)
        assert_attn_close(out3, refs, what)
        return float(attn_bound(refs[0], refs[1], torch.bfloat16).max())

    def nn_indices(tgt, piv, inv, ids):
        return ops.nn_search(tgt.cuda(), piv.cuda(), inv.cuda(), list(ids)).cpu()

    ef.run_edits_cfg1(lambda: ops, torch.device("cuda"), monkeypatch, 2, [0, 10, 16], check_attn, nn_indices,
                      block_tol=lambda attn_tol: 3.0 * attn_tol)
