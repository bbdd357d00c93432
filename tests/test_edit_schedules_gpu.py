"""Per-edit injection state of a multi-edit batch on the GPU (tests/edit_schedule_forms.py has the definition: the slices
of edit e are what the single-edit op computes on [source | uncond_e | cond_e] with edit e's OWN injection flag).

  * the composition (four-bank form off): `ext_attn_edits(..., inject_mask=m)` BIT-IDENTICAL to the parts -- per edit
    `ext_attn_views(part="bank")` with that edit's own flag and q / k views, plus the source part; the uniform masks
    bit-identical to `ext_attn_edits(inject=False / True)`;
  * the four-bank form on (Dh = 40): the plan first, then every edit against the oracle with its own flag under the
    project's attention bound on the three input families.  q, k and v are independent per branch, so a pair that read
    the neighbouring edit's bank instead of the one `gap` branches away, or an edit that does not inject computed with
    the source's q / k, lands O(1) outside the bound;
  * `inject_copy_edits_(x, E, edit_mask=m)` exact, unmasked branches bit-unchanged;
  * the config-1 hook harness with per-edit schedules over the HIP ops.
"""
import pytest
import torch

from oracle import tokenflow_oracle as orc
from tests import edit_forms as ef
from tests import edit_schedule_forms as esf
from tests.test_edits_gpu import _edit_attn_inputs
from tests.test_kernels_gpu import assert_attn_close, attn_bound, attn_ref

pytestmark = pytest.mark.gpu

MV4 = "one<40,1,4,MV4,2,fq0>"
DTYPES = [torch.bfloat16, torch.float16]
# (K, S, heads, dh): ragged frames and the fused small-problem parts / several 64-key tiles per frame, streaming / the
# measured-default class of the four-bank form and the split form on a small grid / a head dim without a four-bank form
SHAPES = [(3, 77, 2, 40), (2, 320, 2, 40), (4, 1024, 8, 40), (2, 320, 2, 80)]
MASKS = {3: [0b000, 0b111, 0b101, 0b010, 0b110], 4: [0b1011, 0b0101]}


def _ops():
    from tokenflow_amd import ops
    return ops


def _parts_reference(ops, q, k, v, K, h, d, mask, E, out_dtype):
    """tests/test_edits_gpu._parts_reference with a flag per edit."""
    B, S, D = 1 + 2 * E, q.shape[1], q.shape[2]
    q4, k4, v4 = (t.view(B, K, S, D) for t in (q, k, v))
    ref = torch.full((B, K, S, D), 7.0, dtype=out_dtype, device=q.device)
    for e, inject in enumerate(esf.mask_bits(mask, E)):
        lo = 1 + 2 * e
        if inject:
            ops.ext_attn_views(q4[0:1], k4[0:1], v4[lo:lo + 2], ref[lo:lo + 2], h, d ** -0.5, True, "bank",
                               branch0=(0, 0, 1, 1))
        else:
            ops.ext_attn_views(q4[lo:lo + 2], k4[lo:lo + 2], v4[lo:lo + 2], ref[lo:lo + 2], h, d ** -0.5, False, "bank",
                               branch0=(1, 1, 1, 1))
    ops.ext_attn_views(q4[0:1], k4[0:1], v4[0:1], ref[0:1], h, d ** -0.5, mask == (1 << E) - 1, "source",
                       branch0=(0, 0, 0, 0))
    return ref.view(B * K, S, D)


@pytest.mark.parametrize("K,S,h,d", SHAPES)
@pytest.mark.parametrize("E", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_composition_equals_the_parts(K, S, h, d, E, dtype):
    ops = _ops()
    B, D = 1 + 2 * E, h * d
    g = torch.Generator(device="cuda").manual_seed(K + S + E + d)
    q, k, v = (torch.randn(B * K, S, D, generator=g, device="cuda").to(dtype) for _ in range(3))
    for mask in MASKS[E]:
        what = f"K{K} S{S} h{h} d{d} E{E} mask {mask:#b} {dtype}"
        plan = ops.attn_edits_plan(K, K, S, h, d, False, E, dtype=dtype, multi_v=False, inject_mask=mask)
        assert MV4 not in plan and plan.count("vt_pack") <= 1, what
        got = ops.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, multi_v=False, inject_mask=mask)
        assert torch.equal(got, _parts_reference(ops, q, k, v, K, h, d, mask, E, dtype)), what
        if mask in (0, (1 << E) - 1):       # the uniform masks ARE today's call
            inject = mask != 0
            assert plan == ops.attn_edits_plan(K, K, S, h, d, inject, E, dtype=dtype, multi_v=False), what
            assert torch.equal(got, ops.ext_attn_edits(q, k, v, h, d ** -0.5, inject, E, multi_v=False)), what
        if (K, S) == (2, 320) and d == 40:  # fp32 output of the composition
            got32 = ops.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, multi_v=False, inject_mask=mask,
                                       out_dtype=torch.float32)
            assert torch.equal(got32, _parts_reference(ops, q, k, v, K, h, d, mask, E, torch.float32)), what + " fp32 out"


def test_uniform_masks_with_the_default_rule_are_the_unmasked_call():
    """Without a hint too (the measured-default class takes the four-bank form under the all-ones mask)."""
    ops = _ops()
    K, S, h, d, E = 4, 1024, 8, 40, 3
    g = torch.Generator(device="cuda").manual_seed(11)
    q, k, v = (torch.randn(7 * K, S, h * d, generator=g, device="cuda").bfloat16() for _ in range(3))
    assert MV4 in ops.attn_edits_plan(K, K, S, h, d, False, E, inject_mask=0b111)
    for mask, inject in ((0, False), (0b111, True)):
        assert ops.attn_edits_plan(K, K, S, h, d, False, E, inject_mask=mask) == ops.attn_edits_plan(K, K, S, h, d, inject, E)
        assert torch.equal(ops.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, inject_mask=mask),
                           ops.ext_attn_edits(q, k, v, h, d ** -0.5, inject, E))


@pytest.mark.parametrize("K,S,h", [s[:3] for s in SHAPES if s[3] == 40])
@pytest.mark.parametrize("E", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_four_bank_form_vs_oracle_per_edit(K, S, h, E, dtype):
    """multi_v=True at Dh = 40: popcount // 2 MV4 launches (the injecting edits in pairs, neighbours or not: 0b101 pairs
    edits 0 and 2), popcount % 2 DUAL launches beside them, one pre-pass.  Every edit against the oracle on
    [source | uncond_e | cond_e] with ITS flag, 16-bit and fp32 output, on N(0,1) / peaked / negative-first-tile inputs.
    The oracle runs once per (input family, edit, flag) and is shared among the masks."""
    ops = _ops()
    d = 40
    B, D = 1 + 2 * E, h * d
    rnd = orc.bf16_round if dtype == torch.bfloat16 else (lambda x: x.half().float())
    odev = "cuda" if K * S > 2048 else "cpu"
    if (K, S, h, E) == (4, 1024, 8, 3):     # the measured-default class: no hint needed
        assert ops.attn_edits_plan(K, K, S, h, d, False, E, dtype=dtype, inject_mask=0b101).count(MV4) == 1
    for kind in ("randn", "peaked", "negfirst"):
        q, k, v = (rnd(x) for x in _edit_attn_inputs(B * K, S, D, h, kind, seed=K * 1000 + S + E + len(kind)))
        dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
        refs = {}

        def ref_of(e, inject):
            if (e, inject) not in refs:
                r = attn_ref(*(ef.edit_slice(t, e, E).to(odev) for t in (q, k, v)), h, d ** -0.5, inject, need_sigma=False)
                refs[(e, inject)] = (r[0].cpu(), r[1].cpu(), None)
            return refs[(e, inject)]

        for mask in MASKS[E]:
            n_inj = esf.popcount(mask)
            plan = ops.attn_edits_plan(K, K, S, h, d, False, E, dtype=dtype, multi_v=True, inject_mask=mask)
            assert plan.count(MV4) == (n_inj // 2 if n_inj >= 2 else 0), (mask, plan)
            if n_inj >= 2:
                assert plan.count("vt_pack") == 1 and sum(1 for t in plan if ",DUAL," in t) == n_inj % 2, (mask, plan)
            got = ops.ext_attn_edits(dq, dk, dv, h, d ** -0.5, False, E, multi_v=True, inject_mask=mask)
            got32 = ops.ext_attn_edits(dq, dk, dv, h, d ** -0.5, False, E, multi_v=True, inject_mask=mask,
                                       out_dtype=torch.float32)
            assert torch.isfinite(got.float()).all() and got32.dtype == torch.float32, (kind, mask)
            for e, inject in enumerate(esf.mask_bits(mask, E)):
                what = f"K{K} S{S} E{E} mask {mask:#b} {kind} {dtype} edit {e} inject {inject}"
                r = ref_of(e, inject)
                err = assert_attn_close(ef.edit_slice(got, e, E), r, what, dtype=dtype)
                assert_attn_close(ef.edit_slice(got32, e, E), r, what + " fp32 out", dtype=dtype)
                print(f"{what}: max abs err {err:.3e} (bound max {float(attn_bound(r[0], r[1], dtype).max()):.3e})")


def test_masked_call_errors():
    ops = _ops()
    K, S, h, d, E = 2, 64, 2, 40, 3
    q, k, v = (torch.randn(7 * K, S, h * d, device="cuda").bfloat16() for _ in range(3))
    with pytest.raises(ValueError):
        ops.ext_attn_edits(q, k, v, h, d ** -0.5, True, E, inject_mask=0b101)
    with pytest.raises(ValueError):
        ops.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, inject_mask=0b1000)
    x = torch.randn(7 * 2, 64, device="cuda")
    with pytest.raises(ValueError):
        ops.inject_copy_edits_(x, E, edit_mask=0b1000)


@pytest.mark.parametrize("E", [3, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inject_copy_edits_masked_exact(E, dtype):
    ops = _ops()
    B, n = 1 + 2 * E, 2
    x = torch.randn(B * n, 1280, 8, 8, device="cuda").to(dtype)
    all_ones = (1 << E) - 1
    for mask in sorted({0, all_ones, 0b101, 0b010, 1 << (E - 1), all_ones & 0b10110110}):
        want = x.clone()
        for e in range(E):
            if (mask >> e) & 1:
                want[(1 + 2 * e) * n:(3 + 2 * e) * n] = x[:n].repeat(2, 1, 1, 1)
        got = ops.inject_copy_edits_(x.clone(), E, edit_mask=mask)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), f"E{E} mask {mask:#b}"   # untouched branches bit-unchanged
        if mask == all_ones:
            assert torch.equal(got, ops.inject_copy_edits_(x.clone(), E))
        if mask == 0:
            assert torch.equal(got.view(torch.uint8), x.view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------- hooks
@pytest.mark.parametrize("step", esf.STEPS)
def test_hooks_edit_schedules_cfg1_on_gpu(monkeypatch, step):
    """The harness of tests/test_edit_schedules_cpu.py over the HIP ops: E = 3, the same schedules and steps (one case per
    step: q/k masks 0b101, 0b001, 0, 0; feature masks all, all, 0b101, 0).  Per-op checks
    at the kernel tolerances (attention: the bound, with every edit's own flag; propagation: bit-exact, tie-aware on the
    indices; feature copy: bit-exact) are the binding ones.  Block outputs against the single-edit pipelines installed with
    each edit's schedules are held to 3 x the block's attention bound: the guard of
    tests/test_edits_gpu.test_hooks_multi_edit_cfg1_on_gpu, for the reason stated there (the multi-edit attention is a
    composition of parts, the single-edit pipeline's the one-call form; each lies within the bound of the oracle)."""
    ops = _ops()

    def check_attn(out3, q3, k3, v3, heads, scale, inject, what):
        r = attn_ref(q3.cuda(), k3.cuda(), v3.cuda(), heads, scale, inject, need_sigma=False)
        refs = (r[0].cpu(), r[1].cpu(), None)
        assert_attn_close(out3, refs, what)
        return float(attn_bound(refs[0], refs[1], torch.bfloat16).max())

    def nn_indices(tgt, piv, inv, ids):
        return ops.nn_search(tgt.cuda(), piv.cuda(), inv.cuda(), list(ids)).cpu()

    esf.run_edit_schedules_cfg1(lambda: ops, torch.device("cuda"), monkeypatch, check_attn, nn_indices,
                                block_tol=lambda attn_tol: 3.0 * attn_tol, steps=[step])
