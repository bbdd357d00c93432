"""Frame-set keyframe bank for a multi-edit batch on the GPU (tf_ext_attn_fwd_frame_sets_edits,
hooks.register_bank_window(..., edits=True, anchors=..., anchor_edits=True)): the uncond / cond branches of EVERY edit attend,
for keyframe i, to the member frames of set i in ascending order; the source branch to its own frame, once; nothing mixes edits.

  * q, k, v are independent per branch and frame, so a launch that read a skipped frame, missed a member, or took another
    edit's bank lands O(1) off.  Every edit and every frame is held to the oracle on the GATHERED member slices of
    [source | uncond_e | cond_e] with edit e's injection flag, within the attention bound of tests/test_kernels_gpu.py, on
    N(0,1) and on peaked inputs, with 16-bit and fp32 output, in the default mode (small grids split the member list into runs;
    the scattered table's sets of 1 to 3 frames leave empty runs) and under no_split.
  * Under no_split edit e's slices are bit-identical to `ops.ext_attn_frame_sets` on [source | uncond_e | cond_e] with edit e's
    flag wherever both plans name the same kernel forms (asserted as a precondition with the plan functions).
  * The frame-set four-bank form: every frame of a paired edit is bit-identical to its OWN four-bank call, `ops.ext_attn_edits`
    on the gathered members with Kq = 1, q_frame0 = the rank of the own frame; planted keys in an anchor land in all four banks,
    planted keys in a skipped frame leave no trace.
  * identities and refusals on the device; one block through the hooks."""
import re

import pytest
import torch

import tokenflow_utils as tfu
from tests import edit_forms as ef
from tests.test_frame_sets_gpu import TABLES, _frame_refs, _gather, _rnd, members
from tests.test_kernels_gpu import assert_attn_close
from tests.test_windows_edits_gpu import MV4_CASES, _bits, _first_edits, _hook_pipe, _inputs
from oracle import golden_cases as gc
from tokenflow_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
K, H = 6, 2
E_MAX = 3
SET_TABLES = ("R1+a0", "scattered")      # one-member sets, skips of 2 and 3 frames, the own frame first, in the middle and last


def _ops():
    from tokenflow_amd import ops
    return ops


def _gather_b(t, B, frames):
    """[B K, S, D] -> the frames `frames` of every branch next to each other, [B len(frames), S, D]."""
    idx = torch.as_tensor(list(frames), device=t.device)
    return t.view(B, K, *t.shape[1:])[:, idx].reshape(B * len(frames), *t.shape[1:]).contiguous()


class _Refs:
    """Per (edit, injection flag): the per-frame oracle results on the gathered member slices, computed once."""

    def __init__(self, q, k, v, sets, Dh):
        self.q, self.k, self.v, self.sets, self.scale, self.memo = q, k, v, sets, Dh ** -0.5, {}

    def __call__(self, e, inj):
        if (e, inj) not in self.memo:
            q3, k3, v3 = (ef.edit_slice(t, e, E_MAX) for t in (self.q, self.k, self.v))
            self.memo[(e, inj)] = _frame_refs(q3, k3, v3, K, self.sets, H, self.scale, inj)
        return self.memo[(e, inj)]


def _check_bound(got, E, mask, refs, what, dtype):
    """Every edit and every frame of `got` (a host tensor) against the oracle on the gathered members."""
    worst = 0.0
    for e, inj in enumerate(_bits(mask, E)):
        got3, fr = ef.edit_slice(got, e, E), refs(e, inj)
        for i in range(K):
            worst = max(worst, assert_attn_close(_gather(got3, K, [i]), fr[i], f"{what} edit {e} frame {i}", dtype=dtype))
    return worst


def _forms(plan, composed):
    """The kernel forms a plan names, (bank launch per edit in launch order, source launch): the tokens without the pre-pass and
    without the query waves of a fused launch (its arithmetic depends on KW and PREC only: include/tokenflow_hip.h).  A
    single-edit call whose ONE launch computes the bank and the source problems (the ALL form, the fused kernel) names that
    kernel for both: its source problems are the SOURCE form's arithmetic."""
    toks = [re.sub(r"qw=\d,", "", t) for t in plan if t != "vt_pack"]
    assert not any(t.startswith("merge") for t in toks), plan
    if composed:
        return toks[:-1], toks[-1]
    if len(toks) == 1:
        return toks, toks[0].replace(",set", "").replace("ALL", "SOURCE")
    assert len(toks) == 2, plan
    return toks[:1], toks[1]


# (S, Dh, kwargs, what the frame-set launches are, dtypes)
COMPOSITION_CASES = [
    (48, 40, {}, "fused", DTYPES),
    (320, 64, {"fused": False}, "one<64", DTYPES),                                     # one-tile streaming, ragged
    (512, 40, {"fused": False, "hints": _lib.TF_ATTN_HINT_MIX}, "il<40", DTYPES[:1]),  # interleaved
    (576, 64, {"fused": False}, "il<64", DTYPES[:1]),                                  # interleaved, LDS-DMA staged
    (128, 160, {"fused": False}, "one<160", DTYPES[:1]),
]
COMPOSITION_PARAMS = [(S, Dh, kw, form, dt) for S, Dh, kw, form, dts in COMPOSITION_CASES for dt in dts]


@pytest.mark.parametrize("S,Dh,kw,form,dtype", COMPOSITION_PARAMS,
                         ids=[f"S{c[0]}-Dh{c[1]}-{c[3].strip('<')}-{str(c[4])[6:]}" for c in COMPOSITION_PARAMS])
@pytest.mark.parametrize("table", SET_TABLES)
def test_composition(S, Dh, kw, form, dtype, table):
    ops = _ops()
    sets, D, scale = TABLES[table], H * Dh, Dh ** -0.5
    n_equal = 0
    for kind in ("randn", "peaked"):
        q, k, v = (_rnd(t, dtype) for t in _inputs(E_MAX, S, D, kind, seed=S + Dh + len(kind)))
        refs = _Refs(q, k, v, sets, Dh)
        dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
        single = {}      # (edit, flag) -> ops.ext_attn_frame_sets on [source | uncond_e | cond_e], under no_split
        for E in (2, 3):
            eq, ek, ev = (_first_edits(t, E) for t in (dq, dk, dv))
            for mask in (0, (1 << E) - 1, 0b01):
                for no_split in (False, True):
                    what = f"S{S} Dh{Dh} {table} E{E} mask {mask:#b} no_split={no_split} {kind} {dtype}"
                    plan = ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, E, mask, dtype=dtype, no_split=no_split, multi_v=False, **kw)
                    marked = [t for t in plan if t.endswith(",set") or t.endswith(",set]")]
                    assert len(marked) == E and all(t.startswith(form) for t in marked), plan
                    assert plan.count("vt_pack") == (0 if form == "fused" else 1) and not any("MV4" in t for t in plan), plan
                    got = ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, False, E, sets, inject_mask=mask, no_split=no_split,
                                                        multi_v=False, **kw)
                    got32 = ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, False, E, sets, inject_mask=mask, no_split=no_split,
                                                          multi_v=False, out_dtype=torch.float32, **kw)
                    assert got32.dtype == torch.float32 and torch.equal(got32.to(dtype), got)
                    assert torch.isfinite(got32).all()
                    err = _check_bound(got.cpu(), E, mask, refs, what, dtype)
                    _check_bound(got32.cpu(), E, mask, refs, what + " fp32 out", dtype)
                    if not no_split:
                        continue
                    banks, source = _forms(plan, composed=True)
                    order = [e for e in range(E) if (mask >> e) & 1] + [e for e in range(E) if not (mask >> e) & 1]
                    for e, inj in enumerate(_bits(mask, E)):
                        own_plan = ops.attn_frame_sets_plan(K, sets, S, H, Dh, inj, dtype=dtype, no_split=True, **kw)
                        own_banks, own_source = _forms(own_plan, composed=False)
                        # the shapes are chosen so that the precondition holds
                        assert [banks[order.index(e)]] == own_banks and source == own_source, (plan, own_plan)
                        if (e, inj) not in single:
                            single[(e, inj)] = ops.ext_attn_frame_sets(*(ef.edit_slice(t, e, E_MAX) for t in (dq, dk, dv)), H, scale, inj,
                                                                       sets, no_split=True, **kw)
                        assert torch.equal(ef.edit_slice(got, e, E), single[(e, inj)]), f"{what} edit {e}"
                        n_equal += 1
                    print(f"{what}: max abs err {err:.3e}, every edit equal to its single-edit frame-set call; plan {plan}")
        if kind == "randn":      # the shared-state spelling is the uniform mask
            eq, ek, ev = (_first_edits(t, 2) for t in (dq, dk, dv))
            for inject in (False, True):
                assert torch.equal(ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, inject, 2, sets, multi_v=False, **kw),
                                   ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, False, 2, sets, inject_mask=3 * inject,
                                                                 multi_v=False, **kw))
    assert n_equal == 2 * 3 * (2 + 3)


@pytest.mark.parametrize("Dh", [40, 64])
@pytest.mark.parametrize("S", [45, 320])      # less than one tile: every tile boundary is a hop / five ragged tiles per frame
@pytest.mark.parametrize("dtype", DTYPES)
def test_four_bank_set_form(Dh, S, dtype):
    ops = _ops()
    D, scale = H * Dh, Dh ** -0.5
    hint = {"multi_v": True} if Dh == 40 else {"multi_v64": True}
    token = "one<40,1,4,MV4,2,fq0>" if Dh == 40 else "one<64,1,8,MV4,2,fq1>"
    n_equal = 0
    for table in SET_TABLES:
        sets = TABLES[table]
        for kind in ("randn", "peaked"):
            q, k, v = (_rnd(t, dtype) for t in _inputs(E_MAX, S, D, kind, seed=S + Dh + len(kind) + 1))
            refs = _Refs(q, k, v, sets, Dh)
            dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
            for E, mask, pair, name in MV4_CASES:
                eq, ek, ev = (_first_edits(t, E) for t in (dq, dk, dv))
                B = 1 + 2 * E
                for no_split in (False, True):
                    what = f"S{S} Dh{Dh} {table} {name} no_split={no_split} {kind} {dtype}"
                    plan = ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, E, mask, dtype=dtype, no_split=no_split, **hint)
                    assert [t for t in plan if "MV4" in t] == [token + ",set"] and plan.count("vt_pack") == 1, plan
                    got = ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, False, E, sets, inject_mask=mask, no_split=no_split, **hint)
                    got32 = ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, False, E, sets, inject_mask=mask, no_split=no_split,
                                                          out_dtype=torch.float32, **hint)
                    assert torch.equal(got32.to(dtype), got) and torch.isfinite(got32).all()
                    err = _check_bound(got.cpu(), E, mask, refs, what, dtype)
                    _check_bound(got32.cpu(), E, mask, refs, what + " fp32 out", dtype)
                    # every frame of a paired edit against its own four-bank call on the gathered members
                    for i, m in enumerate(sets):
                        fr = members(m)
                        own_plan = ops.attn_edits_plan(len(fr), 1, S, H, Dh, False, E, dtype=dtype, no_split=no_split, inject_mask=mask,
                                                       **hint)
                        assert [t for t in own_plan if "MV4" in t] == [token], own_plan
                        own = ops.ext_attn_edits(_gather_b(eq, B, [i]), _gather_b(ek, B, fr), _gather_b(ev, B, fr), H, scale, False, E,
                                                 q_frame0=fr.index(i), no_split=no_split, inject_mask=mask, **hint)
                        for e in pair:
                            for b in (1 + 2 * e, 2 + 2 * e):
                                assert torch.equal(got.view(B, K, S, D)[b, i], own.view(B, 1, S, D)[b, 0]), f"{what} frame {i} branch {b}"
                        n_equal += 1
                    print(f"{what}: max abs err {err:.3e}, paired edits equal to every frame's own four-bank call; plan {plan}")
    assert n_equal == 2 * 2 * len(MV4_CASES) * 2 * K


@pytest.mark.parametrize("Dh", [40, 64])
def test_planted_key_in_the_anchor_and_in_a_skipped_frame_four_bank_form(Dh):
    """Query frame 4 of R1+a0 has the set {0, 3, 4, 5}; both edits inject.  A gain-12 match for frame 4's SOURCE queries placed in
    anchor frame 0, far from the window, must dominate all four bank outputs: the value planted beside it comes out, a different
    one per bank, so swapped banks show.  The same match in frame 1 or 2 -- the frames between anchor and window, which the
    cursors skip -- must leave frame 4 bit for bit unchanged in every branch, while it does change a frame whose set holds it."""
    ops = _ops()
    S, E, f, D, scale = 320, 2, 4, H * Dh, Dh ** -0.5
    B = 1 + 2 * E
    hint = {"multi_v": True} if Dh == 40 else {"multi_v64": True}
    sets = TABLES["R1+a0"]
    assert members(sets[f]) == [0, 3, 4, 5]
    assert any("MV4" in t and t.endswith(",set") for t in ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, E, 0b11, **hint))
    q, k, v = (_rnd(t, torch.bfloat16) for t in _inputs(E, S, D, "randn", seed=23 + Dh))
    rows = torch.arange(0, S, 3)

    def planted(frame):
        k2, v2 = k.clone().view(B, K, S, D), v.clone().view(B, K, S, D)
        k2[0, frame, (rows + 1) % S] = _rnd(q.view(B, K, S, D)[0, f, rows] * 12.0, torch.bfloat16)
        for b in range(1, B):
            v2[b, frame, (rows + 1) % S] = 100.0 + 8.0 * b
        return k2.view(B * K, S, D), v2.view(B * K, S, D)

    dq = q.bfloat16().cuda()
    for no_split in (False, True):
        run = lambda kk, vv: ops.ext_attn_frame_sets_edits(dq, kk.bfloat16().cuda(), vv.bfloat16().cuda(), H, scale, True, E, sets,   # noqa: E731
                                                           no_split=no_split, **hint).float().view(B, K, S, D)
        base = run(k, v)
        anchor = run(*planted(0))
        for b in range(1, B):
            # logit of the match: 12 |q|^2 scale ~ 12 sqrt(Dh) >= 75 above the N(0, 1) scores of <= 1300 other keys
            want = torch.full_like(anchor[b, f, rows], 100.0 + 8.0 * b)
            assert torch.allclose(anchor[b, f, rows], want, rtol=2.0 ** -7), (b, no_split)
            assert not torch.allclose(base[b, f, rows], anchor[b, f, rows], rtol=0.5)
        for skipped, holder in ((1, 2), (2, 3)):      # sets[2] = {0,1,2,3} holds frame 1, sets[3] = {0,2,3,4} holds frame 2
            assert (sets[holder] >> skipped) & 1 and not (sets[f] >> skipped) & 1
            outside = run(*planted(skipped))
            assert torch.equal(outside[:, f], base[:, f]), (skipped, no_split)
            assert not torch.equal(outside[1, holder], base[1, holder]) and not torch.equal(outside[4, holder], base[4, holder])


def test_identities_and_refusals():
    ops = _ops()
    S, Dh = 64, 40
    scale = Dh ** -0.5
    q, k, v = (t.bfloat16().cuda() for t in _inputs(E_MAX, S, H * Dh, "randn", 3))
    irregular = [(0, 1), (0, 3), (1, 4), (3, 1), (2, 4), (4, 2)]
    for kw in ({}, {"fused": False}, {"fused": False, "multi_v": True}):
        single_kw = {x: y for x, y in kw.items() if x == "fused"}
        for E, mask in ((2, 0b11), (3, 0b101), (3, 0)):
            eq, ek, ev = (_first_edits(t, E) for t in (q, k, v))
            for sets in ([(1 << K) - 1] * K, ops.bank_frame_sets(K, K + 4, [2])):      # full sets: the masked multi-edit call
                assert torch.equal(ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, False, E, sets, inject_mask=mask, **kw),
                                   ops.ext_attn_edits(eq, ek, ev, H, scale, False, E, inject_mask=mask, **kw))
            for windows in (ops.bank_windows(K, 1), ops.bank_windows(K, 2), irregular):      # ranges: the windowed multi-edit call
                sets = [((1 << n) - 1) << lo for lo, n in windows]
                assert torch.equal(ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, False, E, sets, inject_mask=mask, **kw),
                                   ops.ext_attn_windows_edits(eq, ek, ev, H, scale, False, E, windows, inject_mask=mask, **kw))
        for inject in (False, True):      # one edit: the frame-set call
            for table in SET_TABLES:
                q1, k1, v1 = (_first_edits(t, 1) for t in (q, k, v))
                assert torch.equal(ops.ext_attn_frame_sets_edits(q1, k1, v1, H, scale, inject, 1, TABLES[table], **kw),
                                   ops.ext_attn_frame_sets(q1, k1, v1, H, scale, inject, TABLES[table], **single_kw))
    eq, ek, ev = (_first_edits(t, 2) for t in (q, k, v))
    good = TABLES["R1+a0"]
    out = torch.full((5 * K, S, H * Dh), 7.0, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):      # a wrong-length table
        ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, True, 2, ops.bank_frame_sets(K - 1, 1, [0]), out=out)
    with pytest.raises(ValueError, match="own frame"):
        ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, True, 2, [0b101] * K, out=out)
    with pytest.raises(ValueError, match="inside"):
        ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, True, 2, [0] + good[1:], out=out)
    for bits in (_lib.TF_ATTN_FOLD_SCALE, _lib.TF_ATTN_BANK_ONLY, _lib.TF_ATTN_SOURCE_ONLY, _lib.TF_ATTN_RUN_MULTI_V):
        with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_fwd_frame_sets_edits"):
            ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, True, 2, good, hints=bits, out=out)
    with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_fwd_frame_sets_edits.*exclude each other"):
        ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, True, 2, good, multi_v=False, multi_v64=True, out=out)
    with pytest.raises(ValueError, match="inject=True beside a mask"):
        ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, True, 2, good, inject_mask=1, out=out)
    with pytest.raises(ValueError):
        ops.ext_attn_frame_sets_edits(eq, ek, ev, H, scale, False, 2, good, inject_mask=0b100, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())      # refused before any launch


# -------------------------------------------------------------------------------------------------------------- hooks
@pytest.mark.parametrize("schedules", [False, True], ids=["shared", "per-edit"])
@pytest.mark.parametrize("no_split", [True, False])
def test_hooks_bank_window_anchor_edits(monkeypatch, schedules, no_split):
    """One block (it injects at this step) through `register_edits(pipe, 2)` + `register_bank_window(pipe, 1, edits=True,
    anchors=[0], anchor_edits=True)`; with per-edit schedules only edit 0 injects.  The attention of the pivotal pass per edit:
    against the oracle on the gathered members, and against the single-edit anchored pass (`ops.ext_attn_frame_sets` on the
    edit's own three branches with its own flag) -- within the bound of the oracle always, bit for bit under no_split where the
    two plans name the same forms.  The pass differs from the windowed and from the whole-bank multi-edit pass, a covering radius
    reproduces the latter bit for bit, and the chunk pass issues what it issues today."""
    ops = _ops()
    monkeypatch.setattr(ops, "FP32_AS", torch.bfloat16)
    monkeypatch.setattr(ops, "NO_SPLIT", no_split)
    Kh, n, S, R, E = 5, 2, 48, 1, 2
    B = 1 + 2 * E
    checked, chunk_calls, n_equal = [], [], [0]
    real, real_single, real_chunks = ops.ext_attn_frame_sets_edits, ops.ext_attn_frame_sets, ops.propagate_chunks_edits

    def spy(q, k, v, heads, scale, inject, n_edits, sets, *, inject_mask=None, **kw):
        out = real(q, k, v, heads, scale, inject, n_edits, sets, inject_mask=inject_mask, **kw)
        assert not inject and n_edits == E
        dh = q.shape[-1] // heads
        qc, kc, vc, oc = (t.float().cpu().contiguous() for t in (q, k, v, out))
        plan = ops.attn_frame_sets_edits_plan(Kh, sets, S, heads, dh, E, inject_mask, dtype=q.dtype, no_split=True)
        order = [e for e in range(E) if (inject_mask >> e) & 1] + [e for e in range(E) if not (inject_mask >> e) & 1]
        for e, inj in enumerate(_bits(inject_mask, E)):
            q3, k3, v3, o3 = (ef.edit_slice(t, e, E) for t in (qc, kc, vc, oc))
            refs = _frame_refs(q3, k3, v3, Kh, sets, heads, scale, inj)
            single = real_single(*(ef.edit_slice(t, e, E).contiguous() for t in (q, k, v)), heads, scale, inj, sets).float().cpu()
            for i in range(Kh):
                assert_attn_close(_gather(o3, Kh, [i]), refs[i], f"hooks edit {e} frame {i}", dtype=q.dtype)
                assert_attn_close(_gather(single, Kh, [i]), refs[i], f"hooks single-edit pass, edit {e} frame {i}", dtype=q.dtype)
            if no_split:
                banks, source = _forms(plan, composed=True)
                own_banks, own_source = _forms(ops.attn_frame_sets_plan(Kh, sets, S, heads, dh, inj, dtype=q.dtype, no_split=True),
                                               composed=False)
                if [banks[order.index(e)]] == own_banks and source == own_source:
                    assert torch.equal(o3, single), f"hooks edit {e}"
                    n_equal[0] += 1
        checked.append((tuple(sets), int(inject_mask), q.dtype))
        return out

    def spy_chunks(tgt, piv, inv_norm, kf_out, w, n_, n_chunks, slot0, first_single, residual, out_dtype, n_edits, **kw):
        chunk_calls.append((tuple(tgt.shape), tuple(kf_out.shape), n_, n_chunks, slot0, first_single, n_edits))
        return real_chunks(tgt, piv, inv_norm, kf_out, w, n_, n_chunks, slot0, first_single, residual, out_dtype, n_edits, **kw)
    monkeypatch.setattr(ops, "ext_attn_frame_sets_edits", spy)
    monkeypatch.setattr(ops, "propagate_chunks_edits", spy_chunks)

    def pipe_for(radius, **kw):
        pipe = _hook_pipe(E)
        if schedules:
            tfu.register_edit_schedules(pipe, qk_schedules=[[801], []])
        if radius is not None:
            tfu.register_bank_window(pipe, radius, **kw)
        return pipe

    def run(pipe):
        blk = pipe.unet.up_blocks[2].attentions[0].transformer_blocks[0]
        D, cross = blk.norm1.normalized_shape[0], gc.BLOCKS_CFG["cross_dim"]
        g = torch.Generator().manual_seed(11)
        x_piv, enc_piv = torch.randn(B * Kh, S, D, generator=g).cuda(), torch.randn(B * Kh, 7, cross, generator=g).cuda()
        x_ch, enc_ch = torch.randn(B * Kh * n, S, D, generator=g).cuda(), torch.randn(B * Kh * n, 7, cross, generator=g).cuda()
        del chunk_calls[:]
        with torch.no_grad():
            tfu.register_pivotal(pipe, True)
            piv = blk(x_piv, encoder_hidden_states=enc_piv)
            tfu.register_pivotal(pipe, False)
            tfu.register_batch_idx(pipe, range(Kh))
            chunks = blk(x_ch, encoder_hidden_states=enc_ch)
        return piv.float(), chunks.float(), list(chunk_calls)

    anc_piv, anc_chunks, anc_calls = run(pipe_for(R, edits=True, anchors=[0], anchor_edits=True))
    assert checked == [(tuple(ops.bank_frame_sets(Kh, R, [0])), 0b01 if schedules else 0b11, torch.bfloat16)]
    assert not no_split or n_equal[0] == E      # the block's shape is one at which the precondition holds
    assert torch.isfinite(anc_piv).all() and torch.isfinite(anc_chunks).all()
    win_piv, _, _ = run(pipe_for(R, edits=True))
    full_piv, full_chunks, full_calls = run(pipe_for(None))
    assert not torch.equal(anc_piv, win_piv) and not torch.equal(anc_piv, full_piv)      # an opt-in that changes the result
    assert anc_calls == full_calls and len(full_calls) == 1    # the chunk pass issues what it issues today
    cov_piv, cov_chunks, cov_calls = run(pipe_for(Kh - 1, edits=True, anchors=[0, 2], anchor_edits=True))
    assert len(checked) == 1 and cov_calls == full_calls       # a covering radius is the whole-bank multi-edit pass, bit for bit
    assert torch.equal(cov_piv, full_piv) and torch.equal(cov_chunks, full_chunks)
    with torch.no_grad(), pytest.raises(ValueError, match="register_bank_window: anchor keyframes in a multi-edit batch"):
        run(pipe_for(R, edits=True, anchors=[0]))              # without the keyword: today's error
