"""Keyframe segments on the GPU: several scenes or clips in one pass (tf_ext_attn_fwd_segments,
tf_nn_gather_blend_chunks_segments, hooks.register_segments).  For every op the slices of segment v must be what the
single-clip op computes on segment v's tensors alone.

  * attention: q, k, v are independent per segment, so a launch that read a neighbour's bank lands O(1) off.  Segments that
    stream are bit-identical to `ops.ext_attn` on the segment's tensors (same kernels on the same values); the joint fused
    launch is bit-identical under no_split=True, where the fused plan is a function of the shape alone.  Everything is held to
    the oracle, per segment, within the attention bound of tests/test_kernels_gpu.py, on N(0,1) and on peaked inputs.
  * propagation: bit-identical to the per-segment `ops.propagate_chunks` / `ops.propagate` calls wherever the C-chunk search
    and the per-segment searches take the same kernel form (asserted as a precondition, shapes chosen on the CPU with
    `ops.nn_plan`: the smallest S at which every call of the case reaches the family); indices tie-aware against the fp32
    oracle.
  * hooks: one block through `register_segments([2, 3])` against two single-clip runs of the same block."""
import re

import pytest
import torch

import tokenflow_utils as tfu
from oracle import golden_cases as gc
from oracle import tokenflow_oracle as orc
from tests import fake_diffusers as fd
from tests import nn_families as nf
from tests.test_kernels_gpu import NN_TAU, assert_attn_close, attn_ref
from tokenflow_amd import _lib, hooks

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _ops():
    from tokenflow_amd import ops
    return ops


def _rnd(x, dtype):
    return x.to(dtype).float()


# ---------------------------------------------------------------------------------------------------------- attention
K_ATTN = 5
SEGMENTS = [(2, 3), (1, 1, 3)]
# (S, H, Dh, kwargs, path): the path a segment's own call takes under these kwargs
ATTN_CASES = [
    (48, 2, 40, {}, "fused"),                                                      # ragged S
    (192, 2, 160, {}, "fused"),
    (320, 2, 64, {"fused": False}, "one<"),                                        # one-tile streaming
    (512, 2, 40, {"fused": False, "hints": _lib.TF_ATTN_HINT_MIX}, "il<"),         # interleaved
    (320, 2, 80, {}, "stream"),                                                    # streaming under no_split; fused on this small grid otherwise
]


def _attn_inputs(S, D, kind, seed):
    """Independent q, k, v for every frame (hence for every segment).  peaked: planted keys of gain 12 inside every frame, many
    in its last 64-key tile (the family of tests/test_edits_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(3 * K_ATTN, S, D, generator=g) for _ in range(3))
    if kind == "peaked":
        s_ = torch.arange(0, S, 5)
        k[:, (s_ * 3 + S - 60) % S] = q[:, s_] * 12.0
    return q, k, v


def _win(t, f0, f1):
    return t.view(3, K_ATTN, *t.shape[1:])[:, f0:f1].reshape(3 * (f1 - f0), *t.shape[1:])


@pytest.mark.parametrize("S,H,Dh,kw,path", ATTN_CASES, ids=[f"S{c[0]}-Dh{c[2]}-{c[4].strip('<')}" for c in ATTN_CASES])
@pytest.mark.parametrize("segs", SEGMENTS, ids=["2+3", "1+1+3"])
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_segments(S, H, Dh, kw, path, segs, inject, dtype):
    ops = _ops()
    D, scale = H * Dh, Dh ** -0.5
    for no_split in (False, True):
        plan = ops.attn_segments_plan(K_ATTN, segs, S, H, Dh, inject, dtype=dtype, no_split=no_split, **kw)
        own = [ops.attn_plan(k, k, S, H, Dh, inject, dtype=dtype, no_split=no_split, **kw) for k in segs]
        fused = any(t.startswith("fused") for t in plan)
        if path == "fused":
            assert plan == [own[0][0][:-1] + f",sets={len(segs)}]"] or not no_split and len(plan) == 1 and fused, plan
        elif path == "stream":
            assert fused != no_split, plan            # S = 320 > 256: the bit-stable mode streams
        else:
            assert not fused and plan.count("vt_pack") == 1 and any(t.startswith(path) for t in plan), plan
        if not fused:
            assert plan == ["vt_pack"] + [t for p in own for t in p[1:]], plan
        for kind in ("randn", "peaked"):
            q, k, v = (_rnd(t, dtype) for t in _attn_inputs(S, D, kind, seed=S + Dh + len(kind)))
            dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
            got = ops.ext_attn_segments(dq, dk, dv, H, scale, inject, segs, no_split=no_split, **kw)
            assert torch.isfinite(got.float()).all()
            got32 = ops.ext_attn_segments(dq, dk, dv, H, scale, inject, segs, no_split=no_split,
                                          out_dtype=torch.float32, **kw)
            assert got32.dtype == torch.float32 and torch.equal(got32.to(dtype), got)
            f0 = 0
            for kv in segs:
                what = f"S{S} Dh{Dh} segs{segs} inject={inject} no_split={no_split} {kind} {dtype} frames {f0}..{f0 + kv - 1}"
                refs = attn_ref(_win(q, f0, f0 + kv), _win(k, f0, f0 + kv), _win(v, f0, f0 + kv), H, scale, inject,
                                need_sigma=False)
                err = assert_attn_close(_win(got, f0, f0 + kv), refs, what, dtype=dtype)
                assert_attn_close(_win(got32, f0, f0 + kv), refs, what + " fp32 out", dtype=dtype)
                alone = ops.ext_attn(_win(dq, f0, f0 + kv).contiguous(), _win(dk, f0, f0 + kv).contiguous(),
                                     _win(dv, f0, f0 + kv).contiguous(), H, scale, inject, no_split=no_split, **kw)
                same = torch.equal(_win(got, f0, f0 + kv), alone)
                print(f"{what}: max abs err {err:.3e}, equal to the segment's own call: {same}")
                if not fused or no_split:
                    assert same, what
                f0 += kv


def test_attention_one_segment_and_refusals():
    ops = _ops()
    S, H, Dh = 64, 2, 40
    q, k, v = (t.bfloat16().cuda() for t in _attn_inputs(S, H * Dh, "randn", 3))
    assert torch.equal(ops.ext_attn_segments(q, k, v, H, Dh ** -0.5, True, [K_ATTN]), ops.ext_attn(q, k, v, H, Dh ** -0.5, True))
    with pytest.raises(ValueError):
        ops.ext_attn_segments(q, k, v, H, Dh ** -0.5, True, [2, 2])
    with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_fwd_segments"):
        ops.ext_attn_segments(q, k, v, H, Dh ** -0.5, True, [2, 3], hints=_lib.TF_ATTN_MULTI_V)


# -------------------------------------------------------------------------------------------------------- propagation
N_PROP, C_PROP = 2, 5
# (S, D, family): the smallest S (ragged where the family allows it) at which EVERY search of a case -- the C = 4 / 5 call, the
# per-segment C = 1..4 calls, P = 1 and 2 -- takes the named kernel (ops.nn_plan on the CPU); more than one target panel
# everywhere, ragged last tiles where S allows
PROP_CASES = [
    (45, 320, "rb"), (96, 320, "rbs<TJ=2>"), (11808, 320, "rbs<TJ=4>"), (2180, 640, "glds"),
    (4040, 72, "wide"), (45, 72, "bk64"), (45, 640, "bk128"), (45, 1280, "deep"),
]
MASKS = [(0b00101, 0, 5), (0b10001, 0, 5), (0b0010, 1, 4)]      # (single_mask, slot0, chunks of the call)


def _form(tokens):
    return re.sub(r"\[.*", "", tokens[0])


def _groups(mask, C):
    """The per-segment calls of a run: (first chunk, chunks, first_single)."""
    cuts = [j for j in range(C) if (mask >> j) & 1]
    starts = sorted(set([0] + cuts))
    return [(j0, (starts[i + 1] if i + 1 < len(starts) else C) - j0, j0 in cuts) for i, j0 in enumerate(starts)]


def _prop_inputs(K, S, D, C, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ln = torch.nn.LayerNorm(D, elementwise_affine=False)
    piv = nf.spread_pivots(K, S, D, dtype, g)[0]               # row norms differ: a misplaced inv_norm changes the indices
    tgt = ln(torch.randn(C * N_PROP * S, D, generator=g, device="cuda")).to(dtype)
    kf = torch.randn(3 * K, S, D, generator=g, device="cuda").to(dtype)
    res = torch.randn(3 * C * N_PROP, S, D, generator=g, device="cuda").to(dtype)
    return tgt, piv, kf, res


def _per_segment(ops, tgt, piv, inv, kf, w, C, slot0, mask, res, norm):
    """The reference: every segment's chunks through today's calls, results put back into the run's layout."""
    n, (S, D) = N_PROP, piv.shape[1:]
    out = torch.empty(3, C, n, S, D, dtype=torch.float32, device="cuda")
    nout = torch.empty(3, C, n, S, D, dtype=kf.dtype, device="cuda")
    for j0, Cg, first in _groups(mask, C):
        single_alone = Cg == 1 and first       # its own pass stores the promoted 16-bit type (P = 1)
        r = ops.propagate_chunks(tgt[j0 * n * S:(j0 + Cg) * n * S], piv, inv, kf, w, n, Cg, slot0 + j0, first,
                                 res.view(3, C, n, S, D)[:, j0:j0 + Cg].reshape(3 * Cg * n, S, D),
                                 kf.dtype if single_alone else torch.float32, norm=norm)
        o, no = r if norm is not None else (r, None)
        out[:, j0:j0 + Cg] = o.float().view(3, Cg, n, S, D)
        if no is not None:
            nout[:, j0:j0 + Cg] = no.view(3, Cg, n, S, D)
    return out.view(3 * C * n, S, D), nout.view(3 * C * n, S, D)


def _decode_indices(ops, tgt, piv, inv, w, C, slot0, mask):
    """The indices the fused call found, read back through an index-coded fp32 keyframe cache: feature 0 of row r holds r in
    the even slots, feature 1 in the odd ones, so a chunk's two gathers land in different features: w * i1 and (1 - w) * i2."""
    n, (K, S, D) = N_PROP, piv.shape
    code = torch.zeros(3, K, S, D, dtype=torch.float32, device="cuda")
    rows = torch.arange(S, dtype=torch.float32, device="cuda")
    code[:, 0::2, :, 0] = rows
    code[:, 1::2, :, 1] = rows
    out = ops.propagate_chunks_segments(tgt, piv, inv, code.view(3 * K, S, D), w, n, C, slot0, mask, None, torch.float32)
    out = out.view(3, C, n, S, D)
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])
    idx = []
    for j in range(C):
        s = slot0 + j
        if (mask >> j) & 1:
            idx.append([out[0, j, :, :, s & 1].reshape(-1).round().long()])
        else:
            i1 = (out[0, j, :, :, s & 1] / w.view(n, 1)).reshape(-1).round().long()
            i2 = (out[0, j, :, :, (s - 1) & 1] / (1 - w).view(n, 1)).reshape(-1).round().long()
            idx.append([i1, i2])
    return idx


@pytest.mark.parametrize("S,D,family", PROP_CASES, ids=[f"{c[2]}-S{c[0]}-D{c[1]}" for c in PROP_CASES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_propagation_mask(S, D, family, dtype):
    ops = _ops()
    n, K = N_PROP, C_PROP
    gamma, beta = (torch.randn(D, device="cuda").to(dtype) for _ in range(2))
    w = orc.blend_weights(n, 1).cuda()
    for mask, slot0, C in MASKS:
        # precondition: one kernel form for the run's search and for every per-segment search
        forms = {_form(ops.nn_plan(n * S, S, D, 2, C))}
        forms |= {_form(ops.nn_plan(n * S, S, D, 1 if (Cg == 1 and first) else 2, Cg)) for _, Cg, first in _groups(mask, C)}
        assert forms == {family}, forms
        assert ops.propagate_segments_plan(n, C, S, D, mask) == ops.nn_plan(n * S, S, D, 2, C) + ["gather[branches=3]"]
        tgt, piv, kf, res = _prop_inputs(K, S, D, C, dtype, seed=S + D + mask)
        inv = ops.pivot_inv_norm(piv)
        got = ops.propagate_chunks_segments(tgt, piv, inv, kf, w, n, C, slot0, mask, res, torch.float32)
        ref, _ = _per_segment(ops, tgt, piv, inv, kf, w, C, slot0, mask, res, None)
        assert torch.equal(got, ref), f"mask {mask:#b}"
        # the fused-norm form: the unfused result, and its rows through ops.layer_norm
        norm = (gamma, beta, 1e-5, dtype)
        got_n = ops.propagate_chunks_segments(tgt, piv, inv, kf, w, n, C, slot0, mask, res, torch.float32, norm=norm)
        assert torch.equal(got_n[0], got), f"mask {mask:#b} (norm form, result)"
        assert torch.equal(got_n[1], ops.layer_norm(got, gamma, beta, 1e-5, dtype)[0]), f"mask {mask:#b} (norm)"
        assert torch.equal(got_n[1], _per_segment(ops, tgt, piv, inv, kf, w, C, slot0, mask, res, norm)[1]), f"mask {mask:#b}"
        # indices, tie-aware against the fp32 oracle (on the device: the similarity matrix of a large case is GBs)
        idx = _decode_indices(ops, tgt, piv, inv, w, C, slot0, mask)
        n_bad = n_diff = 0
        for j in range(C):
            ids = [slot0 + j] if (mask >> j) & 1 else [slot0 + j, slot0 + j - 1]
            sim = orc.batch_cosine_sim(tgt[j * n * S:(j + 1) * n * S].float(), piv[ids].float().reshape(-1, D))
            for s, g_ in zip(sim.chunk(len(ids), dim=1), idx[j]):
                assert int(g_.min()) >= 0 and int(g_.max()) < S
                r = s.argmax(dim=-1)
                rows = torch.arange(s.shape[0], device=s.device)
                diff = r != g_
                n_diff += int(diff.sum())
                n_bad += int((diff & (s[rows, r] - s[rows, g_] > NN_TAU)).sum())     # orc.nn_mismatch_tie_aware, on the device
        print(f"{family} S{S} D{D} {dtype} mask {mask:#b}: {n_diff} indices differ from the fp32 oracle, {n_bad} beyond a near-tie")
        assert n_bad == 0


@pytest.mark.parametrize("S,D,family", [(96, 320, "rbs<TJ=2>"), (45, 1280, "deep"), (2180, 640, "glds")])
def test_propagation_mask_0_and_1_are_the_chunk_form(S, D, family):
    ops = _ops()
    n, K, C = N_PROP, C_PROP, C_PROP
    w = orc.blend_weights(n, 1).cuda()
    norm = tuple(torch.randn(D, device="cuda").bfloat16() for _ in range(2)) + (1e-5, torch.bfloat16)
    for mask, slot0, Cc in ((1, 0, C), (0, 1, C - 1)):
        tgt, piv, kf, res = _prop_inputs(K, S, D, Cc, torch.bfloat16, seed=S + mask)
        inv = ops.pivot_inv_norm(piv)
        assert _form(ops.nn_plan(n * S, S, D, 2, Cc)) == family
        for nm in (None, norm):
            a = ops.propagate_chunks_segments(tgt, piv, inv, kf, w, n, Cc, slot0, mask, res, torch.float32, norm=nm)
            b = ops.propagate_chunks(tgt, piv, inv, kf, w, n, Cc, slot0, bool(mask), res, torch.float32, norm=nm)
            if nm is None:
                assert torch.equal(a, b)
            else:
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("S,D", [(320, 320), (300, 72), (300, 1280)])
def test_propagation_first_index_in_a_mid_call_single_chunk(S, D):
    """Exact duplicate pivot rows in the keyframe of a one-keyframe chunk in the MIDDLE of the call: bit-identical scores, the
    first index must win (torch.argmax) -- and the chunk must not look at keyframe slot0 + j - 1, which holds the targets
    themselves."""
    ops = _ops()
    n, K, C, mask = N_PROP, C_PROP, C_PROP, 0b00101
    tgt, piv, kf, res = _prop_inputs(K, S, D, C, torch.bfloat16, seed=S)
    piv[2, 200:300] = piv[2, 0:100]            # rows 200.. duplicate rows 0..
    piv[2, 150] = piv[2, 10]
    want = torch.tensor([5, 10, 99, 120, 160, 0, 42])
    tgt[2 * n * S:2 * n * S + len(want)] = piv[2, want]
    piv[1, :len(want)] = piv[2, want]          # the previous keyframe holds the targets too: a single chunk never reads it
    inv = ops.pivot_inv_norm(piv)
    w = orc.blend_weights(n, 1).cuda()
    idx = _decode_indices(ops, tgt, piv, inv, w, C, 0, mask)
    assert len(idx[2]) == 1 and idx[2][0][:len(want)].cpu().tolist() == want.tolist()
    got = ops.propagate_chunks_segments(tgt, piv, inv, kf, w, n, C, 0, mask, res, torch.float32)
    assert torch.equal(got, _per_segment(ops, tgt, piv, inv, kf, w, C, 0, mask, res, None)[0])


def test_propagation_argument_errors():
    ops = _ops()
    tgt, piv, kf, res = _prop_inputs(C_PROP, 45, 72, C_PROP, torch.bfloat16, seed=1)
    inv, w = ops.pivot_inv_norm(piv), orc.blend_weights(N_PROP, 1).cuda()
    with pytest.raises(ValueError):
        ops.propagate_chunks_segments(tgt, piv, inv, kf, w, N_PROP, C_PROP, 0, 1 << C_PROP, res, torch.float32)
    with pytest.raises(ValueError):       # chunk 0 would blend slot -1
        ops.propagate_chunks_segments(tgt, piv, inv, kf, w, N_PROP, C_PROP, 0, 0b00100, res, torch.float32)


# -------------------------------------------------------------------------------------------------------------- hooks
HOOK_SEGS = (2, 3)


def _hook_pipe():
    cfg = gc.BLOCKS_CFG
    torch.manual_seed(cfg["seed"])
    pipe = fd.FakePipeline(dims=cfg["dims"], heads=cfg["heads"], cross_dim=cfg["cross_dim"]).eval().cuda()
    tfu.register_extended_attention_pnp(pipe, [801])
    tfu.set_tokenflow(pipe.unet)
    tfu.register_time(pipe, 801)
    return pipe


@pytest.mark.parametrize("fp32_as", DTYPES)
@pytest.mark.parametrize("no_split", [True, False])
def test_hooks_segments_equal_two_single_clip_runs(monkeypatch, fp32_as, no_split):
    """One block (it injects at this step): a pivotal pass plus per-chunk passes, and a pivotal pass plus one all-chunks pass,
    against two separate single-clip runs of the same block, segment by segment.  Bit-identical in the bit-stable mode; in the
    default mode the segmented attention is held to the oracle per segment (the spy below, in both modes), and everything is
    bit-identical again where the joint launch has the geometry (KW, PREC) of the segments' own launches -- the only things
    its arithmetic depends on (include/tokenflow_hip.h)."""
    ops = _ops()
    monkeypatch.setattr(ops, "FP32_AS", fp32_as)
    monkeypatch.setattr(ops, "NO_SPLIT", no_split)
    K, n, S = sum(HOOK_SEGS), 2, 48
    attn_checked = []
    real = ops.ext_attn_segments

    def spy(q, k, v, heads, scale, inject, segments, **kw):
        out = real(q, k, v, heads, scale, inject, segments, **kw)
        qc, kc, vc = (t.float().cpu().contiguous() for t in (q, k, v))
        f0 = 0
        for kv in segments:
            refs = attn_ref(_winK(qc, K, f0, f0 + kv), _winK(kc, K, f0, f0 + kv), _winK(vc, K, f0, f0 + kv), heads, scale, inject,
                            need_sigma=False)
            assert_attn_close(_winK(out, K, f0, f0 + kv), refs, f"hooks frames {f0}..", dtype=q.dtype)
            f0 += kv
        attn_checked.append((tuple(segments), bool(inject), q.dtype))
        return out
    monkeypatch.setattr(ops, "ext_attn_segments", spy)

    def run(pipe, frames, x_piv, enc_piv, x_ch, enc_ch):
        """pivotal + per-chunk passes, then pivotal + one all-chunks pass; chunk outputs as [3, frames, n, S, D]"""
        blk = pipe.unet.up_blocks[2].attentions[0].transformer_blocks[0]
        with torch.no_grad():
            tfu.register_pivotal(pipe, True)
            piv = blk(x_piv, encoder_hidden_states=enc_piv)
            tfu.register_pivotal(pipe, False)
            chunks = []
            for c in range(frames):
                tfu.register_batch_idx(pipe, c)
                chunks.append(blk(_winK(x_ch, frames, c, c + 1).reshape(3 * n, S, -1),
                                  encoder_hidden_states=_winK(enc_ch, frames, c, c + 1).reshape(3 * n, 7, -1)).float())
            tfu.register_pivotal(pipe, True)
            piv2 = blk(x_piv, encoder_hidden_states=enc_piv)
            tfu.register_pivotal(pipe, False)
            tfu.register_batch_idx(pipe, range(frames))
            run_all = blk(x_ch.reshape(3 * frames * n, S, -1), encoder_hidden_states=enc_ch.reshape(3 * frames * n, 7, -1))
        assert torch.equal(piv, piv2)
        D_ = piv.shape[-1]
        return piv, torch.stack([c.view(3, n, S, D_) for c in chunks], dim=1), run_all.float().view(3, frames, n, S, D_)

    pipe = _hook_pipe()
    blk = pipe.unet.up_blocks[2].attentions[0].transformer_blocks[0]
    D, heads, cross = blk.norm1.normalized_shape[0], blk.attn1.heads, gc.BLOCKS_CFG["cross_dim"]
    g = torch.Generator().manual_seed(11)
    x_piv, enc_piv = torch.randn(3 * K, S, D, generator=g).cuda(), torch.randn(3 * K, 7, cross, generator=g).cuda()
    x_ch, enc_ch = torch.randn(3 * K, n * S, D, generator=g).cuda(), torch.randn(3 * K, n * 7, cross, generator=g).cuda()
    tfu.register_segments(pipe, HOOK_SEGS)
    got_piv, got_chunks, got_all = run(pipe, K, x_piv, enc_piv, x_ch, enc_ch)
    assert attn_checked == [(HOOK_SEGS, True, fp32_as)] * 2
    joint = ops.attn_segments_plan(K, HOOK_SEGS, S, heads, D // heads, True, dtype=fp32_as, no_split=no_split)
    own = [ops.attn_plan(k, k, S, heads, D // heads, True, dtype=fp32_as, no_split=no_split) for k in HOOK_SEGS]
    same_arith = all(len(p) == 1 and joint == [p[0][:-1] + f",sets={len(HOOK_SEGS)}]"] for p in own)
    assert same_arith or not no_split, (joint, own)
    f0 = 0
    for kv in HOOK_SEGS:      # a single-clip run of the same block on segment v's tensors alone
        ref_piv, ref_chunks, ref_all = run(_hook_pipe(), kv, _winK(x_piv, K, f0, f0 + kv), _winK(enc_piv, K, f0, f0 + kv),
                                           _winK(x_ch, K, f0, f0 + kv), _winK(enc_ch, K, f0, f0 + kv))
        if same_arith:
            assert torch.equal(_winK(got_piv, K, f0, f0 + kv), ref_piv), f"pivotal pass, frames {f0}.."
            assert torch.equal(got_chunks[:, f0:f0 + kv], ref_chunks), f"per-chunk passes, chunks {f0}.."
            assert torch.equal(got_all[:, f0:f0 + kv], ref_all), f"all-chunks pass, chunks {f0}.."
        f0 += kv


def _winK(t, K, f0, f1):
    return t.view(3, K, *t.shape[1:])[:, f0:f1].reshape(3 * (f1 - f0), *t.shape[1:])
