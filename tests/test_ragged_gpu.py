"""Ragged chunk runs on the GPU (tf_nn_gather_blend_chunks_ragged, `ops.propagate_chunks_ragged`): one search and one gather for
a run of chunks of unequal frame count.  The rows of chunk j must be what the one-chunk call computes on chunk j alone.

  * exact: the families of tests/nn_exact.py (integer scores: the indices do not depend on the kernel form), the whole output
    against the CPU reference of tests/ragged_forms.py as bit patterns -- bf16 and f16, with and without residual, the fused
    norm, one and two edits; the three large shapes with one family and the reference indices from the device;
  * identity: LayerNorm'ed random targets on pivots of different norms against per-chunk `ops.propagate` calls, `torch.equal` on
    the result and on the fused norm (every search of a case takes one kernel form: asserted through the plan entry points);
  * uniform: equal frame lists give the bits and the plan of `ops.propagate_chunks_segments` / `ops.propagate_chunks_edits`;
  * bounds: 64 chunks with bit 63 set, and the same list where the gather passes its grid cap and strides."""
import re

import pytest
import torch

from oracle import tokenflow_oracle as orc
from tests import nn_exact as nx
from tests import nn_families as nf
from tests import ragged_forms as rf

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
F32 = torch.float32


def _ops():
    from tokenflow_amd import ops
    return ops


def _same_bits(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    a, b = nx.bits(got.cpu()), nx.bits(ref.cpu())
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        pos = tuple(int(v) for v in bad[0])
        pytest.fail(f"{what}: {len(bad)} of {a.numel()} elements differ; first at {pos}: got {got.cpu()[pos].item()!r}, "
                    f"want {ref.cpu()[pos].item()!r}")


def _assert_forms(ops, frames, S, D, form, mask=0, E=1):
    """Precondition: the ragged search and every chunk's own search (one and two keyframes) take `form`."""
    plan = ops.propagate_ragged_plan(frames, S, D, mask, E)
    if len(set(frames)) > 1:
        assert re.fullmatch(re.escape(form) + r"\[splits=\d+,ragged\]", plan[0]), plan
        assert plan[1:] == [f"gather[branches={1 + 2 * E},ragged]"], plan
    for n in set(frames):
        for P in (1, 2):
            assert ops.nn_plan(n * S, S, D, P)[0].split("[")[0] == form, (n, P)
    return plan


def _tensors(K, F, S, D, nb, dtype, seed, huge=True):
    g = torch.Generator().manual_seed(seed)
    kf = torch.randn(nb * K, S, D, generator=g).to(dtype)
    res = torch.randn(nb * F, S, D, generator=g).to(dtype)
    kf[K + 1] = nx.edge_frame(S, D, dtype, 0, huge)          # branch 1, slot 1
    res[F] = nx.edge_frame(S, D, dtype, 3, huge)             # branch 1, frame 0
    return kf, res


def _norm(D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return ((1 + 0.2 * torch.randn(D, generator=g)).to(dtype).cuda(), (0.1 * torch.randn(D, generator=g)).to(dtype).cuda(), 1e-5,
            dtype)


def _check_norm(ops, got, ref, norm, what):
    out, nout = got
    _same_bits(out, ref, what)
    _same_bits(nout, ops.layer_norm(out, norm[0], norm[1], norm[2], norm[3])[0], what + " (norm vs ops.layer_norm)")


# --------------------------------------------------------------------------------------------------------------- exact
SMALL_CASES = [(S, D, form, fr) for S, D, form in rf.SMALL for fr in rf.SMALL_FRAMES]


@pytest.mark.parametrize("S,D,form,frames", SMALL_CASES, ids=[f"{c[2]}-S{c[0]}-D{c[1]}-{'_'.join(map(str, c[3]))}" for c in SMALL_CASES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_small(S, D, form, frames, dtype):
    ops = _ops()
    C, F = len(frames), sum(frames)
    w = rf.weights(frames).cuda()
    kf7, res7 = _tensors(C + 1, F, S, D, 5, dtype, seed=S + D + F)
    kf3, res3 = kf7.view(5, -1, S, D)[:3].reshape(-1, S, D), res7.view(5, -1, S, D)[:3].reshape(-1, S, D)
    # the fused-norm calls: edge values without the huge one ((x - mean)^2 of such a row overflows fp32)
    kn7, rn7 = _tensors(C + 1, F, S, D, 5, dtype, seed=S + D + F + 1, huge=False)
    kn3, rn3 = kn7.view(5, -1, S, D)[:3].reshape(-1, S, D), rn7.view(5, -1, S, D)[:3].reshape(-1, S, D)
    norm = _norm(D, dtype, D)
    count = 0
    for family in nx.FAMILIES:
        rg = rf.Ragged(frames, S, D, family)
        tgt = rg.targets("cuda", dtype)
        for mask, slot0 in rf.masks(C):
            _assert_forms(ops, frames, S, D, form, mask)
            want = rg.indices(slot0, mask)
            ref = rf.reference(kf3, frames, slot0, mask, want, res3, F32, 3)
            for scaled in (False, True):
                piv = rg.pivots("cuda", dtype, scaled)
                inv = ops.pivot_inv_norm(piv)
                what = f"{form} S{S} D{D} {frames} {family}{' scaled' if scaled else ''} {dtype} mask {mask:#b}"
                got = ops.propagate_chunks_ragged(tgt, piv, inv, kf3.cuda(), w, frames, slot0, mask, res3.cuda(), F32)
                _same_bits(got, ref, what)
                count += 1
            if family != "pool":
                continue
            # the other gather forms, on the scaled pool family: no residual, the model dtype out, the fused norm, two edits
            got = ops.propagate_chunks_ragged(tgt, piv, inv, kf3.cuda(), w, frames, slot0, mask, None, F32)
            _same_bits(got, rf.reference(kf3, frames, slot0, mask, want, None, F32, 3), what + " no residual")
            got = ops.propagate_chunks_ragged(tgt, piv, inv, kf3.cuda(), w, frames, slot0, mask, res3.cuda(), dtype)
            _same_bits(got, rf.reference(kf3, frames, slot0, mask, want, res3, dtype, 3), what + " out=model dtype")
            got = ops.propagate_chunks_ragged(tgt, piv, inv, kn3.cuda(), w, frames, slot0, mask, rn3.cuda(), F32, norm=norm)
            _check_norm(ops, got, rf.reference(kn3, frames, slot0, mask, want, rn3, F32, 3), norm, what + " fused norm")
            if mask <= 1:
                _assert_forms(ops, frames, S, D, form, mask, 2)
                ref5 = rf.reference(kf7, frames, slot0, mask, want, res7, F32, 5)
                got = ops.propagate_chunks_ragged(tgt, piv, inv, kf7.cuda(), w, frames, slot0, mask, res7.cuda(), F32, n_edits=2)
                _same_bits(got, ref5, what + " two edits")
                got = ops.propagate_chunks_ragged(tgt, piv, inv, kn7.cuda(), w, frames, slot0, mask, rn7.cuda(), F32, n_edits=2,
                                                  norm=norm)
                _check_norm(ops, got, rf.reference(kn7, frames, slot0, mask, want, rn7, F32, 5), norm,
                            what + " two edits, fused norm")
    assert count == 4 * 2 * len(rf.masks(C))


LARGE_CASES = [(S, D, form, fr) for S, D, form in rf.LARGE for fr in rf.LARGE_FRAMES]


@pytest.mark.parametrize("S,D,form,frames", LARGE_CASES, ids=[f"{c[2]}-S{c[0]}-D{c[1]}-{'_'.join(map(str, c[3]))}" for c in LARGE_CASES])
def test_exact_large(S, D, form, frames):
    """The search forms that need a large S: the pool family in bf16, one-keyframe chunks at the front and in the middle; the
    exact indices come from the fp64 reference on the device."""
    ops = _ops()
    dtype = torch.bfloat16
    C, F = len(frames), sum(frames)
    mask, slot0 = rf.masks(C)[1]
    assert mask not in (0, 1)
    _assert_forms(ops, frames, S, D, form, mask)
    rg = rf.Ragged(frames, S, D, "pool", device="cuda")
    kf, res = _tensors(C + 1, F, S, D, 3, dtype, seed=S + D + F)
    piv = rg.pivots("cuda", dtype, True)
    got = ops.propagate_chunks_ragged(rg.targets("cuda", dtype), piv, ops.pivot_inv_norm(piv), kf.cuda(), rf.weights(frames).cuda(),
                                      frames, slot0, mask, res.cuda(), F32)
    _same_bits(got, rf.reference(kf, frames, slot0, mask, rg.indices(slot0, mask), res, F32, 3), f"{form} S{S} D{D} {frames}")


# ------------------------------------------------------------------------------------------------------------ identity
def _identity_inputs(frames, S, D, nb, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    F, K = sum(frames), len(frames) + 1
    ln = torch.nn.LayerNorm(D, elementwise_affine=False)
    piv = nf.spread_pivots(K, S, D, dtype, g)[0]               # row norms differ: a misplaced inv_norm changes the indices
    tgt = ln(torch.randn(F * S, D, generator=g, device="cuda")).to(dtype)
    kf = torch.randn(nb * K, S, D, generator=g, device="cuda").to(dtype)
    res = torch.randn(nb * F, S, D, generator=g, device="cuda").to(dtype)
    return tgt, piv, kf, res


def _per_chunk(ops, tgt, piv, inv, kf, frames, slot0, mask, res, norm, E=1):
    """The reference: every chunk through today's one-chunk call with ITS n and ITS weights, put back into the run's layout."""
    nb, (S, D), F, st = 1 + 2 * E, piv.shape[1:], sum(frames), rf.starts(frames)
    out = torch.empty(nb, F, S, D, dtype=F32, device="cuda")
    nout = torch.empty(nb, F, S, D, dtype=kf.dtype, device="cuda")
    for j, n in enumerate(frames):
        single = bool((mask >> j) & 1)
        ids = [slot0 + j] if single else [slot0 + j, slot0 + j - 1]
        w = orc.blend_weights(n, 1).cuda()
        r_j = res.view(nb, F, S, D)[:, st[j]:st[j + 1]].reshape(nb * n, S, D)
        t_j = tgt[st[j] * S:st[j + 1] * S]
        od = kf.dtype if single else F32              # the one-keyframe chunk's own pass stores the promoted 16-bit type
        if E == 1:
            r = ops.propagate(t_j, piv, inv, ids, kf, None if single else w, n, r_j, od, norm=norm)
        else:
            r = ops.propagate_chunks_edits(t_j, piv, inv, kf, w, n, 1, slot0 + j, single, r_j, od, E, norm=norm)
        o, no = r if norm is not None else (r, None)
        out[:, st[j]:st[j + 1]] = o.float().view(nb, n, S, D)
        if no is not None:
            nout[:, st[j]:st[j + 1]] = no.view(nb, n, S, D)
    return out.view(nb * F, S, D), nout.view(nb * F, S, D)


ID_CASES = SMALL_CASES + LARGE_CASES


@pytest.mark.parametrize("S,D,form,frames", ID_CASES, ids=[f"{c[2]}-S{c[0]}-D{c[1]}-{'_'.join(map(str, c[3]))}" for c in ID_CASES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_with_the_per_chunk_calls(S, D, form, frames, dtype):
    ops = _ops()
    C = len(frames)
    w = rf.weights(frames).cuda()
    norm = _norm(D, dtype, S)
    for mask, slot0 in rf.masks(C):
        for E in (1, 2):
            if E > 1 and (mask > 1 or S > 1000):
                continue
            _assert_forms(ops, frames, S, D, form, mask, E)
            tgt, piv, kf, res = _identity_inputs(frames, S, D, 1 + 2 * E, dtype, seed=S + D + mask + E)
            inv = ops.pivot_inv_norm(piv)
            what = f"{form} S{S} D{D} {frames} {dtype} mask {mask:#b} E={E}"
            got = ops.propagate_chunks_ragged(tgt, piv, inv, kf, w, frames, slot0, mask, res, F32, n_edits=E)
            ref, _ = _per_chunk(ops, tgt, piv, inv, kf, frames, slot0, mask, res, None, E)
            assert torch.equal(got, ref), what
            got_n = ops.propagate_chunks_ragged(tgt, piv, inv, kf, w, frames, slot0, mask, res, F32, n_edits=E, norm=norm)
            assert torch.equal(got_n[0], got), what + " (norm form, result)"
            assert torch.equal(got_n[1], _per_chunk(ops, tgt, piv, inv, kf, frames, slot0, mask, res, norm, E)[1]), what + " (norm)"


# ------------------------------------------------------------------------------------------------------------- uniform
@pytest.mark.parametrize("S,D,form", [(96, 320, "rbs<TJ=2>"), (45, 1280, "deep"), (2180, 640, "glds")])
def test_uniform_frames_are_todays_calls(S, D, form):
    ops = _ops()
    n, C, dtype = 2, 4, torch.bfloat16
    frames = [n] * C
    w = orc.blend_weights(n, 1).cuda()
    w_run = rf.weights(frames).cuda()
    norm = _norm(D, dtype, S)
    for mask, slot0 in ((0b0101, 0), (1, 0), (0b0010, 1)):
        assert ops.propagate_ragged_plan(frames, S, D, mask) == ops.propagate_segments_plan(n, C, S, D, mask)
        tgt, piv, kf, res = _identity_inputs(frames, S, D, 3, dtype, seed=S + mask)
        inv = ops.pivot_inv_norm(piv)
        for nm in (None, norm):
            a = ops.propagate_chunks_ragged(tgt, piv, inv, kf, w_run, frames, slot0, mask, res, F32, norm=nm)
            b = ops.propagate_chunks_segments(tgt, piv, inv, kf, w, n, C, slot0, mask, res, F32, norm=nm)
            assert torch.equal(a, b) if nm is None else (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])), (mask, nm is None)
    for first, slot0 in ((True, 0), (False, 1)):
        assert ops.propagate_ragged_plan(frames, S, D, int(first), 2) == ops.propagate_edits_plan(n, C, S, D, first, 2)
        tgt, piv, kf, res = _identity_inputs(frames, S, D, 5, dtype, seed=S + 7)
        inv = ops.pivot_inv_norm(piv)
        for nm in (None, norm):
            a = ops.propagate_chunks_ragged(tgt, piv, inv, kf, w_run, frames, slot0, int(first), res, F32, n_edits=2, norm=nm)
            b = ops.propagate_chunks_edits(tgt, piv, inv, kf, w, n, C, slot0, first, res, F32, 2, norm=nm)
            assert torch.equal(a, b) if nm is None else (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])), (first, nm is None)


# -------------------------------------------------------------------------------------------------------------- bounds
GRID_CAP = 256 * 16                   # gather_blend.hip: `if (blocks > 256 * 16) blocks = 256 * 16` in launch_gb and launch_gbn


@pytest.mark.parametrize("D,form", [(320, "rb"), (1280, "wide")])
@pytest.mark.parametrize("dtype", DTYPES)
def test_64_chunks_and_the_grid_cap(D, form, dtype):
    """C = 64, the last table entries and bit 63 in use.  At D = 1280 the 7 920 tokens x 160 pieces pass the plain gather's
    4 096 x 256 threads and the 23 760 rows the fused-norm gather's 4 096 x 4 (64 lanes per row): a second trip through the
    grid-stride loops with the per-thread chunk lookup."""
    ops = _ops()
    S, C = 45, 64
    frames = [(1, 2, 3, 5)[j % 4] for j in range(C)]
    F = sum(frames)
    mask, slot0 = (1 << 63) | 1, 0
    pieces, rows = F * S * (D // 8), 3 * F * S
    assert (F, F * S) == (176, 7920)
    if D == 1280:
        assert pieces == 1267200 and pieces > GRID_CAP * 256, "the plain launch does not stride"
        assert rows == 23760 and rows > GRID_CAP * 4 * (64 // 64), "the fused-norm launch does not stride"
    else:
        assert pieces <= GRID_CAP * 256 and rows <= GRID_CAP * 4 * (64 // 16)
    # integer scores: the indices do not depend on the form.  (64 chunks fill the chip: at D = 1280 the rule takes the
    # 128-target panels of `wide`, where a chunk of these alone takes `deep`.)
    plan = ops.propagate_ragged_plan(frames, S, D, mask)
    assert plan == [f"{form}[splits=1,ragged]", "gather[branches=3,ragged]"], plan
    rg = rf.Ragged(frames, S, D, "pool")
    kf, res = _tensors(C + 1, F, S, D, 3, dtype, seed=D, huge=False)
    want = rg.indices(slot0, mask)
    ref = rf.reference(kf, frames, slot0, mask, want, res, F32, 3)
    piv = rg.pivots("cuda", dtype, True)
    inv, tgt, w = ops.pivot_inv_norm(piv), rg.targets("cuda", dtype), rf.weights(frames).cuda()
    got = ops.propagate_chunks_ragged(tgt, piv, inv, kf.cuda(), w, frames, slot0, mask, res.cuda(), F32)
    _same_bits(got, ref, f"D{D} {dtype} plain")
    norm = _norm(D, dtype, D)
    got = ops.propagate_chunks_ragged(tgt, piv, inv, kf.cuda(), w, frames, slot0, mask, res.cuda(), F32, norm=norm)
    _check_norm(ops, got, ref, norm, f"D{D} {dtype} fused norm")


def test_argument_errors():
    ops = _ops()
    frames, S, D = [3, 1, 2], 45, 72
    tgt, piv, kf, res = _identity_inputs(frames, S, D, 3, torch.bfloat16, seed=1)
    inv, w = ops.pivot_inv_norm(piv), rf.weights(frames).cuda()
    with pytest.raises(ValueError):
        ops.propagate_chunks_ragged(tgt, piv, inv, kf, w, frames, 0, 1 << 3, res, F32)
    with pytest.raises(ValueError):       # chunk 0 would blend slot -1
        ops.propagate_chunks_ragged(tgt, piv, inv, kf, w, frames, 0, 0b100, res, F32)
    with pytest.raises(ValueError):       # one weight per frame of the run
        ops.propagate_chunks_ragged(tgt, piv, inv, kf, w[:3], frames, 1, 0, res, F32)
    with pytest.raises(ValueError):
        ops.propagate_chunks_ragged(tgt, piv, inv, kf, w, [3, 0, 3], 1, 0, res, F32)
    with pytest.raises(ValueError):       # segments and multi-edit batches do not combine
        ops.propagate_chunks_ragged(tgt, piv, inv, kf, w, frames, 0, 0b101, res, F32, n_edits=2)


# --------------------------------------------------------------------------------------------------------------- hooks
HOOK_FRAMES = (3, 1, 2, 2, 4)


def _tensors_of(res):
    return tuple(t.float() for t in (res if isinstance(res, tuple) else (res,)))


@pytest.mark.parametrize("segs", [None, (2, 3)], ids=["plain", "segments"])
def test_hooks_ragged_run_equals_the_per_chunk_passes(segs):
    """One block: a pivotal pass, one pass per chunk -- each with its own frame count, what a user has without
    `register_chunk_frames` -- and then the registered run passes.  Bit for bit at two levels:
      * what the propagation returns to the block (the residual stream, and the fused norm where it rides along): every chunk;
      * the block's output: every chunk for which torch's own Linear layers are batch-invariant.  The rest of the block is
        torch GEMMs on [3 n S, D] rows, and for few rows (one frame of 48 tokens: 144 rows) torch takes another GEMM kernel than
        for the run's 1 728, with sums in another order; that is measured here on the block's first feed-forward Linear, per row
        count, and asserted to hold for every chunk of two frames and more."""
    import tokenflow_utils as tfu
    from oracle import golden_cases as gc
    from tests import fake_diffusers as fd
    ops = _ops()
    cfg = gc.BLOCKS_CFG
    torch.manual_seed(cfg["seed"])
    pipe = fd.FakePipeline(dims=cfg["dims"], heads=cfg["heads"], cross_dim=cfg["cross_dim"]).eval().cuda()
    tfu.register_extended_attention_pnp(pipe, [801])
    tfu.set_tokenflow(pipe.unet)
    tfu.register_time(pipe, 801)
    tfu.register_segments(pipe, segs)
    blk = pipe.unet.up_blocks[2].attentions[0].transformer_blocks[0]
    K, S, D, cross = len(HOOK_FRAMES), 48, blk.norm1.normalized_shape[0], cfg["cross_dim"]
    g = torch.Generator().manual_seed(11)
    x_piv, enc_piv = torch.randn(3 * K, S, D, generator=g).cuda(), torch.randn(3 * K, 7, cross, generator=g).cuda()
    xs = {c: (torch.randn(3 * n, S, D, generator=g).cuda(), torch.randn(3 * n, 7, cross, generator=g).cuda())
          for c, n in enumerate(HOOK_FRAMES)}
    lin = [m for m in blk.ff.modules() if isinstance(m, torch.nn.Linear)][0]
    probe = torch.randn(3 * sum(HOOK_FRAMES) * S, D, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")
    seen = []
    real = {name: getattr(ops, name) for name in ("propagate", "propagate_chunks_ragged")}

    def spy(name):
        def fn(*a, **kw):
            res = real[name](*a, **kw)
            seen.append((name, tuple(a[5]) if name == "propagate_chunks_ragged" else None, _tensors_of(res)))
            return res
        return fn
    try:
        for name in real:
            setattr(ops, name, spy(name))
        with torch.no_grad():
            tfu.register_pivotal(pipe, True)
            blk(x_piv, encoder_hidden_states=enc_piv)
            tfu.register_pivotal(pipe, False)
            per_chunk, per_op = {}, {}
            for c in range(K):
                tfu.register_batch_idx(pipe, c)
                per_chunk[c] = blk(xs[c][0], encoder_hidden_states=xs[c][1]).float()
                assert seen[-1][0] == "propagate"
                per_op[c] = seen[-1][2]
            tfu.register_chunk_frames(pipe, HOOK_FRAMES)
            invariant = 0
            for run in (range(0, 5), range(1, 4), range(2, 5)):
                fr = [HOOK_FRAMES[c] for c in run]
                F = sum(fr)
                # precondition of bit-equality: one kernel form for the run's search and for every chunk's own search
                forms = {ops.propagate_ragged_plan(fr, S, D)[0].split("[")[0]}
                forms |= {ops.nn_plan(n * S, S, D, P)[0].split("[")[0] for n in fr for P in (1, 2)}
                assert len(forms) == 1, forms
                x = torch.cat([xs[c][0].view(3, HOOK_FRAMES[c], S, D) for c in run], dim=1).reshape(-1, S, D)
                enc = torch.cat([xs[c][1].view(3, HOOK_FRAMES[c], 7, cross) for c in run], dim=1).reshape(-1, 7, cross)
                tfu.register_batch_idx(pipe, run)
                out = blk(x, encoder_hidden_states=enc).float().view(3, F, S, D)
                assert seen[-1][:2] == ("propagate_chunks_ragged", tuple(fr)), seen[-1][:2]
                run_op = seen[-1][2]
                full = lin(probe[:3 * F * S])
                f0 = 0
                for c in run:
                    n = HOOK_FRAMES[c]
                    assert len(run_op) == len(per_op[c])
                    for a, b in zip(run_op, per_op[c]):
                        assert torch.equal(a.view(3, F, S, D)[:, f0:f0 + n], b.view(3, n, S, D)), (run, c, "propagation")
                    if torch.equal(lin(probe[:3 * n * S]), full[:3 * n * S]):
                        invariant += 1
                        assert torch.equal(out[:, f0:f0 + n].reshape(-1, S, D), per_chunk[c]), (run, c, "block")
                    else:
                        assert n < 2, f"torch's Linear is not batch-invariant at {3 * n * S} rows"
                    f0 += n
            assert invariant >= sum(1 for run in (range(0, 5), range(1, 4), range(2, 5)) for c in run if HOOK_FRAMES[c] >= 2)
    finally:
        for name, fn in real.items():
            setattr(ops, name, fn)
    assert [s_[0] for s_ in seen].count("propagate_chunks_ragged") == 3
