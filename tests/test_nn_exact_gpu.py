"""The NN search and the propagation family on inputs whose scores are exact (tests/nn_exact.py): every index of every target
and every bit of every output is decided, nothing is tie-aware.

  * search: every NN form of tests/kernel_forms.CASES (launch plan asserted first), bf16 and f16, the dense / sparse / pool /
    roll-call families and their scaled variants.  C = 1 cases: `ops.nn_search` must equal the exact first-index reference on
    EVERY target (`torch.equal`; the reference is fp64 dot products in row blocks on the device).  C > 1 cases run
    `ops.propagate_chunks` (first_single) on an index-coded fp32 keyframe cache (feature 0 of row r holds r in the even slots,
    feature 1 in the odd ones, w = 1/2: both indices of a target decode exactly from one call).  A mismatch names the first
    wrong (chunk, keyframe, target, got, want) and where the two rows sit in the kernel's tiles and splits.
    Preconditions with assertions of their own: all rows of the unscaled pivots have ONE fp32 inv_norm, and the inv_norm of
    the scaled rows is that value times 2^-e bit for bit;
  * propagation: `propagate` (P = 1, 2), `propagate_chunks` (with / without first_single), `propagate_chunks_segments` (the masks
    of tests/test_segments_gpu.py), `propagate_chunks_edits` (E = 1, 3; the chunk form and the one-keyframe chunk alone), residual
    None / model dtype / fp32, output fp32 / model dtype -- against `nx.propagation_reference`: the reference's own op order on
    the CPU on the exact indices, compared as bit patterns (-0 and +0 differ).  kf_out and residual are N(0,1) with one frame
    of edge values (+-0, the smallest normal, a subnormal, half the largest finite value);
  * fused norm: the same calls with `norm=` at every mapping boundary of gather_blend_norm_kernel (pieces per lane: D = 384 / 392,
    768 / 776; lanes per row: 512 / 520, 1024 / 1032; the largest fusable D = 1536) beside the model's D: result bit-equal to the
    reference, norm bit-equal to `ops.layer_norm` of the result and within the bound of test_layer_norm_vs_torch_fp32 of torch's
    fp32 layer_norm of the stored result (edge values without the huge one: (x - mean)^2 of such a row overflows fp32 in
    torch as well);
  * grid stride: two launches past the 4096-workgroup cap of the gather kernels, every output element against the reference.
"""
import pytest
import torch

from oracle import tokenflow_oracle as orc
from tests import kernel_forms as kf
from tests import nn_exact as nx
from tests.test_kernels_gpu import layer_norm_bound
from tests.test_segments_gpu import MASKS, PROP_CASES

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _ops():
    from tokenflow_amd import ops
    return ops


def _inv_norm(ops, inp, piv, scaled, base):
    """ops.pivot_inv_norm with the family's exactness preconditions asserted as such."""
    inv = ops.pivot_inv_norm(piv)
    if not scaled:
        assert bool((inv == inv.flatten()[0]).all()), \
            "precondition: tf_pivot_inv_norm is not one fp32 value for rows of one norm"
    else:
        assert torch.equal(inv, base * inp.scale(inv.device)), \
            "precondition: inv_norm of rows scaled by 2^e is not 2^-e times the unscaled value bit for bit"
    return inv


def _exact(tgt8, piv8, slots):
    """[first_argmax per searched slot] of one chunk's int8 targets, on the tensors' device."""
    return [nx.first_argmax(tgt8, piv8[s], block=8192) for s in slots]


def _mismatch(what, form, token, S, got, want):
    bad = (got != want).nonzero().flatten()
    if bad.numel():
        t = int(bad[0])
        g, w_ = int(got[t]), int(want[t])
        pytest.fail(f"{what}: {bad.numel()} of {want.numel()} targets wrong; first: target {t} got {g}, want {w_}\n"
                    f"  got  {nx.locate(form, token, S, g)}\n  want {nx.locate(form, token, S, w_)}")


def _decode(ops, tgt, piv, inv, n, C):
    """The indices propagate_chunks (first_single) found: [[i1] for chunk 0, [i1, i2] for chunk j > 0], int64 [n*S] each."""
    K, S, D = piv.shape
    code = torch.zeros(3, K, S, D, dtype=torch.float32, device="cuda")
    rows = torch.arange(S, dtype=torch.float32, device="cuda")
    code[:, 0::2, :, 0] = rows
    code[:, 1::2, :, 1] = rows
    w = torch.full((n,), 0.5, device="cuda")
    out = ops.propagate_chunks(tgt, piv, inv, code.view(3 * K, S, D), w, n, C, 0, True, None, torch.float32).view(3, C, n * S, D)
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])
    idx = [[out[0, 0, :, 0].long()]]
    for j in range(1, C):
        idx.append([(2 * out[0, j, :, j & 1]).long(), (2 * out[0, j, :, (j - 1) & 1]).long()])
    return idx


# ------------------------------------------------------------------------------------------------------------- search
@pytest.mark.parametrize("form,i", nx.NN_CASES, ids=[f"{f}-{i}" for f, i in nx.NN_CASES])
@pytest.mark.parametrize("family", nx.FAMILIES)
def test_search_exact(form, i, family):
    ops = _ops()
    c = kf.CASES[form][i]
    plan = kf.plan(ops, c)
    assert form in [kf.form(t) for t in plan], plan
    token = [t for t in plan if kf.form(t) == form][0]
    n_tgt, S, C = c["n_tgt"], c["S"], c["C"]
    inp = nx.Inputs.of_case(c, family)
    chunks = inp.chunks
    piv8 = inp.piv.cuda()
    tgt8 = torch.cat([inp.targets(j, "cuda") for j in range(C)])
    want = [_exact(tgt8[j * n_tgt:(j + 1) * n_tgt], piv8, chunks[j]) for j in range(C)]
    if family == "rollcall":      # every index 0 .. S-1 of every searched slot is the answer of its own target
        for j in range(C):
            for s, wnt in zip(chunks[j], want[j]):
                assert torch.equal(wnt.cpu(), inp.rollcall_want(j, s)) and len(torch.unique(wnt)) == S
    for dtype in DTYPES:
        tgt = tgt8.to(dtype)
        base = None
        for scaled in (False, True):
            piv = inp.pivots("cuda", dtype, scaled)
            inv = _inv_norm(ops, inp, piv, scaled, base)
            base = inv if not scaled else base
            what = f"{form}-{i} {family}{' scaled' if scaled else ''} {dtype}"
            if C == 1:
                got = ops.nn_search(tgt, piv, inv, chunks[0]).long()
                for p, s in enumerate(chunks[0]):
                    _mismatch(f"{what} keyframe {s}", form, token, S, got[p], want[0][p])
                    assert torch.equal(got[p], want[0][p])
            else:
                got = _decode(ops, tgt, piv, inv, n_tgt // S, C)
                for j in range(C):
                    for p, s in enumerate(chunks[j]):
                        _mismatch(f"{what} chunk {j} keyframe {s}", form, token, S, got[j][p], want[j][p])
                        assert torch.equal(got[j][p], want[j][p])


# -------------------------------------------------------------------------------------------------------- propagation
K_PROP, NB_MAX = 5, 7
UNIVERSAL = [[j, j - 1] if j else [0] for j in range(K_PROP)]     # chunk j of the video: slots j and j - 1


class Prop:
    """One shape's search inputs (chunk j of a 5-chunk video matches slot j and j - 1; a call takes a run of these chunks), the
    cached outputs / residual of 7 branches, and the exact indices of every (chunk, slot) a call can search."""

    def __init__(self, S, D, n, family, dtype, huge=True, device_ref=False):
        self.S, self.D, self.n, self.dtype = S, D, n, dtype
        self.inp = inp = nx.Inputs(K_PROP, S, D, n * S, UNIVERSAL, family, seed=S * 7 + D + n)
        dev = "cuda" if device_ref else "cpu"
        tgt8 = [inp.targets(j, dev) for j in range(K_PROP)]
        piv8 = inp.piv.to(dev)
        assert all(not torch.equal(piv8[a], piv8[b]) for a in range(K_PROP) for b in range(a)), "two slots are equal"
        self.want = {(j, s): nx.first_argmax(tgt8[j], piv8[s]).cpu() for j in range(K_PROP) for s in (j, j - 1) if s >= 0}
        self.tgt = torch.cat(tgt8).to(dtype).cuda()
        self.piv = inp.pivots("cuda", dtype, scaled=True)
        self.w = orc.blend_weights(n, 1)
        g = torch.Generator().manual_seed(S + D)
        self.kf = torch.randn(NB_MAX, K_PROP, S, D, generator=g).to(dtype)
        self.res = torch.randn(NB_MAX, K_PROP * n, S, D, generator=g).to(dtype)
        self.kf[1, 1] = nx.edge_frame(S, D, dtype, 0, huge)
        self.res[1, ::n] = nx.edge_frame(S, D, dtype, 3, huge)          # frame 0 of every chunk, branch 1

    def args(self, nb, j0, C, res_kind):
        """(tgt, kf_out, residual) of a call over chunks j0 .. j0 + C - 1 and nb branches: (device, cpu) pairs."""
        n, S, D = self.n, self.S, self.D
        kf = self.kf[:nb].reshape(nb * K_PROP, S, D)
        res = None
        if res_kind is not None:
            res = self.res[:nb, j0 * n:(j0 + C) * n].reshape(nb * C * n, S, D).to(res_kind)
        return self.tgt[j0 * n * S:(j0 + C) * n * S], (kf.cuda(), kf), (None if res is None else res.cuda(), res)

    def reference(self, nb, j0, slots, res, out_dtype):
        want = [[self.want[(j0 + j, s)] for s in ss] for j, ss in enumerate(slots)]
        return nx.propagation_reference(self.kf[:nb].reshape(nb * K_PROP, self.S, self.D), slots, want, self.w, res, out_dtype,
                                        nb, self.n)


def _same_bits(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    a, b = nx.bits(got.cpu()), nx.bits(ref)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        pos = tuple(int(v) for v in bad[0])
        pytest.fail(f"{what}: {len(bad)} of {a.numel()} elements differ; first at {pos}: got {got.cpu()[pos].item()!r} "
                    f"({int(a[pos]):#x}), want {ref[pos].item()!r} ({int(b[pos]):#x})")


def _slots(j0, C, mask):
    return [[j0 + j] if (mask >> j) & 1 else [j0 + j, j0 + j - 1] for j in range(C)]


def _calls(ops, pr, inv, norm=None):
    """Every call form on one shape: yields (what, result or (result, norm), reference).  norm: the fusable calls only."""
    n, S, D, dt, w = pr.n, pr.S, pr.D, pr.dtype, pr.w.cuda()
    f32 = torch.float32
    kinds = [dt] if norm is not None else [None, dt, f32]
    fam = nx.kernel_of(ops.nn_plan(n * S, S, D, 2, 3)[0])
    kw = {} if norm is None else {"norm": norm}
    for rk in kinds:
        promoted = dt if rk is None else torch.promote_types(dt, rk)
        # ---- propagate, one and two keyframes
        for ids, j in (([1], 1), ([2, 1], 2)):
            P = len(ids)
            assert nx.kernel_of(ops.nn_plan(n * S, S, D, P)[0]) == fam
            tgt, (kf, kf_c), (res, res_c) = pr.args(3, j, 1, rk)
            for od in ([promoted] if P == 1 else [f32] if norm is not None else [f32, dt]):
                got = ops.propagate(tgt, pr.piv, inv, ids, kf, w if P == 2 else None, n, res, od, **kw)
                yield f"propagate P={P} res={rk} out={od}", got, pr.reference(3, j, [ids], res_c, od)
        # ---- propagate_chunks with and without first_single
        for first, j0, C in ((True, 0, 3), (False, 1, 4)):
            assert ops.propagate_segments_plan(n, C, S, D, int(first)) == ops.nn_plan(n * S, S, D, 2, C) + ["gather[branches=3]"]
            tgt, (kf, _), (res, res_c) = pr.args(3, j0, C, rk)
            for od in ([f32] if norm is not None or rk != dt else [f32, dt]):
                got = ops.propagate_chunks(tgt, pr.piv, inv, kf, w, n, C, j0, first, res, od, **kw)
                yield f"propagate_chunks first_single={first} res={rk} out={od}", got, \
                    pr.reference(3, j0, _slots(j0, C, int(first)), res_c, od)
        if rk == f32:
            continue
        # ---- keyframe segments
        for mask, j0, C in MASKS:
            plan = ops.propagate_segments_plan(n, C, S, D, mask)
            assert plan[-1] == "gather[branches=3]" and nx.kernel_of(plan[0]) == fam, plan
            tgt, (kf, _), (res, res_c) = pr.args(3, j0, C, rk)
            got = ops.propagate_chunks_segments(tgt, pr.piv, inv, kf, w, n, C, j0, mask, res, f32, **kw)
            yield f"propagate_chunks_segments mask={mask:#b} res={rk}", got, pr.reference(3, j0, _slots(j0, C, mask), res_c, f32)
        # ---- multi-edit batches: the chunk form and the one-keyframe chunk alone
        for E in (1, 3):
            nb = 1 + 2 * E
            for j0, C, od in ((0, 3, f32), (1, 1, promoted)):
                plan = ops.propagate_edits_plan(n, C, S, D, True, E)
                assert plan[-1] == f"gather[branches={nb}]" and nx.kernel_of(plan[0]) == fam, plan
                tgt, (kf, _), (res, res_c) = pr.args(nb, j0, C, rk)
                got = ops.propagate_chunks_edits(tgt, pr.piv, inv, kf, w, n, C, j0, True, res, od, E, **kw)
                yield f"propagate_chunks_edits E={E} C={C} res={rk}", got, pr.reference(nb, j0, _slots(j0, C, 1), res_c, od)


SMALL = [(S, D, fam) for S, D, fam in PROP_CASES if S < 1000]
LARGE = [(S, D, fam) for S, D, fam in PROP_CASES if S >= 1000]


@pytest.mark.parametrize("S,D,kernel", SMALL, ids=[f"{c[2]}-S{c[0]}-D{c[1]}" for c in SMALL])
@pytest.mark.parametrize("family", ["pool", "dense"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_propagation_family_vs_oracle(S, D, kernel, family, dtype):
    ops = _ops()
    n = 3 if S == 96 else 2
    assert nx.kernel_of(ops.nn_plan(n * S, S, D, 2, 3)[0]) == nx.kernel_of(kernel)
    pr = Prop(S, D, n, family, dtype)
    inv = ops.pivot_inv_norm(pr.piv)
    count = 0
    for what, got, ref in _calls(ops, pr, inv):
        _same_bits(got, ref, f"S{S} D{D} {family} {dtype} {what}")
        count += 1
    assert count == 3 * 3 + (2 + 4 + 2) + 2 * (3 + 4)      # propagate, propagate_chunks, segments + edits (residual None / model)


@pytest.mark.parametrize("S,D,kernel", LARGE, ids=[f"{c[2]}-S{c[0]}-D{c[1]}" for c in LARGE])
@pytest.mark.parametrize("dtype", DTYPES)
def test_propagation_large_search_forms_vs_oracle(S, D, kernel, dtype):
    """The smallest S of the search families that need a large one (tests/test_segments_gpu.PROP_CASES): a three-chunk call with
    one-keyframe chunks first and in the middle; the exact indices come from the fp64 reference on the device."""
    ops = _ops()
    n, mask, j0, C = 2, 0b101, 0, 3
    plan = ops.propagate_segments_plan(n, C, S, D, mask)
    assert nx.kernel_of(plan[0]) == nx.kernel_of(kernel) and plan[-1] == "gather[branches=3]", plan
    pr = Prop(S, D, n, "pool" if dtype == torch.bfloat16 else "dense", dtype, device_ref=True)
    inv = ops.pivot_inv_norm(pr.piv)
    tgt, (kf, _), (res, res_c) = pr.args(3, j0, C, dtype)
    got = ops.propagate_chunks_segments(tgt, pr.piv, inv, kf, pr.w.cuda(), n, C, j0, mask, res, torch.float32)
    _same_bits(got, pr.reference(3, j0, _slots(j0, C, mask), res_c, torch.float32), f"S{S} D{D} {dtype} mask {mask:#b}")


# --------------------------------------------------------------------------------------------------------- fused norm
# 384 | 392 and 768 | 776: 3 -> 4 pieces per lane; 512 | 520: 16 -> 32 lanes per row; 1024 | 1032: 32 -> 64; 1536: every lane full
NORM_D = [72, 320, 384, 392, 512, 520, 640, 768, 776, 1024, 1032, 1096, 1280, 1536]


def _check_norm(got, ref, gamma, beta, dtype, what):
    ops = _ops()
    out, nout = got
    _same_bits(out, ref, what)
    _same_bits(nout, ops.layer_norm(out, gamma, beta, 1e-5, dtype)[0].cpu(), what + " (norm vs ops.layer_norm)")
    lref = torch.nn.functional.layer_norm(out.float().cpu(), (out.shape[-1],), None if gamma is None else gamma.float().cpu(),
                                          None if beta is None else beta.float().cpu(), 1e-5)
    err = (nout.float().cpu() - lref).abs()
    bound = layer_norm_bound(lref, dtype)
    assert bool((err <= bound).all()), f"{what}: norm exceeds the layer-norm bound by {float((err - bound).max()):.3e}"


@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_norm_vs_oracle(D, affine, dtype):
    ops = _ops()
    S, n = 45, 2
    pr = Prop(S, D, n, "pool" if NORM_D.index(D) % 2 == 0 else "dense", dtype, huge=False)
    inv = ops.pivot_inv_norm(pr.piv)
    g = torch.Generator().manual_seed(D)
    gamma = (1 + 0.2 * torch.randn(D, generator=g)).to(dtype).cuda() if affine else None
    beta = (0.1 * torch.randn(D, generator=g)).to(dtype).cuda() if affine else None
    count = 0
    for what, got, ref in _calls(ops, pr, inv, norm=(gamma, beta, 1e-5, dtype)):
        _check_norm(got, ref, gamma, beta, dtype, f"D{D} affine={affine} {dtype} {what}")
        count += 1
    assert count == 2 + 2 + 3 + 4


# -------------------------------------------------------------------------------------------------------- grid stride
GRID_CAP = 256 * 16                   # gather_blend.hip: `if (blocks > 256 * 16) blocks = 256 * 16` in launch_gb and launch_gbn
STRIDE_CASES = [(1280, 256, 5, 8), (320, 1024, 3, 8)]


@pytest.mark.parametrize("D,S,n,C", STRIDE_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_grid_stride_vs_oracle(D, S, n, C, dtype):
    """Past the grid cap a workgroup takes a second trip through the loop.  gather_blend_kernel: one thread per 8-element piece
    of one token, 256 threads, so one pass covers 4096 * 256 = 1 048 576 pieces (of n C S D/8).  gather_blend_norm_kernel: a
    workgroup of 4 waves owns 4 * (64 / LPR) rows, LPR = 16 lanes per row up to D = 512, 32 up to 1024, 64 above (ln_row.h): one
    pass covers 4096 * 4 * 64 / LPR rows (of 3 n C S)."""
    ops = _ops()
    lpr = 16 if D <= 512 else 32 if D <= 1024 else 64
    pieces, rows = n * C * S * (D // 8), 3 * n * C * S
    assert rows > GRID_CAP * 4 * (64 // lpr), "the fused-norm launch does not stride"
    if D == 1280:
        assert (pieces, rows) == (1638400, 30720) and pieces > GRID_CAP * 256, "the plain launch does not stride"
    else:
        assert rows == 73728
    assert ops.propagate_segments_plan(n, C, S, D, 1)[-1] == "gather[branches=3]"
    inp = nx.Inputs(C, S, D, n * S, [[j, j - 1] if j else [0] for j in range(C)], "pool", seed=D + S)
    tgt8, piv8 = [inp.targets(j, "cuda") for j in range(C)], inp.piv.cuda()
    slots = _slots(0, C, 1)
    want = [[nx.first_argmax(tgt8[j], piv8[s]).cpu() for s in ss] for j, ss in enumerate(slots)]
    g = torch.Generator().manual_seed(D)
    kf = torch.randn(3 * C, S, D, generator=g).to(dtype)
    res = torch.randn(3 * C * n, S, D, generator=g).to(dtype)
    kf[C + 1] = nx.edge_frame(S, D, dtype, 0, huge=False)
    w = orc.blend_weights(n, 1)
    ref = nx.propagation_reference(kf, slots, want, w, res, torch.float32, 3, n)
    piv = inp.pivots("cuda", dtype, scaled=True)
    inv = ops.pivot_inv_norm(piv)
    tgt = torch.cat(tgt8).to(dtype)
    got = ops.propagate_chunks(tgt, piv, inv, kf.cuda(), w.cuda(), n, C, 0, True, res.cuda(), torch.float32)
    _same_bits(got, ref, f"D{D} S{S} {dtype} plain")
    gamma, beta = ((1 + 0.2 * torch.randn(D, generator=g)).to(dtype).cuda(), (0.1 * torch.randn(D, generator=g)).to(dtype).cuda())
    got = ops.propagate_chunks(tgt, piv, inv, kf.cuda(), w.cuda(), n, C, 0, True, res.cuda(), torch.float32,
                               norm=(gamma, beta, 1e-5, dtype))
    _check_norm(got, ref, gamma, beta, dtype, f"D{D} S{S} {dtype} fused norm")
