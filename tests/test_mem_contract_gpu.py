"""The memory contract of every entry point, on the GPU (tests/mem_contract.py; tests/test_mem_contract_cpu.py shows on mutants
that these assertions fail on a kernel that breaks it).

Every call runs with its tensors in a POISON-filled arena (NaN neighbours for the float tensors, -1 for the indices; q, k, v as
column slabs with NaN gap columns on both sides of every row), on scratch of EXACTLY the size the library reports (guarded on
both sides, the rear guard as large as the payload), filled with 0xFF (NaN), 0x00 and 0x7F (huge).  Asserted per call:

  * the wrapper ran on the arena's tensors, not on copies (Spy);
  * no byte outside the output changed -- inputs, gap columns, the 4 KiB between tensors, the guards;
  * the scratch guards are intact: the reported size covers every write;
  * the input slabs the call has no use for (v of branches it does not compute, q and k of branches that take the source's, a
    keyframe the search is not aimed at) hold NaN;
  * the rows the call does not own keep their sentinel, the result is finite and right -- the census tolerance of
    tests/attn_exact.py, the exact first-index reference of tests/nn_exact.py, the bit-exact propagation reference, the
    references and tolerances of the tests that already cover the small kernels;
  * the result is bit-identical under the three scratch fills: nothing is read from scratch the call did not write.

Attention: every case of attn_exact.GPU_CASES in each of its modes, bf16 and f16 (census flat negative; 16-bit output under the
three fills, fp32 output under 0xFF).  The run wrapper copies what is not contiguous, so its cases are placed dense and run
once more on column slabs through the `_views` form.
NN search: every case of nn_exact.NN_CASES on the dense family.  Propagation: every call of test_nn_exact_gpu._calls on the
SMALL cases, plain and with the fused norm.  Then the small kernels.
"""
import math

import pytest
import torch

from oracle import golden_cases as gc
from oracle import tokenflow_oracle as orc
from tests import attn_exact as ax
from tests import attn_run_forms as rf
from tests import kernel_forms as kf
from tests import mem_contract as mc
from tests import nn_exact as nx
from tests.test_kernels_gpu import layer_norm_bound
from tests.test_nn_exact_gpu import SMALL, Prop, _calls, _check_norm, _same_bits

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
F32 = torch.float32
IDX_SENTINEL = -7


def _ops():
    from tokenflow_amd import ops
    return ops


def _nbytes(t):
    return t.numel() * t.element_size()


def _es(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _log(family, requests):
    for tag, nbytes in requests:
        print(f"SCRATCH {family} {tag} {nbytes}")


def _arena(inputs, outputs):
    """An arena holding the `inputs` {name: tensor} (dense) and the `outputs` {name: (shape, dtype, fill)}; the views."""
    sizes = [_nbytes(t) for t in inputs.values()] + [math.prod(s) * _es(d) for s, d, _ in outputs.values()]
    arena = mc.Arena("cuda", mc.Arena.footprint(*sizes))
    t = {name: arena.place(name, x) for name, x in inputs.items()}
    t.update({name: arena.place_out(name, s, d, f) for name, (s, d, f) in outputs.items()})
    return arena, t


def _checked(monkeypatch, arena, writable, call, fill=mc.POISON):
    """One call under Scratch(fill) + Spy, held to `mc.verify`; returns (the call's result, the scratch requests)."""
    ops = _ops()
    snap = arena.snapshot()
    with monkeypatch.context() as mp:
        scratch, spy = mc.Scratch(mp, ops, fill), mc.Spy(mp, ops)
        got = call()
        mc.verify(arena, snap, writable, scratch, spy)
    return got, scratch.requests


# ---------------------------------------------------------------------------------------------------------- attention
def _attn_ws_bytes(ops, name, spec, dtype):
    """The size function of the case's entry point (every request must be exactly this)."""
    from tokenflow_amd import _lib
    lib, dt = _lib.load(), ops._DT[dtype]
    K, Kq, S, H, d = spec.K, spec.Kq, spec.S, spec.H, spec.d
    if name in ax.RUN_CASES:
        return lib.tf_ext_attn_runs_workspace_bytes(K, Kq, S, H, d, 3, dt)
    if name in ax.SEGMENT_CASES:
        return lib.tf_ext_attn_segments_workspace_bytes(K, S, H, d, dt)
    if name in ax.EDIT_CASES:
        return lib.tf_ext_attn_edits_workspace_bytes(K, S, H, d, (spec.nbr - 1) // 2, dt)
    return lib.tf_ext_attn_workspace_bytes(K, S, H, d, dt)


def _attn_contract(monkeypatch, case, dtype, dense=False, call=None):
    """dense: q, k, v placed dense instead of as column slabs; call: made instead of case.call (same arguments)."""
    ops, spec = _ops(), case.spec
    call = case.call if call is None else call
    v, ones = ax.census_v(spec)
    c, n = ax.census_expected(spec, v)
    q, k = ax.census_qk(spec, "flat", case.seed)
    ld, col0 = (None, 0) if dense else (spec.D + 16, 8)
    row = (spec.D if dense else ld) * 2
    arena = mc.Arena("cuda", mc.Arena.footprint(q.shape[0] * spec.S * row, k.shape[0] * spec.S * row, k.shape[0] * spec.S * row,
                                                q.numel() * 2, q.numel() * 4))
    dq, dk, dv = (arena.place(name, t.to(dtype), ld, col0) for name, t in (("q", q), ("k", k), ("v", v)))
    # the slabs the call has no use for -- v of the branches it does not compute, q and k of those whose scores come from the
    # source's -- are "never touched" (tokenflow_hip.h): they hold NaN
    need_qk, need_v = {spec.qk_branch(b) for b in spec.owned}, set(spec.owned)
    for b in range(spec.nbr):
        if b not in need_qk:
            dq[b * spec.Kq:(b + 1) * spec.Kq] = math.nan
            dk[b * spec.K:(b + 1) * spec.K] = math.nan
        if b not in need_v:
            dv[b * spec.K:(b + 1) * spec.K] = math.nan
    outs = [("out16", arena.place_out("out16", q.shape, dtype, ax.SENTINEL), dtype, mc.FILLS),
            ("out32", arena.place_out("out32", q.shape, F32, ax.SENTINEL), F32, (mc.POISON,))]
    want_bytes = _attn_ws_bytes(ops, case.name, spec, dtype)
    for mode in case.modes:
        for out_name, out, out_dtype, fills in outs:
            case.check_plan(case.plan(ops, dtype, out_dtype, **mode), dtype, **mode)
            reqs = mc.check_census_call(monkeypatch, ops, lambda o: call(ops, dq, dk, dv, o, **mode), arena, out, out_name,
                                        spec, (c, n, ones, out_dtype), fills, what=f"{case.name} {mode} {dtype} -> {out_dtype}")
            assert len(reqs) == len(fills) and all(nb == want_bytes for _, nb in reqs), (reqs, want_bytes)
            _log("attn-" + case.name.split("-")[0], reqs)


ATTN_GROUPS = {"forms": ax.FORM_CASES, "sets": ax.SET_CASES, "edits": ax.EDIT_CASES, "runs": ax.RUN_CASES, "segments": ax.SEGMENT_CASES}


def test_every_attention_case_is_covered():
    assert sum(len(g) for g in ATTN_GROUPS.values()) == len(ax.GPU_CASES)
    assert {name for g in ATTN_GROUPS.values() for name in g} == set(ax.GPU_CASES)


@pytest.mark.parametrize("name", list(ax.FORM_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_kernel_forms(monkeypatch, name, dtype):
    _attn_contract(monkeypatch, ax.FORM_CASES[name], dtype)


@pytest.mark.parametrize("name", list(ax.SET_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_frame_sets_and_windows(monkeypatch, name, dtype):
    _attn_contract(monkeypatch, ax.SET_CASES[name], dtype)


@pytest.mark.parametrize("name", list(ax.EDIT_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_edits(monkeypatch, name, dtype):
    _attn_contract(monkeypatch, ax.EDIT_CASES[name], dtype)


@pytest.mark.parametrize("name", list(ax.RUN_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_runs(monkeypatch, name, dtype):
    """`ext_attn_runs` makes q, k, v contiguous -- a column slab would be copied and the Spy would say so -- so the wrapper runs
    on dense tensors; the run kernels see the column slabs through `ext_attn_runs_views`, called as the wrapper calls it."""
    case = ax.RUN_CASES[name]
    spec, g = case.spec, rf.BASE
    kw = [kw for S, H, d, kw in ax.RUN_SHAPES if (S, H, d) == (spec.S, spec.H, spec.d)][0]
    _attn_contract(monkeypatch, case, dtype, dense=True)

    def views(ops, q, k, v, out):
        K, Kq, S, D = spec.K, spec.Kq, spec.S, spec.D
        k4, v4 = k.unflatten(0, (3, K)), v.unflatten(0, (3, K))
        kv_runs = [(k4[:, f0:f0 + n], v4[:, f0:f0 + n], 0, 0) for f0, n in g["runs"]]
        ops.ext_attn_runs_views(q.unflatten(0, (3, Kq)), kv_runs, out.view(3, Kq, S, D), spec.H, spec.scale, spec.inject[1], g["runs"], K,
                                q_frame0=g["q_frame0"], **kw)
    _attn_contract(monkeypatch, case, dtype, call=views)


@pytest.mark.parametrize("name", list(ax.SEGMENT_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_segments(monkeypatch, name, dtype):
    _attn_contract(monkeypatch, ax.SEGMENT_CASES[name], dtype)


# ----------------------------------------------------------------------------------------------------------- NN search
def _across_fills(what, ref, fill, got):
    """Keep the first fill's result (a clone), compare the later ones with it bit for bit."""
    if ref is None:
        return fill, tuple(t.clone() for t in got)
    for a, b in zip(ref[1], got):
        mc.assert_same_across_fills(what, {ref[0]: a, fill: b})
    return ref


@pytest.mark.parametrize("form,i", nx.NN_CASES, ids=[f"{f}-{i}" for f, i in nx.NN_CASES])
def test_contract_nn_search(monkeypatch, form, i):
    ops = _ops()
    c = kf.CASES[form][i]
    assert form in [kf.form(t) for t in kf.plan(ops, c)]
    n_tgt, S, D, C, P = c["n_tgt"], c["S"], c["D"], c["C"], c["P"]
    inp = nx.Inputs.of_case(c, "dense")
    chunks, K, n = inp.chunks, inp.K, n_tgt // S
    piv8 = inp.piv.cuda()
    tgt8 = torch.cat([inp.targets(j, "cuda") for j in range(C)])
    want = [[nx.first_argmax(tgt8[j * n_tgt:(j + 1) * n_tgt], piv8[s], block=8192) for s in chunks[j]] for j in range(C)]
    from tokenflow_amd import _lib
    lib = _lib.load()
    for dtype in DTYPES:
        inputs = {"tgt": tgt8.to(dtype), "piv": inp.pivots("cuda", dtype, False)}
        outputs = {"inv_norm": ((K, S), F32, ax.SENTINEL)}
        if C == 1:
            outputs["idx"] = ((P, n_tgt), torch.int32, IDX_SENTINEL)
            want_bytes = lib.tf_nn_search_workspace_bytes(n_tgt, S, D, P)
        else:      # as test_search_exact decodes both indices of a target from ONE propagate_chunks call on an index-coded cache
            code = torch.zeros(3, K, S, D, dtype=F32, device="cuda")
            rows = torch.arange(S, dtype=F32, device="cuda")
            code[:, 0::2, :, 0] = rows
            code[:, 1::2, :, 1] = rows
            inputs.update(kf_out=code.view(3 * K, S, D), w=torch.full((n,), 0.5, device="cuda"))
            outputs["out"] = ((3 * C * n, S, D), F32, ax.SENTINEL)
            want_bytes = lib.tf_nn_gather_blend_chunks_workspace_bytes(n * S, S, D, C)
        arena, t = _arena(inputs, outputs)
        del inputs
        what = f"{form}-{i} dense {dtype}"
        _checked(monkeypatch, arena, ["inv_norm"], lambda: ops.pivot_inv_norm(t["piv"], out=t["inv_norm"]))
        assert bool((t["inv_norm"] == t["inv_norm"].flatten()[0]).all()), "precondition: one fp32 inv_norm for rows of one norm"
        for s in set(range(K)) - {s for ss in chunks for s in ss}:      # a keyframe the call does not search holds NaN
            t["piv"][s] = math.nan
            t["inv_norm"][s] = math.nan
        ref = None
        for fill in mc.FILLS:
            if C == 1:
                t["idx"].fill_(IDX_SENTINEL)
                got, reqs = _checked(monkeypatch, arena, ["idx"],
                                     lambda: ops.nn_search(t["tgt"], t["piv"], t["inv_norm"], chunks[0], idx=t["idx"]), fill)
                assert got is t["idx"]
                for p, s in enumerate(chunks[0]):
                    assert torch.equal(got[p].long(), want[0][p]), f"{what} fill {fill:#04x} keyframe {s}"
            else:
                t["out"].fill_(ax.SENTINEL)
                got, reqs = _checked(monkeypatch, arena, ["out"],
                                     lambda: ops.propagate_chunks(t["tgt"], t["piv"], t["inv_norm"], t["kf_out"], t["w"], n, C, 0, True,
                                                                  None, F32, out=t["out"]), fill)
                assert got is t["out"]
                o = got.view(3, C, n * S, D)
                assert torch.equal(o[0], o[1]) and torch.equal(o[0], o[2])
                idx = [[o[0, 0, :, 0].long()]] + [[(2 * o[0, j, :, j & 1]).long(), (2 * o[0, j, :, (j - 1) & 1]).long()] for j in range(1, C)]
                for j in range(C):
                    for p, s in enumerate(chunks[j]):
                        assert torch.equal(idx[j][p], want[j][p]), f"{what} fill {fill:#04x} chunk {j} keyframe {s}"
            assert reqs == [("nn", want_bytes)], (reqs, want_bytes)
            _log("nn_search" if C == 1 else "propagate_chunks(search cases)", reqs)
            ref = _across_fills(what, ref, fill, (got,))
        del arena, t, ref


# --------------------------------------------------------------------------------------------------------- propagation
class ArenaOps:
    """`ops` as tests.test_nn_exact_gpu._calls sees it: every propagate* call is made with ALL its tensors -- targets, pivots,
    inv_norm, kf_out, residual, weights, norm weights, the result and the norm output -- placed in a fresh arena, once per scratch
    fill under Scratch + Spy, held to `mc.verify` and to bit-equality across the fills; what it returns is the result in the
    arena (a clone).  Everything else is the module's."""

    def __init__(self, ops, monkeypatch):
        self._ops, self._mp, self.requests = ops, monkeypatch, []

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def _run(self, what, tensors, shape, out_dtype, norm, call):
        inputs = {k_: v_ for k_, v_ in tensors.items() if v_ is not None}
        outputs = {"out": (shape, out_dtype, ax.SENTINEL)}
        if norm is not None:
            gamma, beta, eps, ndt = norm
            inputs.update({k_: v_ for k_, v_ in (("gamma", gamma), ("beta", beta)) if v_ is not None})
            outputs["norm_out"] = (shape, ndt, ax.SENTINEL)
        arena, t = _arena(inputs, outputs)
        kw = {"out": t["out"]}
        if norm is not None:
            kw.update(norm=(t.get("gamma"), t.get("beta"), eps, ndt), norm_out=t["norm_out"])
        ref = None
        for fill in mc.FILLS:
            for name in outputs:
                t[name].fill_(ax.SENTINEL)
            got, reqs = _checked(self._mp, arena, list(outputs), lambda: call({k_: t.get(k_) for k_ in tensors}, kw), fill)
            got = got if norm is not None else (got,)
            assert got[0] is t["out"] and (norm is None or got[1] is t["norm_out"]), f"{what}: the caller's buffers were not used"
            assert len(reqs) == 1 and reqs[0][0] == "nn", reqs
            self.requests += reqs
            ref = _across_fills(what, ref, fill, got)
        return ref[1] if norm is not None else ref[1][0]

    def propagate(self, tgt, piv, inv, ids, kf_out, w, n, residual, out_dtype, norm=None):
        S, D = piv.shape[1:]
        return self._run("propagate", dict(tgt=tgt, piv=piv, inv_norm=inv, kf_out=kf_out, w=w, residual=residual), (3 * n, S, D),
                         out_dtype, norm, lambda t, kw: self._ops.propagate(t["tgt"], t["piv"], t["inv_norm"], ids, t["kf_out"], t["w"],
                                                                            n, t["residual"], out_dtype, **kw))

    def propagate_chunks(self, tgt, piv, inv, kf_out, w, n, C, slot0, first, residual, out_dtype, norm=None):
        S, D = piv.shape[1:]
        return self._run("propagate_chunks", dict(tgt=tgt, piv=piv, inv_norm=inv, kf_out=kf_out, w=w, residual=residual),
                         (3 * C * n, S, D), out_dtype, norm,
                         lambda t, kw: self._ops.propagate_chunks(t["tgt"], t["piv"], t["inv_norm"], t["kf_out"], t["w"], n, C, slot0,
                                                                  first, t["residual"], out_dtype, **kw))

    def propagate_chunks_segments(self, tgt, piv, inv, kf_out, w, n, C, slot0, mask, residual, out_dtype, norm=None):
        S, D = piv.shape[1:]
        return self._run("propagate_chunks_segments", dict(tgt=tgt, piv=piv, inv_norm=inv, kf_out=kf_out, w=w, residual=residual),
                         (3 * C * n, S, D), out_dtype, norm,
                         lambda t, kw: self._ops.propagate_chunks_segments(t["tgt"], t["piv"], t["inv_norm"], t["kf_out"], t["w"], n, C,
                                                                           slot0, mask, t["residual"], out_dtype, **kw))

    def propagate_chunks_edits(self, tgt, piv, inv, kf_out, w, n, C, slot0, first, residual, out_dtype, E, norm=None):
        S, D = piv.shape[1:]
        return self._run("propagate_chunks_edits", dict(tgt=tgt, piv=piv, inv_norm=inv, kf_out=kf_out, w=w, residual=residual),
                         ((1 + 2 * E) * C * n, S, D), out_dtype, norm,
                         lambda t, kw: self._ops.propagate_chunks_edits(t["tgt"], t["piv"], t["inv_norm"], t["kf_out"], t["w"], n, C,
                                                                        slot0, first, t["residual"], out_dtype, E, **kw))


@pytest.mark.parametrize("S,D,kernel", SMALL, ids=[f"{c[2]}-S{c[0]}-D{c[1]}" for c in SMALL])
@pytest.mark.parametrize("fused_norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_propagation(monkeypatch, S, D, kernel, fused_norm, dtype):
    ops = _ops()
    n = 3 if S == 96 else 2
    assert nx.kernel_of(ops.nn_plan(n * S, S, D, 2, 3)[0]) == nx.kernel_of(kernel)
    pr = Prop(S, D, n, "pool" if dtype == torch.bfloat16 else "dense", dtype, huge=not fused_norm)
    inv = ops.pivot_inv_norm(pr.piv)
    g = torch.Generator().manual_seed(D)
    gamma = (1 + 0.2 * torch.randn(D, generator=g)).to(dtype).cuda()
    beta = (0.1 * torch.randn(D, generator=g)).to(dtype).cuda()
    aops = ArenaOps(ops, monkeypatch)
    count = 0
    for what, got, ref in _calls(aops, pr, inv, norm=(gamma, beta, 1e-5, dtype) if fused_norm else None):
        what = f"S{S} D{D} {dtype} {what}"
        if fused_norm:
            _check_norm(got, ref, gamma, beta, dtype, what)
        else:
            _same_bits(got, ref, what)
        count += 1
    assert count == (2 + 2 + 3 + 4 if fused_norm else 3 * 3 + (2 + 4 + 2) + 2 * (3 + 4))      # as the tests of test_nn_exact_gpu count them
    assert len(aops.requests) == 3 * count
    _log("propagate", aops.requests)


# ---------------------------------------------------------------------------------------------------- the small kernels
@pytest.mark.parametrize("rows,D", [(5, 72), (37, 1280), (3, 2048), (515, 640)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_layer_norm(monkeypatch, rows, D, dtype):
    """As test_layer_norm_vs_torch_fp32: torch's fp32 layer_norm of the same input within `layer_norm_bound`, the inverse norms
    those of the rounded output rows; the fp32 inv_norm has -- like every tensor here -- NaN behind row rows - 1."""
    ops = _ops()
    g = torch.Generator().manual_seed(rows * 7 + D)
    x = (torch.randn(rows, D, generator=g) * 3 + 0.5).to(dtype)
    w, b = (1 + 0.2 * torch.randn(D, generator=g)).to(dtype), (0.1 * torch.randn(D, generator=g)).to(dtype)
    ref = torch.nn.functional.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-5)
    arena, t = _arena({"x": x, "w": w, "b": b}, {"out": ((rows, D), dtype, ax.SENTINEL), "inv": ((rows,), F32, ax.SENTINEL)})
    (out, inv), reqs = _checked(monkeypatch, arena, ["out", "inv"], lambda: ops.layer_norm(t["x"], t["w"], t["b"], 1e-5, dtype,
                                                                                          want_inv_norm=True, out=t["out"], inv_out=t["inv"]))
    assert out is t["out"] and inv is t["inv"] and reqs == []
    got = out.float().cpu()
    assert bool(((got - ref).abs() <= layer_norm_bound(ref, dtype)).all())
    assert torch.allclose(inv.cpu(), 1.0 / got.norm(dim=-1), rtol=2e-6, atol=0)
    # and without the side output: nothing but `out` is written
    t["out"].fill_(ax.SENTINEL)
    _checked(monkeypatch, arena, ["out"], lambda: ops.layer_norm(t["x"], t["w"], t["b"], 1e-5, dtype, out=t["out"]))
    assert torch.equal(t["out"].float().cpu(), got)


@pytest.mark.parametrize("rows,D", [(5, 72), (37, 1280)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_add_layer_norm(monkeypatch, rows, D, dtype):
    """As test_add_layer_norm_equals_add_then_norm: torch's a + b and tf_layer_norm of it, bit for bit."""
    ops = _ops()
    g = torch.Generator().manual_seed(rows + D)
    a, b = (torch.randn(rows, D, generator=g) * 2).to(dtype), (torch.randn(rows, D, generator=g) + 0.3).to(dtype)
    w, bias = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    arena, t = _arena({"a": a, "b": b, "w": w, "bias": bias},
                      {"total": ((rows, D), dtype, ax.SENTINEL), "out": ((rows, D), dtype, ax.SENTINEL)})
    (total, out), _ = _checked(monkeypatch, arena, ["total", "out"],
                               lambda: ops.add_layer_norm(t["a"], t["b"], t["w"], t["bias"], 1e-5, dtype, total=t["total"], out=t["out"]))
    assert total is t["total"] and out is t["out"]
    want = a.cuda() + b.cuda()
    assert torch.equal(total, want) and torch.equal(out, ops.layer_norm(want, w.cuda(), bias.cuda(), 1e-5, dtype)[0])


@pytest.mark.parametrize("K,S,D", [(2, 45, 72), (1, 515, 640), (3, 7, 1280)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_pivot_inv_norm(monkeypatch, K, S, D, dtype):
    ops = _ops()
    g = torch.Generator().manual_seed(K + S + D)
    piv = torch.randn(K, S, D, generator=g).to(dtype)
    arena, t = _arena({"piv": piv}, {"inv": ((K, S), F32, ax.SENTINEL)})
    inv, _ = _checked(monkeypatch, arena, ["inv"], lambda: ops.pivot_inv_norm(t["piv"], out=t["inv"]))
    assert inv is t["inv"] and torch.equal(inv, ops.pivot_inv_norm(piv.cuda()))
    assert torch.allclose(inv.cpu(), 1.0 / piv.float().norm(dim=-1), rtol=2e-6, atol=0)


@pytest.mark.parametrize("name", list(gc.PROP_CASES))
def test_contract_gather_blend(monkeypatch, name):
    """As test_gather_blend_bit_exact_vs_golden: the oracle's gather_blend on the oracle's indices, bit for bit."""
    ops = _ops()
    K, n, S, D, dt = gc.PROP_CASES[name]
    piv, kf_out, hidden = gc.prop_inputs(name)
    w = orc.blend_weights(n, 1)
    for bi in range(K):
        ids = orc.keyframe_ids(bi)
        idx, _ = orc.nn_search(hidden[bi].float().view(3, n, S, D)[0], piv[0], bi)
        ref = orc.gather_blend(kf_out, idx, bi, n, residual=hidden[bi])
        arena, t = _arena({"kf_out": kf_out, "idx": torch.stack(idx).int(), "w": w, "residual": hidden[bi]},
                          {"out": ((3 * n, S, D), ref.dtype, ax.SENTINEL)})
        out, _ = _checked(monkeypatch, arena, ["out"], lambda: ops.gather_blend(t["kf_out"], t["idx"], t["w"] if len(ids) == 2 else None,
                                                                                ids, n, t["residual"], ref.dtype, out=t["out"]))
        assert out is t["out"] and torch.equal(out.cpu(), ref), f"{name}/chunk{bi}"


DDIM_N = [1, 255, 257, 256 * 8 * 256 + 3]      # the last: one past the grid cap, the stride loop runs


@pytest.mark.parametrize("n", DDIM_N)
@pytest.mark.parametrize("dtype", DTYPES + [F32])
def test_contract_ddim_step(monkeypatch, n, dtype):
    """As test_ddim_step_bit_exact: the oracle's restatement, bit for bit, out of place and with out = x."""
    ops = _ops()
    g = torch.Generator().manual_seed(7 + n)
    x, eps = (torch.randn(n, generator=g).to(dtype) for _ in range(2))
    co = (0.9734, 0.2291, 0.9581, 0.2864)
    ref = orc.ddim_step(x, eps, *co)
    arena, t = _arena({"x": x, "eps": eps}, {"out": ((n,), dtype, ax.SENTINEL)})
    out, _ = _checked(monkeypatch, arena, ["out"], lambda: ops.ddim_step(t["x"], t["eps"], *co, out=t["out"]))
    assert out is t["out"] and torch.equal(out.cpu(), ref)
    _checked(monkeypatch, arena, ["x"], lambda: ops.ddim_step(t["x"], t["eps"], *co, out=t["x"]))
    assert torch.equal(t["x"].cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES + [F32])
def test_contract_inject_copy(monkeypatch, dtype):
    """As test_inject_copy_exact / test_inject_copy_edits_masked_exact, on branches of 2 * 5 * 7 * 4 = 280 elements: whole 16-byte
    pieces (the kernels' precondition) but no multiple of 256 elements, so the last workgroup is ragged."""
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(6, 5, 7, 4, generator=g).to(dtype)
    arena, t = _arena({"x": x}, {})
    _checked(monkeypatch, arena, ["x"], lambda: ops.inject_copy_(t["x"]))
    assert torch.equal(t["x"].cpu(), orc.conv_inject_(x.clone()))
    E, n = 3, 2
    for mask in (None, 0b101, 0b010):
        x = torch.randn((1 + 2 * E) * n, 5, 7, 4, generator=g).to(dtype)
        want = x.clone()
        for e in range(E):
            if mask is None or (mask >> e) & 1:
                want[(1 + 2 * e) * n:(3 + 2 * e) * n] = x[:n].repeat(2, 1, 1, 1)
        arena, t = _arena({"x": x}, {})
        _checked(monkeypatch, arena, ["x"], lambda: ops.inject_copy_edits_(t["x"], E, edit_mask=mask))
        assert torch.equal(t["x"].cpu().view(torch.uint8), want.view(torch.uint8)), mask


@pytest.mark.parametrize("W,Kl,S,D,dtype", [(2, 3, 200, 160, torch.float16), (4, 2, 64, 1280, torch.bfloat16), (2, 2, 45, 80, F32)])
def test_contract_head_pack_unpack(monkeypatch, W, Kl, S, D, dtype):
    """As test_head_pack_unpack: the torch formulation of the re-layout, bit for bit, from column slabs of a fused projection
    output (q | k | v side by side: the slabs' neighbouring columns are the other projections; the arena guards the tensor)."""
    ops = _ops()
    g = torch.Generator().manual_seed(W + S)
    hd = D // W
    fused = torch.randn(3 * Kl, S, 3 * D, generator=g).to(dtype)
    recv2 = torch.randn(W, Kl, 2, S, hd, generator=g).to(dtype)
    arena, t = _arena({"fused": fused, "recv": recv2},
                      {"send": ((W, Kl, 6, S, hd), dtype, ax.SENTINEL), "dst": ((3, Kl, S, D), dtype, 0.0)})
    q3, k3, v3 = (t["fused"][..., i * D:(i + 1) * D].unflatten(0, (3, Kl)) for i in range(3))
    slabs = [q3[1], q3[2], k3[1], k3[2], v3[1], v3[2]]
    send, _ = _checked(monkeypatch, arena, ["send"], lambda: ops.head_pack(slabs, W, out=t["send"]))
    want = torch.stack([s.reshape(Kl, S, W, hd) for s in slabs], dim=1).permute(3, 0, 1, 2, 4)
    assert send is t["send"] and torch.equal(send, want)
    _checked(monkeypatch, arena, ["dst"], lambda: ops.head_unpack(t["recv"], [t["dst"][1], t["dst"][2]]))
    assert torch.equal(t["dst"][1:3].view(2, Kl, S, W, hd), t["recv"].permute(2, 1, 3, 0, 4)) and bool((t["dst"][0] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_window_halo_pack(monkeypatch, dtype):
    """As test_halo_pack (strided): torch indexing, bit for bit; a frame in two segments, an empty side."""
    ops = _ops()
    Kl, S, D = 3, 72, 80
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(3, Kl, S, 3 * D, generator=g).to(dtype)
    for pick in ((1, 2), (0,)):
        for segs in ([(0, 3), (0, 3), (2, 1)], [(0, 0), (0, 3), (1, 2)], [(1, 1), (0, 0), (0, 0)]):
            frames = [f for f0, n in segs for f in range(f0, f0 + n)]
            ns = 2 * len(pick)
            arena, t = _arena({"qkv": qkv}, {"out": ((len(frames), ns, S, D), dtype, ax.SENTINEL)})
            k3, v3 = t["qkv"][..., D:2 * D], t["qkv"][..., 2 * D:]
            slabs = [k3[b] for b in pick] + [v3[b] for b in pick]
            got, _ = _checked(monkeypatch, arena, ["out"], lambda: ops.window_halo_pack(slabs, segs, out=t["out"]))
            assert got is t["out"] and torch.equal(got, torch.stack([torch.stack([s[f] for s in slabs]) for f in frames])), segs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ns", [3, 6])
def test_contract_frame_set_halo_pack(monkeypatch, dtype, ns):
    """As test_frame_set_halo_pack: strided slab views (frame stride != S * ld, ld > D), an empty peer, a full peer, a frame sent
    to three peers, a non-contiguous mask."""
    ops = _ops()
    Kl, S, D = 3, 3, 8
    g = torch.Generator().manual_seed(3 + ns)
    buf = torch.randn(6, Kl + 1, S + 2, 3 * D, generator=g).to(dtype)
    for masks in ([0b000, 0b111, 0b101], [0b010, 0b010, 0b011, 0b110], [0b100], [0b111] * 5):
        frames = [f for m in masks for f in ax.members(m)]
        arena, t = _arena({"buf": buf}, {"out": ((len(frames), ns, S, D), dtype, ax.SENTINEL)})
        slabs = [t["buf"][i, :Kl, 1:1 + S, D * (i % 3):D * (i % 3) + D] for i in range(ns)]
        got, _ = _checked(monkeypatch, arena, ["out"], lambda: ops.frame_set_halo_pack(slabs, masks, out=t["out"]))
        assert got is t["out"] and torch.equal(got, torch.stack([torch.stack([s[f] for s in slabs]) for f in frames])), masks


# ------------------------------------------------------------------------------------------------- caller buffers
def test_caller_buffers_are_validated():
    """idx= / out= / norm_out= / total=: shape, dtype, contiguity and device, ValueError otherwise; without them the calls
    allocate as before."""
    ops = _ops()
    K, n, S, D, dt = 2, 2, 45, 72, torch.bfloat16
    g = torch.Generator().manual_seed(5)
    piv, tgt = torch.randn(K, S, D, generator=g).to(dt).cuda(), torch.randn(n * S, D, generator=g).to(dt).cuda()
    kf_out, res = torch.randn(3 * K, S, D, generator=g).to(dt).cuda(), torch.randn(3 * n, S, D, generator=g).to(dt).cuda()
    inv, w = ops.pivot_inv_norm(piv), orc.blend_weights(n, 1).cuda()
    idx = ops.nn_search(tgt, piv, inv, [1, 0])
    buf = torch.empty_like(idx)
    assert ops.nn_search(tgt, piv, inv, [1, 0], idx=buf) is buf and torch.equal(buf, idx)
    bad_idx = [torch.empty(2, n * S + 1, dtype=torch.int32, device="cuda"), torch.empty(2, n * S, dtype=torch.int64, device="cuda"),
               torch.empty(n * S, 2, dtype=torch.int32, device="cuda").T, torch.empty(2, n * S, dtype=torch.int32)]
    for b in bad_idx[:3]:
        with pytest.raises(ValueError, match="idx"):
            ops.nn_search(tgt, piv, inv, [1, 0], idx=b)
    with pytest.raises(Exception):      # a CPU buffer: refused before anything is launched
        ops.nn_search(tgt, piv, inv, [1, 0], idx=bad_idx[3])
    want = ops.propagate(tgt, piv, inv, [1, 0], kf_out, w, n, res, F32)
    out = torch.empty_like(want)
    assert ops.propagate(tgt, piv, inv, [1, 0], kf_out, w, n, res, F32, out=out) is out and torch.equal(out, want)
    assert torch.equal(ops.gather_blend(kf_out, idx, w, [1, 0], n, res, F32, out=out), want)
    norm = (None, None, 1e-5, dt)
    want2, wantn = ops.propagate(tgt, piv, inv, [1, 0], kf_out, w, n, res, F32, norm=norm)
    nout = torch.empty_like(wantn)
    got2, gotn = ops.propagate(tgt, piv, inv, [1, 0], kf_out, w, n, res, F32, norm=norm, out=out, norm_out=nout)
    assert got2 is out and gotn is nout and torch.equal(out, want2) and torch.equal(nout, wantn)
    for kw in ({"out": out.bfloat16()}, {"out": out[:, :, ::2]}, {"out": out[1:]}, {"norm_out": nout}):
        with pytest.raises(ValueError):
            ops.propagate(tgt, piv, inv, [1, 0], kf_out, w, n, res, F32, **kw)
    with pytest.raises(ValueError, match="norm_out"):
        ops.propagate(tgt, piv, inv, [1, 0], kf_out, w, n, res, F32, norm=norm, norm_out=nout.float())
    with pytest.raises(ValueError, match="out"):
        ops.gather_blend(kf_out, idx, w, [1, 0], n, res, F32, out=out.bfloat16())
    for fn, args in ((ops.propagate_chunks, (2, 1, False)), (ops.propagate_chunks_segments, (2, 0, 0b01))):
        tg2 = torch.cat([tgt, tgt])
        r2 = torch.cat([res.view(3, n, S, D)] * 2, 1).reshape(6 * n, S, D)
        with pytest.raises(ValueError, match="out"):
            fn(tg2, torch.cat([piv, piv]), torch.cat([inv, inv]), torch.cat([kf_out.view(3, K, S, D)] * 2, 1).reshape(6 * K, S, D), w,
               n, *args, r2, F32, out=out)
    with pytest.raises(ValueError, match="out"):
        ops.propagate_chunks_edits(tgt, piv, inv, kf_out, w, n, 1, 1, False, res, F32, 1, out=out[1:])
    a = torch.randn(5, D, generator=g).to(dt).cuda()
    with pytest.raises(ValueError, match="total"):
        ops.add_layer_norm(a, a, None, None, 1e-5, dt, total=torch.empty(5, D, dtype=F32, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        ops.add_layer_norm(a, a, None, None, 1e-5, dt, out=torch.empty(4, D, dtype=dt, device="cuda"))
