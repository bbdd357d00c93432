"""Every entry point under the issue contract (tests/issue_contract.py: P1 late inputs on a busy side stream, P2 the call does
not wait, P3 graph replay, P4 beside itself; tests/test_issue_contract_mutants_gpu.py shows that each protocol bites), and P5:

  P5  scratch for a foreign stream (the wrappers that take `stream=`): a small case and then a larger one are issued with
      stream=raw on a busy stream that is not current, so the cached scratch of that stream is replaced while the launches that
      use the old one are still queued.  A buffer of the old size allocated on the current stream right then must not be the
      old block (a control shows that the allocator does hand a block dropped on the current stream straight back), must still
      hold its fill afterwards, and both results must be the eager ones.

Expected values are the same calls issued eagerly on the default stream; everything is compared bit for bit.  Inputs are seeded
N(0,1) tensors (set A and set B), index tensors are results of the search itself.

Coverage: every case of attn_exact.GPU_CASES in each of its modes, bf16 and f16, under P1 + P2, and the first case of every
distinct launch plan under P3 + P4; the eight `_views` wrappers at a bank-part geometry (Kq < K, q_frame0 > 0, column slabs,
a fused and a streaming form) under P1-P4, the three with `stream=` also with stream= the capturing stream and under P5, the run
wrappers with `streams=` under P1; every NN search case and every call form of test_nn_exact_gpu._calls on the SMALL shapes; the
small kernels; the rank executors on a loopback world under P1 + P2.

Found on an MI355X ("The issue contract"): every kernel, wrapper and executor passes P1, P2 and P4 and every
single-stream call P3.  `ops._workspace` failed P3 with stream= the capturing stream (the graph's buffer was cached for later eager
calls) and P5 on all three wrappers (the allocator handed the outgrown block of the busy foreign stream to the next request on
the current stream, and a queued vt_pack wrote into it); both are fixed there.
"""
import contextlib
import inspect

import pytest
import torch

from tests import attn_exact as ax
from tests import attn_run_forms as rf
from tests import issue_contract as ic
from tests import kernel_forms as kf
from tests import nn_exact as nx
from tests.test_mem_contract_gpu import _attn_ws_bytes
from tests.test_nn_exact_gpu import SMALL, Prop, _calls

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
F32 = torch.float32
DT_ID = {torch.bfloat16: "bf16", torch.float16: "f16"}


def _ops():
    from tokenflow_amd import ops
    return ops


def _randn(shape, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda").to(dtype)


def _full(shape, dtype, fill=ax.SENTINEL):
    return lambda: torch.full(tuple(shape), fill, dtype=dtype, device="cuda")


@contextlib.contextmanager
def _requests(ops):
    """The (tag, bytes) scratch requests made inside the block."""
    inner, seen = ops._workspace, []

    def spy(nbytes, device, tag="attn", stream=None):
        seen.append((tag, int(nbytes)))
        return inner(nbytes, device, tag, stream)
    ops._workspace = spy
    try:
        yield seen
    finally:
        ops._workspace = inner


def _ws_bytes(ops, bundle):
    """The eager scratch of the bundle's call (what the wrapper asks `_workspace` for: its size function's answer, at least the
    1 MiB the cache allocates)."""
    with _requests(ops) as seen:
        bundle.eager(bundle.A)
    return max([max(n, 1 << 20) for _, n in seen], default=0)


def _check(bundle, protocols=ic.ALL, larger=None):
    ops = _ops()
    ws = _ws_bytes(ops, bundle) if "P3" in protocols else 0
    ic.check(bundle, None, None, None, None, protocols=protocols, drop=ops.drop_workspaces, cache=lambda: ops._ws_cache,
             ws_bytes=ws, larger=larger)


# ----------------------------------------------------------------------------------------------------------- attention
def _attn_bundle(case, mode, dtype):
    ops, spec = _ops(), case.spec
    nq, nk = spec.nbr * spec.Kq, spec.nbr * spec.K

    def gen(seed):
        return [_randn((n, spec.S, spec.D), dtype, seed + i) for i, n in enumerate((nq, nk, nk))]
    return ic.Bundle(lambda t, out: case.call(ops, t[0], t[1], t[2], out, **mode), gen(1000 + 7 * case.seed), gen(5000 + 7 * case.seed),
                     _full((nq, spec.S, spec.D), dtype), f"{case.name} {mode} {DT_ID[dtype]}")


def _plan_key(ops, case, mode, dtype):
    return (DT_ID[dtype], str(case.plan(ops, dtype, dtype, **mode)))


def _plan_subset():
    """The first (case, mode) of every distinct launch plan, per dtype, in table order."""
    ops, first = _ops(), {}
    for name, case in ax.GPU_CASES.items():
        for m, mode in enumerate(case.modes):
            for dtype in DTYPES:
                first.setdefault(_plan_key(ops, case, mode, dtype), (name, m, dtype))
    return first


PLAN_SUBSET = _plan_subset()
_largest = {}


def _tag(name):
    return "attn_runs" if name in ax.RUN_CASES else "attn"


def _larger_attn(name, dtype):
    """The case of the same scratch tag with the largest scratch (None for that case itself)."""
    ops = _ops()
    key = (_tag(name), dtype)
    if key not in _largest:
        sizes = {n: _attn_ws_bytes(ops, n, c.spec, dtype) for n, c in ax.GPU_CASES.items() if _tag(n) == key[0]}
        big = max(sizes, key=sizes.get)
        _largest[key] = (big, sizes, _attn_bundle(ax.GPU_CASES[big], ax.GPU_CASES[big].modes[0], dtype))
    big, sizes, bundle = _largest[key]
    return bundle if sizes[big] > sizes[name] else None


def test_every_attention_case_is_covered():
    """P1 + P2 run on every case (the parametrisation below is the table); P3 + P4 on a subset in which every plan token occurs."""
    ops = _ops()
    assert [n for n in ATTN_NAMES] == list(ax.GPU_CASES)
    tokens = {t for c in ax.GPU_CASES.values() for m in c.modes for d in DTYPES for t in _flat_tokens(c.plan(ops, d, d, **m))}
    chosen = {t for name, m, d in PLAN_SUBSET.values()
              for t in _flat_tokens(ax.GPU_CASES[name].plan(ops, d, d, **ax.GPU_CASES[name].modes[m]))}
    assert tokens and chosen == tokens
    assert {_plan_key(ops, c, m, d) for c in ax.GPU_CASES.values() for m in c.modes for d in DTYPES} == set(PLAN_SUBSET)


def _flat_tokens(plan):
    return [t for p in plan for t in (_flat_tokens(p) if isinstance(p, (list, tuple)) else [p])]


ATTN_NAMES = list(ax.GPU_CASES)


@pytest.mark.parametrize("name", ATTN_NAMES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.values())
def test_attention_late_inputs_and_no_wait(name, dtype):
    case = ax.GPU_CASES[name]
    for mode in case.modes:
        _check(_attn_bundle(case, mode, dtype), ("P1", "P2"))


@pytest.mark.parametrize("name,m,dtype", list(PLAN_SUBSET.values()), ids=[f"{n}-m{m}-{DT_ID[d]}" for n, m, d in PLAN_SUBSET.values()])
def test_attention_graph_replay_and_beside_itself(name, m, dtype):
    case = ax.GPU_CASES[name]
    _check(_attn_bundle(case, case.modes[m], dtype), ("P3", "P4"), larger=_larger_attn(name, dtype))


# ------------------------------------------------------------------------------------------- the _views / _part wrappers
VIEW_SHAPES = {"fused": (48, 2, 40, {}), "streaming": (320, 2, 64, {"fused": False})}
P5_SHAPES = {"small": (320, 2, 40, {"fused": False}), "large": (320, 2, 64, {"fused": False})}      # both write their scratch (vt_pack)
VK, VKQ, VF0 = 4, 2, 1                                  # a bank part: query frames 1, 2 of a 4-frame bank
VWIN = [(0, 3), (1, 3)]
VSETS = [ax.mask(0, 1, 3), ax.mask(2, 3)]
VE, VMASK = 2, 0b01
WITH_STREAM = ["ext_attn_views", "ext_attn_windows_views", "ext_attn_frame_sets_views"]
RUN_VIEWS = ["ext_attn_runs_views", "ext_attn_runs_edits_views"]
VIEWS = WITH_STREAM + ["ext_attn_edits_views", "ext_attn_windows_edits_views", "ext_attn_frame_sets_edits_views"] + RUN_VIEWS


def _view_plan(ops, wrapper, S, H, d, kw, dtype):
    a = dict(dtype=dtype, no_split=False, **kw)
    if wrapper == "ext_attn_views":
        return ops.attn_plan(VK, VKQ, S, H, d, False, part="bank", **a)
    if wrapper == "ext_attn_windows_views":
        return ops.attn_windows_part_plan(VK, VKQ, VF0, VWIN, S, H, d, False, **a)
    if wrapper == "ext_attn_frame_sets_views":
        return ops.attn_frame_sets_part_plan(VK, VKQ, VF0, VSETS, S, H, d, False, **a)
    if wrapper == "ext_attn_edits_views":
        return ops.attn_edits_part_plan(VK, VKQ, S, H, d, VE, VMASK, part="bank", **a)
    if wrapper == "ext_attn_windows_edits_views":
        return ops.attn_windows_edits_part_plan(VK, VKQ, VF0, VWIN, S, H, d, VE, VMASK, **a)
    if wrapper == "ext_attn_frame_sets_edits_views":
        return ops.attn_frame_sets_edits_part_plan(VK, VKQ, VF0, VSETS, S, H, d, VE, VMASK, **a)
    g = rf.BASE
    if wrapper == "ext_attn_runs_views":
        return [ops.attn_run_plan(g["K"], g["Kq"], n, len(g["runs"]), S, H, d, False, dtype=dtype, bank_only=r != 0)
                for r, (_f0, n) in enumerate(g["runs"])]
    return [ops.attn_run_edits_plan(g["K"], g["Kq"], n, len(g["runs"]), S, H, d, VE, VMASK, dtype=dtype, bank_only=r != 0)
            for r, (_f0, n) in enumerate(g["runs"])]


def _view_bundle(wrapper, form, dtype, stream="current", streams=None, seed=0):
    """The wrapper on column slabs of fused projection outputs: q = columns D..2D of [branches, Kq, S, 3D], k and v columns 0..D
    and 2D..3D of [branches, K, S, 3D].  stream: "current" (no keyword), "own" (stream= the raw handle of the stream the call is
    issued on), or a raw handle."""
    ops = _ops()
    S, H, d, kw = {**VIEW_SHAPES, **P5_SHAPES}[form]
    D, scale = H * d, d ** -0.5
    run = wrapper in RUN_VIEWS
    edits = "edits" in wrapper
    g = rf.BASE
    K, Kq, f0 = (g["K"], g["Kq"], g["q_frame0"]) if run else (VK, VKQ, VF0)
    nbr = 1 + 2 * VE if edits else 3
    plan = _flat_tokens(_view_plan(ops, wrapper, S, H, d, {} if run else kw, dtype))
    if run:
        assert any(t.endswith(",run>") for t in plan), plan
    else:
        assert any(t.startswith("fused[") for t in plan) == (form == "fused"), plan
    A = [_randn((nbr, Kq, S, 3 * D), dtype, 11 + seed), _randn((nbr, K, S, 3 * D), dtype, 12 + seed)]
    B = [_randn((nbr, Kq, S, 3 * D), dtype, 13 + seed), _randn((nbr, K, S, 3 * D), dtype, 14 + seed)]

    def call(t, out):
        q, k, v = t[0][..., D:2 * D], t[1][..., :D], t[1][..., 2 * D:]
        skw = {}
        if stream != "current":
            skw["stream"] = torch.cuda.current_stream().cuda_stream if stream == "own" else stream
        if wrapper == "ext_attn_views":
            ops.ext_attn_views(q, k, v, out, H, scale, False, "bank", q_frame0=f0, **kw, **skw)
        elif wrapper == "ext_attn_windows_views":
            ops.ext_attn_windows_views(q, k, v, out, H, scale, False, VWIN, "bank", q_frame0=f0, **kw, **skw)
        elif wrapper == "ext_attn_frame_sets_views":
            ops.ext_attn_frame_sets_views(q, k, v, out, H, scale, False, VSETS, "bank", q_frame0=f0, **kw, **skw)
        elif wrapper == "ext_attn_edits_views":
            ops.ext_attn_edits_views(q, k, v, out, H, scale, VE, VMASK, "bank", q_frame0=f0, **kw)
        elif wrapper == "ext_attn_windows_edits_views":
            ops.ext_attn_windows_edits_views(q, k, v, out, H, scale, VE, VMASK, VWIN, "bank", q_frame0=f0, **kw)
        elif wrapper == "ext_attn_frame_sets_edits_views":
            ops.ext_attn_frame_sets_edits_views(q, k, v, out, H, scale, VE, VMASK, VSETS, "bank", q_frame0=f0, **kw)
        elif wrapper == "ext_attn_runs_views":
            kv = [(k[:, r0:r0 + n], v[:, r0:r0 + n], 0, 0) for r0, n in g["runs"]]
            ops.ext_attn_runs_views(q, kv, out, H, scale, False, g["runs"], K, q_frame0=f0, streams=streams)
        else:
            kv = [(k[:, r0:r0 + n], v[:, r0:r0 + n], 0, 0, False) for r0, n in g["runs"]]
            ops.ext_attn_runs_edits_views(q, kv, out, H, scale, VE, VMASK, g["runs"], K, q_frame0=f0, streams=streams)
    what = f"{wrapper} {form} {DT_ID[dtype]}" + ("" if stream == "current" else " stream=") + (" streams=" if streams else "")
    return ic.Bundle(call, A, B, _full((nbr, Kq, S, D), dtype), what)


@pytest.mark.parametrize("wrapper", VIEWS)
@pytest.mark.parametrize("form", list(VIEW_SHAPES))
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.values())
def test_views_wrappers(wrapper, form, dtype):
    larger = _view_bundle(wrapper, "streaming", dtype, seed=100) if form == "fused" else None
    _check(_view_bundle(wrapper, form, dtype), larger=larger)


@pytest.mark.parametrize("wrapper", WITH_STREAM)
@pytest.mark.parametrize("form", list(VIEW_SHAPES))
def test_views_wrappers_captured_with_an_explicit_stream(wrapper, form):
    """P3 with stream= the capturing stream's raw handle (and P1, P2, P4 with stream= the stream the call is issued on): scratch
    asked for while that stream is capturing is the graph's, never cached (S1)."""
    larger = _view_bundle(wrapper, "streaming", torch.bfloat16, stream="own", seed=100) if form == "fused" else None
    _check(_view_bundle(wrapper, form, torch.bfloat16, stream="own"), larger=larger)


@pytest.mark.parametrize("wrapper", RUN_VIEWS)
@pytest.mark.parametrize("form", list(VIEW_SHAPES))
def test_run_wrappers_on_their_own_streams(wrapper, form):
    """streams=: the runs are forked behind the caller's stream and joined in front of the merge (P1 only: not captured)."""
    streams = [None, torch.cuda.Stream(), torch.cuda.Stream()]
    _check(_view_bundle(wrapper, form, torch.bfloat16, streams=streams), ("P1", "P2"))


# ---- P5
FILL5 = 0x5A


def foreign_stream_scratch(ops, wrapper, dtype=torch.bfloat16):
    """The P5 sequence; returns a dict of what was seen (the test below asserts on it)."""
    side = torch.cuda.Stream()
    raw = side.cuda_stream
    small, large = (_view_bundle(wrapper, f, dtype, seed=i) for i, f in enumerate(("small", "large")))
    s_raw, l_raw = (_view_bundle(wrapper, f, dtype, stream=raw, seed=i) for i, f in enumerate(("small", "large")))
    want_s, want_l = small.ref()[1], large.ref()[1]
    ops.drop_workspaces()
    ws, wl, os_, ol = s_raw.work(s_raw.B), l_raw.work(l_raw.B), s_raw.make_out(), l_raw.make_out()
    torch.cuda.synchronize()
    key = ("attn", torch.cuda.current_device(), raw)
    d = ic.Delay(side)
    s_raw.call(ws, os_)
    ptr0, size0 = ops._ws_cache[key].data_ptr(), ops._ws_cache[key].numel()
    l_raw.call(wl, ol)
    replaced = ops._ws_cache[key].numel() > size0
    T = torch.empty(size0, dtype=torch.uint8, device="cuda")
    T.fill_(FILL5)
    pending = not d.t1.query()
    side.synchronize()
    torch.cuda.synchronize()
    d.verify(f"{wrapper} P5")
    seen = dict(replaced=replaced, pending=pending, handed_back=T.data_ptr() == ptr0, intact=bool((T == FILL5).all()),
                small_ok=ic.same_bits(os_, want_s[0]), large_ok=ic.same_bits(ol, want_l[0]))
    # control: a block of that size dropped on the CURRENT stream is what the next request of that size gets
    ops.drop_workspaces()
    del T
    c = torch.empty(size0, dtype=torch.uint8, device="cuda")
    p = c.data_ptr()
    del c
    c2 = torch.empty(size0, dtype=torch.uint8, device="cuda")
    seen["control"] = c2.data_ptr() == p
    return seen


@pytest.mark.parametrize("wrapper", WITH_STREAM)
def test_scratch_for_a_foreign_stream(wrapper):
    ops = _ops()
    seen = foreign_stream_scratch(ops, wrapper)
    print(f"P5 {wrapper}: {seen}")
    if not (seen["replaced"] and seen["pending"] and seen["control"]):
        pytest.fail(f"P5 {wrapper}: not exercised: {seen} (the cache entry must be replaced while the stream is still busy, and the "
                    "allocator must hand a block dropped on the current stream straight back)")
    assert not seen["handed_back"], (f"P5 {wrapper}: the outgrown scratch of a foreign stream was handed to the current stream while "
                                     f"launches that use it were still queued ({seen})")
    assert seen["intact"], f"P5 {wrapper}: a buffer allocated on the current stream was written by a queued launch ({seen})"
    assert seen["small_ok"] and seen["large_ok"], f"P5 {wrapper}: a result differs from its eager reference ({seen})"


# --------------------------------------------------------------------------------------------- NN search and propagation
@pytest.mark.parametrize("form,i", nx.NN_CASES, ids=[f"{f}-{i}" for f, i in nx.NN_CASES])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.values())
def test_nn_search(form, i, dtype):
    """C = 1 cases through `ops.nn_search`; C > 1 cases as test_search_exact runs them: `ops.propagate_chunks` (first_single) on an
    index-coded cache (set B's code is shifted by S, so every row differs whatever the indices)."""
    ops = _ops()
    c = kf.CASES[form][i]
    assert form in [kf.form(t) for t in kf.plan(ops, c)]
    n_tgt, S, D, C, P = c["n_tgt"], c["S"], c["D"], c["C"], c["P"]
    sets = []
    for family in ("dense", "pool"):
        inp = nx.Inputs.of_case(c, family)
        piv = inp.pivots("cuda", dtype, False)
        tgt = torch.cat([inp.targets(j, "cuda") for j in range(C)]).to(dtype)
        sets.append([tgt, piv, ops.pivot_inv_norm(piv)])
    chunks, K, n = inp.chunks, inp.K, n_tgt // S
    if C == 1:
        b = ic.Bundle(lambda t, out: ops.nn_search(t[0], t[1], t[2], chunks[0], idx=out), sets[0], sets[1],
                      _full((P, n_tgt), torch.int32, -7), f"nn_search {form}-{i} {DT_ID[dtype]}")
    else:
        rows = torch.arange(S, dtype=F32, device="cuda")
        for x, shift in zip(sets, (0, S)):
            code = torch.zeros(3, K, S, D, dtype=F32, device="cuda")
            code[:, 0::2, :, 0] = rows + shift
            code[:, 1::2, :, 1] = rows + shift
            x.append(code.view(3 * K, S, D))
        w = torch.full((n,), 0.5, device="cuda")
        b = ic.Bundle(lambda t, out: ops.propagate_chunks(t[0], t[1], t[2], t[3], w, n, C, 0, True, None, F32, out=out), sets[0], sets[1],
                      _full((3 * C * n, S, D), F32), f"propagate_chunks (search case {form}-{i}) {DT_ID[dtype]}")
    _check(b)


class Recorder:
    """`ops` as tests.test_nn_exact_gpu._calls sees it: every propagate* call is made and recorded (name, args, keywords, result), so
    that the same form can be issued again -- on other tensors, into given buffers, on another stream.  Everything else is the
    module's."""
    FORMS = ("propagate", "propagate_chunks", "propagate_chunks_segments", "propagate_chunks_edits")

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if name not in self.FORMS:
            return fn

        def rec(*args, **kw):
            got = fn(*args, **kw)
            self.calls.append((name, args, kw, got))
            return got
        return rec


def _form_bundle(ops, rec_a, rec_b, what):
    """One recorded form: set A its tensors, set B those of the other recording -- other targets, pivots and inverse norms; the
    keyframe outputs and the residual, which the two recordings share, are fresh N(0,1) values in B (A keeps the edge values)."""
    name, args, kw, got = rec_a
    assert rec_b[0] == name and len(rec_b[1]) == len(args)
    pos = [i for i, a in enumerate(args) if isinstance(a, torch.Tensor)]
    A = [args[i] for i in pos]
    B = [_randn(x.shape, x.dtype, 90 + i) if x.dim() == 3 and torch.equal(x, args[i]) else x for i, x in ((i, rec_b[1][i]) for i in pos)]
    outs = got if isinstance(got, tuple) else (got,)
    names = ("out", "norm_out")[:len(outs)]

    def call(t, out):
        a = list(args)
        for i, x in zip(pos, t):
            a[i] = x
        getattr(ops, name)(*a, **kw, **dict(zip(names, ic._flat(out))))

    def make_out():
        o = tuple(torch.full(x.shape, ax.SENTINEL, dtype=x.dtype, device="cuda") for x in outs)
        return o if len(o) > 1 else o[0]
    return ic.Bundle(call, A, B, make_out, what)


@pytest.mark.parametrize("S,D,kernel", SMALL, ids=[f"{c[2]}-S{c[0]}-D{c[1]}" for c in SMALL])
@pytest.mark.parametrize("fused_norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.values())
def test_propagation(S, D, kernel, fused_norm, dtype):
    ops = _ops()
    n = 3 if S == 96 else 2
    g = torch.Generator().manual_seed(D)
    gamma = (1 + 0.2 * torch.randn(D, generator=g)).to(dtype).cuda()
    beta = (0.1 * torch.randn(D, generator=g)).to(dtype).cuda()
    recs = []
    for family in ("pool", "dense"):
        pr = Prop(S, D, n, family, dtype, huge=not fused_norm)
        rec = Recorder(ops)
        for _ in _calls(rec, pr, ops.pivot_inv_norm(pr.piv), norm=(gamma, beta, 1e-5, dtype) if fused_norm else None):
            pass
        recs.append(rec.calls)
    count = (2 + 2 + 3 + 4 if fused_norm else 3 * 3 + (2 + 4 + 2) + 2 * (3 + 4))      # as the tests of test_nn_exact_gpu count them
    assert len(recs[0]) == len(recs[1]) == count
    larger = None
    for k, (a, b) in enumerate(zip(*recs)):
        kw = {x: y for x, y in a[2].items() if x != "norm"}
        bundle = _form_bundle(ops, a, b, f"{a[0]} #{k} S{S} D{D} {DT_ID[dtype]}{' norm' if fused_norm else ''} "
                                         f"{[x for x in a[1] if not isinstance(x, torch.Tensor)]} {kw}")
        if k == 0:      # the one-keyframe `propagate`: the smallest scratch of the shape; the chunk forms outgrow it
            first = bundle
        if a[0] == "propagate_chunks" and larger is None:
            larger = bundle
        _check(bundle)
    _check(first, ("P3", "P4"), larger=larger)


# ---------------------------------------------------------------------------------------------------- the small kernels
def _gen(shapes, dtype, seed, scale=1.0, shift=0.0):
    return [(_randn(s, F32, seed + i) * scale + shift).to(dtype) for i, s in enumerate(shapes)]


def _small_bundles(dtype):
    ops = _ops()
    out = {}

    def add(name, call, A, B, make_out):
        out[name] = ic.Bundle(call, A, B, make_out, f"{name} {DT_ID[dtype]}")
    K, S, D = 2, 45, 72
    add("pivot_inv_norm", lambda t, o: ops.pivot_inv_norm(t[0], out=o), _gen([(K, S, D)], dtype, 1), _gen([(K, S, D)], dtype, 2),
        _full((K, S), F32))
    lr, lD = 5, 72
    add("layer_norm", lambda t, o: ops.layer_norm(t[0], t[1], t[2], 1e-5, dtype, want_inv_norm=True, out=o[0], inv_out=o[1]),
        _gen([(lr, lD), (lD,), (lD,)], dtype, 3, 3.0, 0.5), _gen([(lr, lD), (lD,), (lD,)], dtype, 6, 3.0, 0.5),
        lambda: (_full((lr, lD), dtype)(), _full((lr,), F32)()))
    add("add_layer_norm", lambda t, o: ops.add_layer_norm(t[0], t[1], t[2], t[3], 1e-5, dtype, total=o[0], out=o[1]),
        _gen([(lr, lD), (lr, lD)], dtype, 9, 2.0) + _gen([(lD,), (lD,)], F32, 11),
        _gen([(lr, lD), (lr, lD)], dtype, 13, 2.0) + _gen([(lD,), (lD,)], F32, 15),
        lambda: (_full((lr, lD), dtype)(), _full((lr, lD), dtype)()))
    # gather_blend on the indices the search found (the same valid indices for both sets: they are no input of the protocol)
    K, n, S, D = 2, 2, 45, 72
    piv, tgt = _randn((K, S, D), dtype, 17), _randn((n * S, D), dtype, 18)
    idx = ops.nn_search(tgt, piv, ops.pivot_inv_norm(piv), [1, 0])
    w = torch.tensor([0.25, 0.75], device="cuda")
    add("gather_blend", lambda t, o, n=n: ops.gather_blend(t[0], idx, w, [1, 0], n, t[1], F32, out=o),
        _gen([(3 * K, S, D), (3 * n, S, D)], dtype, 19), _gen([(3 * K, S, D), (3 * n, S, D)], dtype, 21), _full((3 * n, S, D), F32))

    def inject(t, o):
        o.copy_(t[0])
        ops.inject_copy_(o)
    add("inject_copy_", inject, _gen([(6, 5, 7, 4)], dtype, 23), _gen([(6, 5, 7, 4)], dtype, 24), _full((6, 5, 7, 4), dtype))
    E, n = 3, 2

    def inject_edits(t, o):
        o.copy_(t[0])
        ops.inject_copy_edits_(o, E, edit_mask=0b101)
    shape = ((1 + 2 * E) * n, 5, 7, 4)
    add("inject_copy_edits_", inject_edits, _gen([shape], dtype, 25), _gen([shape], dtype, 26), _full(shape, dtype))
    co = (0.9734, 0.2291, 0.9581, 0.2864)
    add("ddim_step", lambda t, o: ops.ddim_step(t[0], t[1], *co, out=o), _gen([(257,), (257,)], dtype, 27), _gen([(257,), (257,)], dtype, 29),
        _full((257,), dtype))
    pW, pKl, pS, pD = 2, 2, 45, 80
    hd = pD // pW

    def pack(t, o):
        q3, k3, v3 = (t[0][..., i * pD:(i + 1) * pD].unflatten(0, (3, pKl)) for i in range(3))
        ops.head_pack([q3[1], q3[2], k3[1], k3[2], v3[1], v3[2]], pW, out=o)
    add("head_pack", pack, _gen([(3 * pKl, pS, 3 * pD)], dtype, 31), _gen([(3 * pKl, pS, 3 * pD)], dtype, 32), _full((pW, pKl, 6, pS, hd), dtype))
    add("head_unpack", lambda t, o: ops.head_unpack(t[0], [o[1], o[2]]), _gen([(pW, pKl, 2, pS, hd)], dtype, 33),
        _gen([(pW, pKl, 2, pS, hd)], dtype, 34), _full((3, pKl, pS, pD), dtype))
    wKl, wS, wD = 3, 72, 80
    segs = [(0, 3), (0, 3), (2, 1)]

    def wpack(t, o):
        k3, v3 = t[0][..., wD:2 * wD], t[0][..., 2 * wD:]
        ops.window_halo_pack([k3[1], k3[2], v3[1], v3[2]], segs, out=o)
    add("window_halo_pack", wpack, _gen([(3, wKl, wS, 3 * wD)], dtype, 35), _gen([(3, wKl, wS, 3 * wD)], dtype, 36), _full((7, 4, wS, wD), dtype))
    Kl, S, D, ns = 3, 3, 8, 3
    masks = [0b000, 0b111, 0b101]

    def slabs_of(buf, k):
        return [buf[i, :Kl, 1:1 + S, D * (i % 3):D * (i % 3) + D] for i in range(k)]
    add("frame_set_halo_pack", lambda t, o: ops.frame_set_halo_pack(slabs_of(t[0], ns), masks, out=o),
        _gen([(6, Kl + 1, S + 2, 3 * D)], dtype, 37), _gen([(6, Kl + 1, S + 2, 3 * D)], dtype, 38), _full((5, ns, S, D), dtype))
    nq = 3
    add("edit_halo_pack", lambda t, o: ops.edit_halo_pack(slabs_of(t[0], 7), masks, [t[1][i, :, :S, D:] for i in range(nq)], out=o[0],
                                                         q_out=o[1]),
        _gen([(7, Kl + 1, S + 2, 3 * D), (3, Kl, S + 1, 2 * D)], dtype, 39), _gen([(7, Kl + 1, S + 2, 3 * D), (3, Kl, S + 1, 2 * D)], dtype, 41),
        lambda: (_full((5, 7, S, D), dtype)(), _full((nq, Kl, S, D), dtype)()))
    return out


SMALL_KERNELS = ["pivot_inv_norm", "layer_norm", "add_layer_norm", "gather_blend", "inject_copy_", "inject_copy_edits_", "ddim_step",
                 "head_pack", "head_unpack", "window_halo_pack", "frame_set_halo_pack", "edit_halo_pack"]


@pytest.mark.parametrize("kernel", SMALL_KERNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.values())
def test_small_kernels(kernel, dtype):
    bundles = _small_bundles(dtype)
    assert list(bundles) == SMALL_KERNELS
    _check(bundles[kernel])


# ------------------------------------------------------------------------------------------------------- rank executors
RK, RS, RDH = 6, 64, 40         # rank 1 of a 3-rank loopback world holds keyframes 2, 3 of 6


def _shard_bundle(sh, what, H, nbr, call):
    Kl, D = sh.Kl, H * RDH
    A = [_randn((nbr * Kl, RS, D), torch.bfloat16, 50 + i) for i in range(3)]
    B = [_randn((nbr * Kl, RS, D), torch.bfloat16, 60 + i) for i in range(3)]

    def run(t, out):
        out.copy_(call(t[0], t[1], t[2]))
    return ic.Bundle(run, A, B, _full((nbr * Kl, RS, D), torch.bfloat16), what)


EXECUTOR_CALLS = ["heads", "bank", "bank_runs", "window", "window+anchor", "edits", "window_edits", "block+halo"]


@pytest.mark.parametrize("which", EXECUTOR_CALLS)
def test_rank_executors(which):
    """One pass of a native rank executor on rank 1 of a 3-rank loopback world (what is received is this rank's own data: a
    function of the inputs like everything else).  The executor forks its own auxiliary, exchange and halo streams: P1 checks
    that those forks sit behind the caller's pending work, P2 that the pass does not wait.  Not captured."""
    from tokenflow_amd import sharded
    from tokenflow_amd.comm import HipComm
    ops = _ops()
    scale = RDH ** -0.5
    comms, sh = [HipComm.loopback(1, 3), HipComm.loopback(1, 3)], None
    try:
        if which in ("heads", "bank", "bank_runs"):
            H = 3 if which == "heads" else 2
            sh = sharded.NativeShard(RK, comms[0], comms[1], bank_runs=True if which == "bank_runs" else None)
            b = _shard_bundle(sh, f"NativeShard.pivotal_attention {which}", H, 3,
                              lambda q, k, v: sh.pivotal_attention(q, k, v, H, scale, True, mode=which))
        elif which in ("window", "window+anchor"):
            H, anchors = 2, (0,) if which == "window+anchor" else None
            sh = sharded.NativeShard(RK, comms[0], comms[1])
            b = _shard_bundle(sh, f"NativeShard.pivotal_attention {which}", H, 3,
                              lambda q, k, v: sh.pivotal_attention(q, k, v, H, scale, True, window=1, anchors=anchors))
        elif which == "edits":
            H = 2
            sh = sharded.NativeEditShard(RK, comms[0], comms[1])
            b = _shard_bundle(sh, "NativeEditShard.pivotal_attention E=2", H, 5,
                              lambda q, k, v: sh.pivotal_attention(q, k, v, H, scale, False, mode="bank", n_edits=2, inject_mask=0b01))
        elif which == "window_edits":
            H = 2
            sh = sharded.NativeEditShard(RK, comms[0], comms[1], window_edits=True)
            b = _shard_bundle(sh, "NativeEditShard.pivotal_attention E=2 window=1", H, 5,
                              lambda q, k, v: sh.pivotal_attention(q, k, v, H, scale, False, n_edits=2, inject_mask=0b01, window=1))
        else:
            H = 2
            D = H * RDH
            sh = sharded.NativeShard(RK, comms[0], comms[1])
            Kl = sh.Kl
            ext = sh.ext_alloc(RS, D, torch.bfloat16, torch.device("cuda", torch.cuda.current_device()))
            A = [_randn((3 * Kl, RS, D), torch.bfloat16, 70 + i) for i in range(3)] + [_randn((Kl, RS, D), torch.bfloat16, 73)]
            B = [_randn((3 * Kl, RS, D), torch.bfloat16, 80 + i) for i in range(3)] + [_randn((Kl, RS, D), torch.bfloat16, 83)]

            def block(t, out):
                for e in ext:
                    e.zero_()
                ext[0][1:].copy_(t[3])
                pe, ie, ke, reqs = sh.pivotal_block(t[0], t[1], t[2], H, scale, True, ext, mode="bank", inv_norm=True)
                assert len(reqs) == 1
                for r in reqs:
                    r.wait()        # the slot wait the block returned, on the caller's stream
                out[0].copy_(ke)
                out[1].copy_(pe)
                out[2].copy_(ie)
            b = ic.Bundle(block, A, B, lambda: (_full((3 * (Kl + 1), RS, D), torch.bfloat16)(), _full((Kl + 1, RS, D), torch.bfloat16)(),
                                                _full((Kl + 1, RS), F32)()), "NativeShard.pivotal_block with the halo")
        _check(b, ("P1", "P2"))
    finally:
        torch.cuda.synchronize()
        if sh is not None:
            sh.close()
        for c in comms:
            c.close()


def test_every_listed_entry_point_is_covered():
    ops = _ops()
    assert all(hasattr(ops, w) for w in VIEWS + SMALL_KERNELS)
    assert set(Recorder.FORMS) == {"propagate", "propagate_chunks", "propagate_chunks_segments", "propagate_chunks_edits"}
    assert all("stream" in inspect.signature(getattr(ops, w)).parameters for w in WITH_STREAM)
