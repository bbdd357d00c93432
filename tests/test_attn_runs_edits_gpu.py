"""The run form of the multi-edit attention (ops.ext_attn_runs_edits: tf_ext_attn_run_edits + tf_ext_attn_runs_merge_edits)
on an MI355X: run sets on the BASE geometry of tests/attn_run_forms.py.

Inputs are independent N(0,1) q, k, v per branch, rounded once to the dtype: a launch that reads a neighbouring edit's bank,
or the source's q / k for an edit that does not inject, lands O(1) outside the bound.  A HIP result is compared with the
fp32 oracle under the attention bound of tests/test_kernels_gpu.py (per edit, on [source | uncond_e | cond_e] with that
edit's flag), or bit for bit with another HIP result.  No tolerance between two HIP results appears in this file.
"""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import tokenflow_oracle as orc  # noqa: E402
from tests import attn_run_edit_forms as ef  # noqa: E402
from tests.test_kernels_gpu import assert_attn_close, attn_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
CASES = ef.CASES


def _ops():
    from tokenflow_amd import ops
    return ops


def _rnd(dtype):
    return orc.bf16_round if dtype == torch.bfloat16 else (lambda x: x.half().float())


def _nbr(c):
    return 1 + 2 * c["n_edits"]


@functools.lru_cache(maxsize=None)
def _inputs(S, H, dh, K, E, dtype):
    """fp32 (rounded to dtype) q, k, v [B*K, S, D] on the CPU; the same for every mask of a shape."""
    g = torch.Generator().manual_seed(17 + S + dh + E)
    return tuple(_rnd(dtype)(torch.randn((1 + 2 * E) * K, S, H * dh, generator=g)) for _ in range(3))


def _qkv(c, dtype):
    return _inputs(c["S"], c["heads"], c["dh"], c["K"], c["n_edits"], dtype)


def _rows(t, c, nbr):
    """Rows of a [nbr*K, S, D] tensor that belong to the query frames: [nbr*Kq, S, D]."""
    K, q0, Kq = c["K"], c["q_frame0"], c["Kq"]
    return t.view(nbr, K, *t.shape[1:])[:, q0:q0 + Kq].reshape(nbr * Kq, *t.shape[1:])


def _edit3(t, e, n):
    """[source | uncond_e | cond_e] of a [B*n, S, D] tensor: [3n, S, D]."""
    return torch.cat([t[:n], t[(1 + 2 * e) * n:(3 + 2 * e) * n]])


@functools.lru_cache(maxsize=None)
def _dev(S, H, dh, K, E, dtype):
    return tuple(t.to(dtype).cuda() for t in _inputs(S, H, dh, K, E, dtype))


def _run(ops, c, dtype, **kw):
    dq, dk, dv = _dev(c["S"], c["heads"], c["dh"], c["K"], c["n_edits"], dtype)
    return ops.ext_attn_runs_edits(_rows(dq, c, _nbr(c)).contiguous(), dk, dv, c["heads"], c["dh"] ** -0.5, c["n_edits"],
                                   c["mask"], c["runs"], q_frame0=c["q_frame0"], **kw)


@functools.lru_cache(maxsize=None)
def _base(i, dtype):
    """The in-order, one-stream result of case i (shared by the tests that compare against it; never written to)."""
    return _run(_ops(), CASES[i], dtype)


@functools.lru_cache(maxsize=None)
def _edit_refs(S, H, dh, K, E, e, inject, dtype):
    q, k, v = _inputs(S, H, dh, K, E, dtype)
    return attn_ref(_edit3(q, e, K), _edit3(k, e, K), _edit3(v, e, K), H, dh ** -0.5, inject, need_sigma=False)


IDX = list(range(len(CASES)))
_id = lambda i: ef.case_id(CASES[i])  # noqa: E731


def test_cases_cover_the_run_forms():
    ops = _ops()
    toks = {t for c in CASES for p in ef.case_plans(ops, c) for t in p}
    for dh in (40, 64, 80):
        assert any(f"<{dh}," in t and ",DUAL," in t and t.endswith(",run>") for t in toks), (dh, sorted(toks))
    for dh in (40, 64, 80, 160):
        assert any(f"<{dh}," in t and ",ALL," in t and t.endswith(",run>") for t in toks), (dh, sorted(toks))
    assert "merge[runs=3,edits=2]" in toks and "merge[runs=3,edits=3]" in toks


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("i", IDX, ids=_id)
def test_every_edit_and_the_source_vs_oracle(i, dtype):
    c = CASES[i]
    out = _base(i, dtype)
    assert torch.isfinite(out.float()).all()
    Kq = c["Kq"]
    for e in range(c["n_edits"]):
        inj = bool((c["mask"] >> e) & 1)
        refs = _edit_refs(c["S"], c["heads"], c["dh"], c["K"], c["n_edits"], e, inj, dtype)
        refs = tuple(None if r is None else _rows(r, c, 3) for r in refs)
        err = assert_attn_close(_edit3(out, e, Kq), refs, f"{_id(i)} edit {e}", dtype=dtype)
        print(f"{_id(i)} {dtype} edit {e}: max abs err {err:.3e}")


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("i", IDX, ids=_id)
def test_every_edit_equals_its_single_edit_run_set(i, dtype):
    """Bank branches and source branch of edit e == ops.ext_attn_runs on [source | uncond_e | cond_e], same runs, its flag."""
    ops = _ops()
    c = CASES[i]
    out = _base(i, dtype)
    K, Kq = c["K"], c["Kq"]
    dq, dk, dv = _dev(c["S"], c["heads"], c["dh"], K, c["n_edits"], dtype)
    dq = _rows(dq, c, _nbr(c))
    for e in range(c["n_edits"]):
        one = ops.ext_attn_runs(_edit3(dq, e, Kq), _edit3(dk, e, K), _edit3(dv, e, K), c["heads"], c["dh"] ** -0.5,
                                bool((c["mask"] >> e) & 1), c["runs"], q_frame0=c["q_frame0"])
        assert torch.equal(_edit3(out, e, Kq), one), f"{_id(i)} edit {e}"


# 3, 4 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("i", IDX, ids=_id)
def test_order_streams_and_compact_k_do_not_change_a_bit(i, dtype):
    ops = _ops()
    c = CASES[i]
    base = _base(i, dtype)
    n = len(c["runs"])
    rev = list(range(n))[::-1]
    assert torch.equal(_run(ops, c, dtype, order=rev), base)
    streams = [torch.cuda.Stream() for _ in range(n)]
    assert torch.equal(_run(ops, c, dtype, streams=streams), base)
    assert torch.equal(_run(ops, c, dtype, streams=streams, order=rev), base)
    # the remote runs read a compact k (source slot where an edit injects, then the non-injecting edits' slots)
    assert torch.equal(_run(ops, c, dtype, k_compact=True), base)
    assert torch.equal(_run(ops, c, dtype, k_compact=True, streams=streams, order=rev), base)
    torch.cuda.synchronize()


# 5 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_f32_output(dtype):
    i = next(j for j in IDX if (CASES[j]["S"], CASES[j]["dh"], CASES[j]["mask"], CASES[j]["n_edits"]) == (576, 64, 0b01, 2))
    c = CASES[i]
    out = _run(_ops(), c, dtype, out_dtype=torch.float32)
    assert out.dtype == torch.float32
    for e in range(c["n_edits"]):
        refs = _edit_refs(c["S"], c["heads"], c["dh"], c["K"], c["n_edits"], e, bool((c["mask"] >> e) & 1), dtype)
        refs = tuple(None if r is None else _rows(r, c, 3) for r in refs)
        assert_attn_close(_edit3(out, e, c["Kq"]), refs, f"f32 {_id(i)} edit {e}", dtype=dtype)
    assert torch.equal(out.to(dtype), _base(i, dtype))   # the 16-bit output is the one rounding of this accumulator


# 6 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("d", [40, 64])
def test_peaked_logits_across_runs(d, dtype):
    """Planted keys aligned with their queries (gain 12), as tests/test_attn_runs_gpu.py plants them, in every branch: for
    half of the planted queries the key lies in a REMOTE run, for the others in the local one.  Mixed mask."""
    ops = _ops()
    c = dict(S=576, heads=2, dh=d, n_edits=2, mask=0b01, K=5, Kq=2, q_frame0=2, runs=[(2, 2), (0, 2), (4, 1)])
    K, S, q0, Kq, nbr = c["K"], c["S"], c["q_frame0"], c["Kq"], 5
    g = torch.Generator().manual_seed(29 + S + d)
    q, k, v = (torch.randn(nbr * K, S, 2 * d, generator=g) for _ in range(3))
    remote = [f for f in range(K) if not q0 <= f < q0 + Kq]
    for b in range(nbr):
        for fq in range(q0, q0 + Kq):
            for j, s_ in enumerate(range(0, S, 5)):
                kf = remote[(j // 2) % len(remote)] if j % 2 == 0 else fq
                k[b * K + kf, (s_ * 3 + S - 60 + 7 * fq) % S] = q[b * K + fq, s_] * 12.0
    q, k, v = (_rnd(dtype)(x) for x in (q, k, v))
    dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
    out = ops.ext_attn_runs_edits(_rows(dq, c, nbr).contiguous(), dk, dv, 2, d ** -0.5, 2, c["mask"], c["runs"], q_frame0=q0)
    assert torch.isfinite(out.float()).all()
    for e in range(2):
        refs = attn_ref(_edit3(q, e, K), _edit3(k, e, K), _edit3(v, e, K), 2, d ** -0.5, bool((c["mask"] >> e) & 1),
                        need_sigma=False)
        refs = tuple(None if r is None else _rows(r, c, 3) for r in refs)
        assert_attn_close(_edit3(out, e, Kq), refs, f"peaked d{d} edit {e}", dtype=dtype)


# 7 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("S,H,dh", ef.SHAPES, ids=lambda x: str(x))
@pytest.mark.parametrize("inject", [False, True])
def test_one_edit_is_ext_attn_runs(S, H, dh, inject, dtype):
    ops = _ops()
    c = dict(S=S, heads=H, dh=dh, n_edits=1, mask=int(inject), K=5, Kq=2, q_frame0=2, runs=[(2, 2), (0, 2), (4, 1)])
    dq, dk, dv = _dev(S, H, dh, 5, 1, dtype)
    dq = _rows(dq, c, 3).contiguous()
    got = ops.ext_attn_runs_edits(dq, dk, dv, H, dh ** -0.5, 1, int(inject), c["runs"], q_frame0=2)
    assert torch.equal(got, ops.ext_attn_runs(dq, dk, dv, H, dh ** -0.5, inject, c["runs"], q_frame0=2))
