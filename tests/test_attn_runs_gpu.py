"""Extended attention over a bank that arrives in pieces (ops.ext_attn_runs: tf_ext_attn_run + tf_ext_attn_runs_merge) on
an MI355X.

A HIP result is compared with the fp32 oracle under the attention bound of tests/test_kernels_gpu.py (full-size cases:
the plain 1e-3 of tests/test_fullsize_gpu.py on the fp32 output), or bit for bit with another HIP result that must be the
same arithmetic.  No tolerance between two HIP results appears anywhere in this file.
"""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import tokenflow_oracle as orc  # noqa: E402
from tests import attn_run_forms as rf  # noqa: E402
from tests.test_kernels_gpu import assert_attn_close, attn_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _ops():
    from tokenflow_amd import ops
    return ops


def _unique_cases():
    seen, out = set(), []
    for f, cases in rf.CASES.items():
        for c in cases:
            if repr(c) not in seen:
                seen.add(repr(c))
                out.append(c)
    return out


CASES = _unique_cases()


def _case_id(c):
    return "K{K}q{Kq}@{q_frame0}-S{S}-H{heads}-d{dh}-inj{inject:d}-fold{fold_scale:d}-h{hints}-ns{no_split:d}".format(**c)


def _rnd(dtype):
    return orc.bf16_round if dtype == torch.bfloat16 else (lambda x: x.half().float())


def _inputs(c, dtype, seed):
    """fp32 (rounded to dtype) q, k, v of all K frames on the CPU."""
    g = torch.Generator().manual_seed(seed)
    D = c["heads"] * c["dh"]
    return tuple(_rnd(dtype)(torch.randn(3 * c["K"], c["S"], D, generator=g)) for _ in range(3))


def _rank_rows(t, c):
    """Rows of a [3K, S, D] tensor that belong to the query frames: [3Kq, S, D]."""
    K, q0, Kq = c["K"], c["q_frame0"], c["Kq"]
    return t.view(3, K, *t.shape[1:])[:, q0:q0 + Kq].reshape(3 * Kq, *t.shape[1:])


def _run(ops, c, dev, **kw):
    dq, dk, dv = dev
    return ops.ext_attn_runs(_rank_rows(dq, c).contiguous(), dk, dv, c["heads"], c["dh"] ** -0.5, c["inject"], c["runs"],
                             q_frame0=c["q_frame0"], fold_scale=c["fold_scale"], no_split=c["no_split"], hints=c["hints"],
                             **kw)


def _to_dev(qkv, dtype):
    return tuple(t.to(dtype).cuda() for t in qkv)


def test_cases_cover_every_run_form():
    ops = _ops()
    forms = {rf.form(t) for c in CASES for p in rf.case_plans(ops, c) for t in p}
    assert forms == set(rf.CASES), sorted(set(rf.CASES) ^ forms)


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_runs_vs_oracle(c, dtype):
    """Every run form, source branch included, against the oracle on the full tensors."""
    ops = _ops()
    qkv = _inputs(c, dtype, 11 + c["S"] + c["dh"])
    refs = attn_ref(*qkv, c["heads"], c["dh"] ** -0.5, c["inject"])
    refs = tuple(None if r is None else _rank_rows(r, c) for r in refs)
    out = _run(ops, c, _to_dev(qkv, dtype))
    assert torch.isfinite(out.float()).all()
    err = assert_attn_close(out, refs, _case_id(c), dtype=dtype, folded=c["fold_scale"])
    print(f"{_case_id(c)} {dtype}: max abs err {err:.3e}")


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_runs_order_and_stream_independent(c, dtype):
    """The same runs issued in reverse order, and each on a stream of its own joined by events in front of the merge:
    bit for bit the result of the in-order issue on one stream."""
    ops = _ops()
    dev = _to_dev(_inputs(c, dtype, 11 + c["S"] + c["dh"]), dtype)
    base = _run(ops, c, dev)
    n = len(c["runs"])
    rev = _run(ops, c, dev, order=list(range(n))[::-1])
    assert torch.equal(rev, base)
    streams = [torch.cuda.Stream() for _ in range(n)]
    par = _run(ops, c, dev, streams=streams)
    assert torch.equal(par, base)
    par_rev = _run(ops, c, dev, streams=streams, order=list(range(n))[::-1])
    assert torch.equal(par_rev, base)
    torch.cuda.synchronize()


# 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_run_source_branch_equals_source_only_call(c, dtype):
    """Same kernel, same keys: the source branch out of the run call == ops.ext_attn(part="source", no_split=True,
    fused=False) on the query frames."""
    ops = _ops()
    dev = _to_dev(_inputs(c, dtype, 11 + c["S"] + c["dh"]), dtype)
    out = _run(ops, c, dev)
    Kq = c["Kq"]
    sub = tuple(_rank_rows(t, c).contiguous() for t in dev)
    src = ops.ext_attn(*sub, c["heads"], c["dh"] ** -0.5, c["inject"], part="source", no_split=True, fused=False,
                       fold_scale=c["fold_scale"], hints=c["hints"], out=torch.zeros_like(out))
    assert torch.equal(out[:Kq], src[:Kq])


# 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("S,h,d", [(576, 2, 64), (1024, 8, 40), (328, 2, 40), (264, 1, 80), (72, 1, 160), (515, 1, 64)])
@pytest.mark.parametrize("inject", [False, True])
def test_one_run_is_the_whole_bank_f32(S, h, d, inject, dtype):
    ops = _ops()
    c = rf.R(S, h, d, inject=inject, K=4, Kq=4, q_frame0=0, runs=[(0, 4)])
    qkv = _inputs(c, dtype, 5 + S)
    refs = attn_ref(*qkv, h, d ** -0.5, inject, need_sigma=False)
    out = _run(ops, c, _to_dev(qkv, dtype), out_dtype=torch.float32)
    assert out.dtype == torch.float32
    assert_attn_close(out, refs, f"whole bank S{S} d{d} inj{inject}", dtype=dtype)


# 5 -------------------------------------------------------------------------------------------------------------------
PARTITIONS = [
    rf.R(256, 2, 40, K=8, Kq=2, q_frame0=3, runs=[(3, 2)] + [(f, 1) for f in (0, 1, 2, 5, 6, 7)]),   # (almost) one frame per run
    rf.R(320, 2, 64, K=8, Kq=1, q_frame0=5, runs=[(5, 1)] + [(f, 1) for f in (0, 1, 2, 3, 4, 6, 7)]),   # n_runs = K = 8
    rf.R(45, 2, 40),                                                                                # fewer than two 64-key tiles
    rf.R(45, 1, 160, inject=True),
    rf.R(576, 2, 64, K=4, Kq=4, q_frame0=0, runs=[(0, 4)]),                                        # Kq = K
    rf.R(256, 5, 64, K=25, Kq=3, q_frame0=4, runs=[(4, 3), (0, 4), (7, 18)]),                      # cfg5's rank geometry, level 2
    rf.R(256, 5, 64, inject=True, K=25, Kq=3, q_frame0=4, runs=[(4, 3), (0, 4), (7, 18)]),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("c", PARTITIONS, ids=_case_id)
def test_partitions(c, dtype):
    ops = _ops()
    qkv = _inputs(c, dtype, 3 + c["S"] + c["K"])
    refs = tuple(None if r is None else _rank_rows(r, c)
                 for r in attn_ref(*qkv, c["heads"], c["dh"] ** -0.5, c["inject"], need_sigma=False))
    dev = _to_dev(qkv, dtype)
    out = _run(ops, c, dev)
    assert_attn_close(out, refs, _case_id(c), dtype=dtype)
    assert torch.equal(_run(ops, c, dev, order=list(range(len(c["runs"])))[::-1]), out)


# 6 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("d", [40, 64])
@pytest.mark.parametrize("inject", [False, True])
def test_peaked_logits_across_runs(d, inject, dtype):
    """Planted keys aligned with their queries (gain 12, the construction of test_ext_attn_d64_score_bound_shift_paths): for
    half of the planted queries the key lies in a REMOTE run, for the others in the local one -- one run's shift dwarfs
    the others' in the merge."""
    ops = _ops()
    c = rf.R(576, 2, d, inject=inject)
    K, S, q0, Kq = c["K"], c["S"], c["q_frame0"], c["Kq"]
    g = torch.Generator().manual_seed(29 + S + d)
    q, k, v = (torch.randn(3 * K, S, 2 * d, generator=g) for _ in range(3))
    remote = [f for f in range(K) if not q0 <= f < q0 + Kq]
    for b in range(3):
        for fq in range(q0, q0 + Kq):
            for i, s_ in enumerate(range(0, S, 5)):
                kf = remote[(i // 2) % len(remote)] if i % 2 == 0 else fq
                k[b * K + kf, (s_ * 3 + S - 60 + 7 * fq) % S] = q[b * K + fq, s_] * 12.0
    q, k, v = (_rnd(dtype)(x) for x in (q, k, v))
    refs = tuple(None if r is None else _rank_rows(r, c) for r in attn_ref(q, k, v, 2, d ** -0.5, inject, need_sigma=False))
    out = _run(ops, c, _to_dev((q, k, v), dtype))
    assert torch.isfinite(out.float()).all()
    assert_attn_close(out, refs, f"peaked d{d} inj{inject}", dtype=dtype)


# 7 -------------------------------------------------------------------------------------------------------------------
def _oracle_rows(q, k, v, K, S, h, d, b, fq, f_bank, head, rows, inject):
    """fp32 oracle for a few query rows of one (branch, query frame, head): tokenflow_utils.py:173-179.  q holds the query
    frames only (index fq), k / v the bank (the query frame is bank frame f_bank)."""
    Kq = q.shape[0] // 3
    qv = q.view(3, Kq, S, h, d)
    kv, vv = k.view(3, K, S, h, d), v.view(3, K, S, h, d)
    bq = 0 if (inject and b > 0) else b
    qr = qv[bq, fq, rows, head].float()
    if b == 0:
        kk, vals = kv[0, f_bank, :, head].float(), vv[0, f_bank, :, head].float()
    else:
        kk, vals = kv[bq, :, :, head].reshape(K * S, d).float(), vv[b, :, :, head].reshape(K * S, d).float()
    p = torch.softmax(qr @ kk.T * d ** -0.5, dim=-1)
    return p @ vals


@pytest.mark.parametrize("inject", [False, True])
def test_fullsize_cfg2_level0_rank1_of_8(inject):
    """BASELINE config 2, level 0, rank 1 of 8: K = 8, its one keyframe, runs local / left / right; fp32 output,
    max per-token deviation < 1e-3 (the north-star number, as tests/test_fullsize_gpu.py asserts it)."""
    ops = _ops()
    K, Kq, q0, S, h, d = 8, 1, 1, 4096, 8, 40
    g = torch.Generator(device="cuda").manual_seed(207)
    q, k, v = (torch.randn(3 * n, S, h * d, generator=g, device="cuda").bfloat16() for n in (Kq, K, K))
    out = ops.ext_attn_runs(q, k, v, h, d ** -0.5, inject, [(1, 1), (0, 1), (2, 6)], q_frame0=q0, out_dtype=torch.float32)
    torch.cuda.synchronize()
    qc, kc, vc, oc = q.cpu(), k.cpu(), v.cpu(), out.cpu().view(3, Kq, S, h, d)
    rows = torch.tensor(sorted({0, 1, 31, 32, 63, 64, 127, 128, S // 2 + 5, S - 129, S - 2, S - 1}))
    worst = 0.0
    for b, head in [(0, 0), (0, h - 1), (1, 3), (1, 0), (2, h - 1), (2, 5)]:
        ref = _oracle_rows(qc, kc, vc, K, S, h, d, b, 0, q0, head, rows, inject)
        worst = max(worst, float((oc[b, 0, rows, head] - ref).abs().max()))
    print(f"cfg2 level 0 rank 1/8 inject {inject}: max per-token deviation {worst:.3e}")
    assert worst < 1e-3, f"inject {inject}: max per-token deviation (fp32 output) {worst:.3e}"


def test_fullsize_cfg5_level0_rank0():
    """BASELINE config 5, level 0, rank 0 of 8: K = 25, the rank's four keyframes 0..3, runs local / right (there is no
    left run); the oracle on 256 query rows per frame picked by a seeded permutation, all heads; fp32 output, < 1e-3."""
    ops = _ops()
    K, Kq, q0, S, h, d = 25, 4, 0, 4096, 5, 64
    g = torch.Generator(device="cuda").manual_seed(505)
    q, k, v = (torch.randn(3 * n, S, h * d, generator=g, device="cuda").bfloat16() for n in (Kq, K, K))
    out = ops.ext_attn_runs(q, k, v, h, d ** -0.5, False, [(0, 4), (4, 21)], q_frame0=q0, out_dtype=torch.float32)
    torch.cuda.synchronize()
    qc, kc, vc, oc = q.cpu(), k.cpu(), v.cpu(), out.cpu().view(3, Kq, S, h, d)
    worst = 0.0
    for fq in range(Kq):
        rows = torch.randperm(S, generator=torch.Generator().manual_seed(1000 + fq))[:256].sort().values
        for b in range(3):
            for head in range(h):
                ref = _oracle_rows(qc, kc, vc, K, S, h, d, b, fq, q0 + fq, head, rows, False)
                worst = max(worst, float((oc[b, fq, rows, head] - ref).abs().max()))
    print(f"cfg5 level 0 rank 0: max per-token deviation {worst:.3e}")
    assert worst < 1e-3, f"max per-token deviation (fp32 output) {worst:.3e}"


# 8 -------------------------------------------------------------------------------------------------------------------
def test_run_argument_errors_launch_nothing():
    """Every TF_ERR_* of tf_ext_attn_run / tf_ext_attn_runs_merge: the code, a tf_last_error text naming the function, and
    no launch (the output and the workspace keep their fill)."""
    from tokenflow_amd import _lib
    lib = _lib.load()
    K, Kq, q0, S, H, Dh, n_runs = 5, 2, 2, 128, 2, 40, 3
    D = H * Dh
    dt = _lib.TF_BF16
    q = torch.randn(3 * Kq, S, D, device="cuda").bfloat16()
    k = torch.randn(3 * K, S, D, device="cuda").bfloat16()
    v = torch.randn(3 * K, S, D, device="cuda").bfloat16()
    out = torch.full((3 * Kq, S, D), 7.0, device="cuda").bfloat16()
    nbytes = lib.tf_ext_attn_runs_workspace_bytes(K, Kq, S, H, Dh, n_runs, dt)
    assert nbytes > 0
    assert lib.tf_ext_attn_runs_workspace_bytes(K, Kq, S, H, Dh, n_runs, _lib.TF_F32) == 0
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    fs = S * D
    strides = (ctypes.c_int64 * 9)(Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, D)
    st = torch.cuda.current_stream().cuda_stream

    def run(qp=None, kp=None, Kq_=Kq, q0_=q0, f0=2, n=2, r=0, nr=n_runs, Dh_=Dh, ld=D, flags=0, dtype=dt, wsp=None,
            wsb=nbytes, sp=strides):
        return lib.tf_ext_attn_run(q.data_ptr() if qp is None else qp, k.data_ptr() if kp is None else kp, v.data_ptr(),
                                   out.data_ptr(), K, Kq_, q0_, f0, n, r, nr, S, H, Dh_, ld, ctypes.cast(sp, ctypes.c_void_p),
                                   1.0, flags, dtype, ws.data_ptr() if wsp is None else wsp, wsb, st)

    def merge(nr=n_runs, Dh_=Dh, o_bs=Kq * fs, o_fs=fs, dtype=dt, wsb=nbytes, op=None, wsp=None):
        return lib.tf_ext_attn_runs_merge(out.data_ptr() if op is None else op, K, Kq, S, H, Dh_, nr, o_bs, o_fs, 0, dtype,
                                          ws.data_ptr() if wsp is None else wsp, wsb, st)

    E = _lib
    bad = [
        (lambda: run(qp=0), -1), (lambda: run(wsp=0), -1), (lambda: run(sp=None), -1),
        (lambda: run(dtype=E.TF_F32), -2),
        (lambda: run(Dh_=48), -3),
        (lambda: run(n=0), -3),                       # empty run
        (lambda: run(f0=4, n=2), -3),                 # run beyond the bank
        (lambda: run(f0=-1, n=2, flags=E.TF_ATTN_BANK_ONLY), -3),
        (lambda: run(r=3), -3), (lambda: run(r=-1), -3),   # run >= n_runs
        (lambda: run(nr=0), -3), (lambda: run(nr=K + 1), -3),
        (lambda: run(f0=0, n=2), -3),                 # source branch wanted, query frames outside the run
        (lambda: run(f0=2, n=1), -3),
        (lambda: run(Kq_=6), -3), (lambda: run(q0_=4), -3),
        (lambda: run(ld=D + 4), -3),
        (lambda: run(flags=E.TF_ATTN_SOURCE_ONLY), -3), (lambda: run(flags=E.TF_ATTN_FUSED), -3),
        (lambda: run(flags=E.attn_hint(qw=2)), -3), (lambda: run(flags=E.TF_ATTN_PRECISE_P), -3),
        (lambda: run(qp=q.data_ptr() + 2), -4), (lambda: run(kp=k.data_ptr() + 8), -4), (lambda: run(wsp=ws.data_ptr() + 4), -4),
        (lambda: run(wsb=nbytes - 1), -5),
        (lambda: merge(op=0), -1), (lambda: merge(dtype=E.TF_F32), -2), (lambda: merge(Dh_=48), -3), (lambda: merge(nr=0), -3),
        (lambda: merge(o_fs=fs + 4), -3), (lambda: merge(op=out.data_ptr() + 2), -4), (lambda: merge(wsb=nbytes - 1), -5),
    ]
    for i, (call, want) in enumerate(bad):
        rc = call()
        msg = lib.tf_last_error().decode()
        assert rc == want, (i, rc, want, msg)
        assert "tf_ext_attn_run" in msg, (i, msg)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0x5A).all()), "an argument error launched something"
    # and the same arguments without the error run
    assert run() == 0 and run(f0=0, n=2, r=1, flags=E.TF_ATTN_BANK_ONLY) == 0
    assert run(f0=4, n=1, r=2, flags=E.TF_ATTN_BANK_ONLY) == 0 and merge() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()) and not bool((out == 7.0).all())
