"""The four-bank run form of the multi-edit attention on an MI355X (ops.ext_attn_runs_edits(..., multi_v=True):
TF_ATTN_RUN_MULTI_V -- each pair of injecting edits is ONE MODE_MV4 launch per run that leaves both edits' partial results).

Geometry: H = 2 heads, a bank of K = 6 frames, the queries of frames 2 and 3, runs (1,4), (0,1), (5,1): the local run holds
the query frames and, with 4 frames of 256 tokens, splits itself into more than one slot by the library's own rule
(`test_the_local_run_fills_more_than_one_slot`); frames of 256 tokens and a ragged 288; head dims 40 (the packed image) and 64
(four unpacked banks).  (E, mask) covers a neighbouring pair, a pair plus an odd injecting edit, a pair around a
non-injecting edit (branch distance 4), a pair beside both, and a mask with nothing to pair.

q, k, v are independent per branch, so a launch that reads or writes a neighbouring edit's bank, or the wrong partial region,
lands O(1) outside the bound.  A HIP result is compared with the fp32 oracle under the attention bound of
tests/test_kernels_gpu.py (2e-4 + eps |ref| + eps softmax.|V|, eps = 2^-8 bf16 / 2^-11 f16; per edit, on [source | uncond_e |
cond_e] with that edit's flag), or bit for bit with another HIP result.  No tolerance between two HIP results appears here.
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
from tests.test_kernels_gpu import assert_attn_close, attn_ref  # noqa: E402

pytestmark = pytest.mark.gpu

H, K, KQ, Q0 = 2, 6, 2, 2
RUNS = [(1, 4), (0, 1), (5, 1)]
CONFIGS = [(2, 0b11), (3, 0b111), (3, 0b101), (4, 0b0111), (3, 0b010)]
SIZES = [256, 288]
KINDS = ["randn", "peaked3", "peaked12", "negfirst"]
BF16, F16 = torch.bfloat16, torch.float16


def _ops():
    from tokenflow_amd import ops
    return ops


def _rnd(dtype):
    return orc.bf16_round if dtype == BF16 else (lambda x: x.half().float())


def _pairs(E, mask):
    inj = [e for e in range(E) if (mask >> e) & 1]
    return [(inj[i], inj[i + 1]) for i in range(0, len(inj) - 1, 2)]


def _paired(E, mask):
    return {e for p in _pairs(E, mask) for e in p}


@functools.lru_cache(maxsize=None)
def _inputs(S, dh, E, kind, dtype):
    """fp32 (rounded to dtype) q, k, v [B*K, S, D] on the CPU, every branch its own draw.  The families of
    tests/test_edits_gpu.py: N(0,1); peaked -- planted keys aligned with their queries (gain 3 / 12), for half of the planted
    queries in a REMOTE run, for the others in their own frame (the local run), as tests/test_attn_runs_edits_gpu.py plants
    them; a strongly negative first 64-key tile in every frame (every one of its scores ~ -110)."""
    B, D = 1 + 2 * E, H * dh
    g = torch.Generator().manual_seed(41 + S + dh + E + len(kind))
    q, k, v = (torch.randn(B * K, S, D, generator=g) for _ in range(3))
    if kind.startswith("peaked"):
        gain = float(kind[len("peaked"):])
        remote = [f for f in range(K) if not Q0 <= f < Q0 + KQ]
        for b in range(B):
            for fq in range(Q0, Q0 + KQ):
                for j, s_ in enumerate(range(0, S, 5)):
                    kf = remote[(j // 2) % len(remote)] if j % 2 == 0 else fq
                    k[b * K + kf, (s_ * 3 + S - 60 + 7 * fq) % S] = q[b * K + fq, s_] * gain
    elif kind == "negfirst":
        u = torch.nn.functional.normalize(torch.randn(H, dh, generator=g), dim=-1)
        amp = (110.0 * dh ** 0.5) ** 0.5
        q = (amp * u.view(1, 1, H, dh) + 0.05 * q.view(B * K, S, H, dh)).reshape(B * K, S, D)
        kv = k.view(B * K, S, H, dh)
        kv[:, :64] = -amp * u.view(1, 1, H, dh) + 0.05 * kv[:, :64]
    return tuple(_rnd(dtype)(x) for x in (q, k, v))


@functools.lru_cache(maxsize=None)
def _dev(S, dh, E, kind, dtype):
    return tuple(t.to(dtype).cuda() for t in _inputs(S, dh, E, kind, dtype))


def _rows(t, nbr):
    """Rows of a [nbr*K, S, D] tensor that belong to the query frames: [nbr*Kq, S, D]."""
    return t.view(nbr, K, *t.shape[1:])[:, Q0:Q0 + KQ].reshape(nbr * KQ, *t.shape[1:])


def _edit3(t, e, n):
    """[source | uncond_e | cond_e] of a [B*n, S, D] tensor: [3n, S, D]."""
    return torch.cat([t[:n], t[(1 + 2 * e) * n:(3 + 2 * e) * n]])


def _call(S, dh, E, mask, kind, dtype, multi_v, v=None, **kw):
    dq, dk, dv = _dev(S, dh, E, kind, dtype)
    return _ops().ext_attn_runs_edits(_rows(dq, 1 + 2 * E).contiguous(), dk, dv if v is None else v, H, dh ** -0.5, E, mask,
                                      RUNS, q_frame0=Q0, multi_v=multi_v, **kw)


@functools.lru_cache(maxsize=None)
def _base(S, dh, E, mask, kind, dtype, multi_v):
    """The in-order, one-stream result (shared by the tests that compare against it; never written to)."""
    return _call(S, dh, E, mask, kind, dtype, multi_v)


@functools.lru_cache(maxsize=None)
def _refs(S, dh, E, e, inject, kind, dtype):
    q, k, v = _inputs(S, dh, E, kind, dtype)
    r = attn_ref(_edit3(q, e, K), _edit3(k, e, K), _edit3(v, e, K), H, dh ** -0.5, inject, need_sigma=False)
    return tuple(None if x is None else _rows(x, 3) for x in r)


def _assert_oracle(out, S, dh, E, mask, kind, dtype, what):
    assert torch.isfinite(out.float()).all(), what
    for e in range(E):
        refs = _refs(S, dh, E, e, bool((mask >> e) & 1), kind, dtype)
        err = assert_attn_close(_edit3(out, e, KQ), refs, f"{what} edit {e}", dtype=dtype)
        print(f"{what} edit {e}: max abs err {err:.3e}")


def _id(S, dh, E, mask):
    return f"S{S}-d{dh}-E{E}-m{mask:b}"


GRID = [(S, dh, E, m) for dh in (40, 64) for S in SIZES for E, m in CONFIGS]
GRID_IDS = [_id(*g) for g in GRID]
SMALL = [(256, dh, E, m) for dh in (40, 64) for E, m in CONFIGS] + [(288, 40, 3, 0b101), (288, 64, 4, 0b0111)]
SMALL_IDS = [_id(*g) for g in SMALL]


def test_the_plans_hold_the_four_bank_run_tokens():
    ops = _ops()
    tok = {40: "one<40,1,4,MV4,2,fq0,run>", 64: "one<64,1,8,MV4,2,fq1,run>"}
    for S, dh, E, m in GRID:
        for r, (f0, n) in enumerate(RUNS):
            plan = ops.attn_run_edits_plan(K, KQ, n, len(RUNS), S, H, dh, E, m, bank_only=r != 0, multi_v=True)
            assert plan.count(tok[dh]) == len(_pairs(E, m)), (S, dh, E, m, plan)


@pytest.mark.parametrize("dh", [40, 64])
@pytest.mark.parametrize("S", SIZES)
def test_the_local_run_fills_more_than_one_slot(S, dh):
    """A pair launch splits into the slots of its run's injecting state: the split a bank-only call under injection over the
    run's 4 frames takes by the library's rule (its plan names it), no environment override.  And the one-pass form
    (no_split=True) of the same run set re-associates the sums: the paired edits' bits differ from the split form's."""
    ops = _ops()
    plan = ops.attn_plan(RUNS[0][1], KQ, S, H, dh, True, part="bank", fused=False, no_split=False)
    nseg = [int(t[len("merge[nseg="):-1]) for t in plan if t.startswith("merge[nseg=")]
    assert nseg and nseg[0] > 1, plan
    a = _base(S, dh, 2, 0b11, "randn", BF16, True)
    b = _call(S, dh, 2, 0b11, "randn", BF16, True, no_split=True)
    assert not torch.equal(a[KQ:], b[KQ:])
    assert torch.equal(a[:KQ], b[:KQ])          # (the source branch never splits)


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,dh,E,mask", GRID, ids=GRID_IDS)
def test_every_edit_and_the_source_vs_oracle(S, dh, E, mask):
    for kind in KINDS:
        out = _base(S, dh, E, mask, kind, BF16, True)
        _assert_oracle(out, S, dh, E, mask, kind, BF16, f"{_id(S, dh, E, mask)} {kind} bf16")


@pytest.mark.parametrize("dh", [40, 64])
def test_f16_vs_oracle(dh):
    for S, E, mask in ((256, 3, 0b111), (288, 3, 0b101)):
        for kind in KINDS:
            out = _base(S, dh, E, mask, kind, F16, True)
            _assert_oracle(out, S, dh, E, mask, kind, F16, f"{_id(S, dh, E, mask)} {kind} f16")


def test_f32_output():
    S, dh, E, mask = 256, 64, 3, 0b111
    for d, S_ in ((dh, S), (40, 288)):
        out = _call(S_, d, E, mask, "randn", BF16, True, out_dtype=torch.float32)
        assert out.dtype == torch.float32
        _assert_oracle(out, S_, d, E, mask, "randn", BF16, f"f32 {_id(S_, d, E, mask)}")
        # the 16-bit output is the one rounding of this accumulator
        assert torch.equal(out.to(BF16), _base(S_, d, E, mask, "randn", BF16, True))


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,dh,E,mask", GRID, ids=GRID_IDS)
def test_unpaired_edits_and_the_source_keep_their_bits(S, dh, E, mask):
    """The non-injecting edits, the odd injecting edit and the source branch are those of the call without the flag, and a mask
    with nothing to pair changes nothing at all.  (Nothing is asserted of the paired edits here: where the flag-less launch is
    the packed DUAL form of the same kernel -- head dim 40 on ragged frames -- the four-bank launch sums in the same order and
    gives the same bits; against the interleaved DUAL kernels it does not.)"""
    on, off = _base(S, dh, E, mask, "randn", BF16, True), _base(S, dh, E, mask, "randn", BF16, False)
    nbr = 1 + 2 * E
    on4, off4 = on.view(nbr, KQ, *on.shape[1:]), off.view(nbr, KQ, *off.shape[1:])
    assert torch.equal(on4[0], off4[0]), "source branch"
    paired = _paired(E, mask)
    for e in range(E):
        if e not in paired:
            assert torch.equal(on4[1 + 2 * e:3 + 2 * e], off4[1 + 2 * e:3 + 2 * e]), f"edit {e} (not in a pair) changed with the flag"
    if not paired:
        assert torch.equal(on, off)


# 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,dh,E,mask", [g for g in SMALL if _pairs(g[2], g[3])],
                         ids=[i for g, i in zip(SMALL, SMALL_IDS) if _pairs(g[2], g[3])])
def test_a_pairs_edits_do_not_see_each_others_values(S, dh, E, mask):
    """Replacing one edit's v (both branches, every frame) leaves every other edit -- its pair partner first of all -- and
    the source branch bit for bit, and changes that edit."""
    base = _base(S, dh, E, mask, "randn", BF16, True)
    nbr = 1 + 2 * E
    dv = _dev(S, dh, E, "randn", BF16)[2]
    g = torch.Generator().manual_seed(5)
    for e0, e1 in _pairs(E, mask):
        for e in (e0, e1):
            v2 = dv.clone()
            sl = slice((1 + 2 * e) * K, (3 + 2 * e) * K)
            v2[sl] = torch.randn(2 * K, S, H * dh, generator=g).to(BF16).cuda()
            got = _call(S, dh, E, mask, "randn", BF16, True, v=v2).view(nbr, KQ, S, H * dh)
            want = base.view(nbr, KQ, S, H * dh)
            for b in range(nbr):
                if b in (1 + 2 * e, 2 + 2 * e):
                    assert not torch.equal(got[b], want[b]), (e, b)
                else:
                    assert torch.equal(got[b], want[b]), f"branch {b} changed with the values of edit {e}"


# 4, 5 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,dh,E,mask", SMALL, ids=SMALL_IDS)
def test_order_streams_and_compact_k_do_not_change_a_bit(S, dh, E, mask):
    base = _base(S, dh, E, mask, "randn", BF16, True)
    n = len(RUNS)
    rev = list(range(n))[::-1]
    assert torch.equal(_call(S, dh, E, mask, "randn", BF16, True, order=rev), base)
    streams = [torch.cuda.Stream() for _ in range(n)]
    assert torch.equal(_call(S, dh, E, mask, "randn", BF16, True, streams=streams), base)
    assert torch.equal(_call(S, dh, E, mask, "randn", BF16, True, streams=streams, order=rev), base)
    # the remote runs read a compact k (the source slot, then the non-injecting edits' slots) against the dense q
    assert torch.equal(_call(S, dh, E, mask, "randn", BF16, True, k_compact=True), base)
    assert torch.equal(_call(S, dh, E, mask, "randn", BF16, True, k_compact=True, streams=streams, order=rev), base)
    torch.cuda.synchronize()


# 6 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,dh,E,mask", SMALL, ids=SMALL_IDS)
def test_one_pass_runs_vs_oracle(S, dh, E, mask):
    for kind in KINDS:
        out = _call(S, dh, E, mask, kind, BF16, True, no_split=True)
        _assert_oracle(out, S, dh, E, mask, kind, BF16, f"no_split {_id(S, dh, E, mask)} {kind}")
    # the flag-less one-pass call: the unpaired edits and the source keep their bits here too
    on = _call(S, dh, E, mask, "randn", BF16, True, no_split=True).view(1 + 2 * E, KQ, S, H * dh)
    off = _call(S, dh, E, mask, "randn", BF16, False, no_split=True).view(1 + 2 * E, KQ, S, H * dh)
    keep = [0] + [b for e in range(E) if e not in _paired(E, mask) for b in (1 + 2 * e, 2 + 2 * e)]
    assert torch.equal(on[keep], off[keep])


def test_the_flag_selects_nothing_outside_its_form():
    """Head dim 80, the folded scale, TF_ATTN_NO_MULTI_V, one edit: the same bits as without the flag."""
    from tokenflow_amd import _lib
    ops = _ops()
    S, E, mask = 256, 2, 0b11
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(5 * K, S, H * 80, generator=g).to(BF16).cuda() for _ in range(3))
    args = (_rows(q, 5).contiguous(), k, v, H, 80 ** -0.5, E, mask, RUNS)
    assert torch.equal(ops.ext_attn_runs_edits(*args, q_frame0=Q0, multi_v=True), ops.ext_attn_runs_edits(*args, q_frame0=Q0))
    off = _base(S, 40, E, mask, "randn", BF16, False)
    assert torch.equal(_call(S, 40, E, mask, "randn", BF16, True, hints=_lib.TF_ATTN_NO_MULTI_V), off)
    assert torch.equal(_call(S, 40, E, mask, "randn", BF16, True, fold_scale=True),
                       _call(S, 40, E, mask, "randn", BF16, False, fold_scale=True))
    dq, dk, dv = (t[:3 * K] for t in _dev(S, 64, E, "randn", BF16))
    one = (_rows(dq, 3).contiguous(), dk, dv, H, 64 ** -0.5, 1, 1, RUNS)
    assert torch.equal(ops.ext_attn_runs_edits(*one, q_frame0=Q0, multi_v=True),
                       ops.ext_attn_runs_edits(*one, q_frame0=Q0))
