"""The four-bank shared-softmax form at head dim 64 on the GPU (TF_ATTN_MULTI_V64, plan token one<64,..,MV4,..>): one
workgroup computes QK^T and the online softmax of the source's q and k once and the four P.V products of a PAIR of
injecting edits.

Shapes (K, S, heads): the smallest that still go wrong in every way the kernel can -- several 64-key tiles per frame and
several bank frames (the O rescale crosses tiles and frames), a ragged last tile (S = 77: 13 keys, its second 32-key half
all padding; S = 320), a partly filled workgroup and a partly filled second query tile (256 queries per workgroup), more
than one head.  The oracle runs on the host at these sizes, once per (shape, dtype, input family, edit, injection state).

q, k and v are independent per branch: a launch that read a neighbour's bank, skipped the rescale of banks 2-4, or computed
a non-injecting edit with the source's q and k lands O(1) outside the project's attention bound."""
import functools
import re

import pytest
import torch

from oracle import tokenflow_oracle as orc
from tests import edit_forms as ef
from tests.test_edits_gpu import _edit_attn_inputs, _parts_reference
from tests.test_kernels_gpu import assert_attn_close, attn_bound, attn_ref

pytestmark = pytest.mark.gpu

MV4_64 = re.compile(r"one<64,\d+,\d+,MV4,")
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(3, 192, 2), (2, 77, 2), (2, 320, 5)]     # (K, S, heads)
D_HEAD = 64
KINDS = ["randn", "peaked", "negfirst"]             # "negfirst" plants its first 64 keys: S >= 64 holds for every shape
E_MAX = 3
POISON = 7.0


def _ops():
    from tokenflow_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _inputs(K, S, h, dtype, kind):
    """q, k, v of 1 + 2 * E_MAX branches, fp32 holding values of `dtype`; a batch of E edits is the first 1 + 2E branches."""
    rnd = orc.bf16_round if dtype == torch.bfloat16 else (lambda x: x.half().float())
    B = 1 + 2 * E_MAX
    return tuple(rnd(x) for x in _edit_attn_inputs(B * K, S, h * D_HEAD, h, kind, seed=K * 1000 + S + h + len(kind)))


@functools.lru_cache(maxsize=None)
def _refs(K, S, h, dtype, kind, e, inject):
    """The oracle on [source | uncond_e | cond_e] with edit e's own injection state."""
    q, k, v = _inputs(K, S, h, dtype, kind)
    return attn_ref(*(ef.edit_slice(t, e, E_MAX) for t in (q, k, v)), h, D_HEAD ** -0.5, inject, need_sigma=False)


def _device_inputs(K, S, h, dtype, kind, E):
    n = (1 + 2 * E) * K
    return tuple(t[:n].to(dtype).cuda() for t in _inputs(K, S, h, dtype, kind))


def _assert_plan(ops, K, S, h, E, mask, dtype):
    plan = ops.attn_edits_plan(K, K, S, h, D_HEAD, False, E, dtype=dtype, inject_mask=mask, multi_v64=True)
    n_inj = bin(mask).count("1")
    assert sum(1 for t in plan if MV4_64.match(t)) == n_inj // 2 and plan.count("vt_pack") == 1, plan
    assert sum(1 for t in plan if ",DUAL," in t) == n_inj % 2, plan
    assert not any(t.startswith("merge") for t in plan), plan
    return plan


@pytest.mark.parametrize("K,S,h", SHAPES)
@pytest.mark.parametrize("E,mask", [(2, 0b11), (3, 0b111), (3, 0b101)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_edit_vs_oracle(K, S, h, E, mask, dtype):
    """A pair; a pair plus the odd DUAL edit; a pair of edits that are not neighbours (gap = 4) around an edit that does
    not inject.  Every edit against the oracle under the attention bound, on the three input families; the fp32 output
    rounds to the 16-bit output exactly; everything finite."""
    ops = _ops()
    _assert_plan(ops, K, S, h, E, mask, dtype)
    for kind in KINDS:
        dq, dk, dv = _device_inputs(K, S, h, dtype, kind, E)
        got = ops.ext_attn_edits(dq, dk, dv, h, D_HEAD ** -0.5, False, E, inject_mask=mask, multi_v64=True)
        got32 = ops.ext_attn_edits(dq, dk, dv, h, D_HEAD ** -0.5, False, E, inject_mask=mask, multi_v64=True,
                                   out_dtype=torch.float32)
        assert torch.isfinite(got.float()).all() and torch.isfinite(got32).all(), kind
        assert got32.dtype == torch.float32 and torch.equal(got32.to(dtype), got), kind
        for e in range(E):
            refs = _refs(K, S, h, dtype, kind, e, bool((mask >> e) & 1))
            what = f"four-bank d64 K{K} S{S} h{h} E{E} mask {mask:#b} {kind} {dtype} edit {e}"
            err = assert_attn_close(ef.edit_slice(got, e, E), refs, what, dtype=dtype)
            assert_attn_close(ef.edit_slice(got32, e, E), refs, what + " fp32 out", dtype=dtype)
            print(f"{what}: max abs err {err:.3e} (bound max {float(attn_bound(refs[0], refs[1], dtype).max()):.3e})")


@pytest.mark.parametrize("K,S,h", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_partner_independence_and_determinism(K, S, h, dtype):
    """P and the row sums depend on the source's q and k only: the bank branches of edit 0 are bit-equal whichever edit
    shares its launch (edit 1 as a neighbour, in a batch of two or three; edit 2 across a non-injecting edit).  Two calls
    give the same bits."""
    ops = _ops()
    for kind in ("randn", "peaked"):
        banks = []
        for E, mask in [(2, 0b11), (3, 0b011), (3, 0b101)]:
            _assert_plan(ops, K, S, h, E, mask, dtype)
            dq, dk, dv = _device_inputs(K, S, h, dtype, kind, E)
            got = ops.ext_attn_edits(dq, dk, dv, h, D_HEAD ** -0.5, False, E, inject_mask=mask, multi_v64=True)
            again = ops.ext_attn_edits(dq, dk, dv, h, D_HEAD ** -0.5, False, E, inject_mask=mask, multi_v64=True)
            assert torch.equal(got, again), (kind, E, mask)
            banks.append(got.view(1 + 2 * E, K, S, h * D_HEAD)[1:3].clone())
        assert torch.equal(banks[0], banks[1]), f"{kind}: edit 0 differs between E = 2 and E = 3 (mask 0b011)"
        assert torch.equal(banks[0], banks[2]), f"{kind}: edit 0 differs between partners (mask 0b11 / 0b101)"


@pytest.mark.parametrize("K,S,h", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_flag_off_is_the_composition(K, S, h, dtype):
    """multi_v=False and no flag: bit for bit the bank / source parts, as before."""
    ops = _ops()
    for E in (2, 3):
        dq, dk, dv = _device_inputs(K, S, h, dtype, "randn", E)
        ref = _parts_reference(ops, dq, dk, dv, K, h, D_HEAD, True, E, dtype)
        for kw in (dict(multi_v=False), dict()):
            plan = ops.attn_edits_plan(K, K, S, h, D_HEAD, True, E, dtype=dtype, **kw)
            assert not any(MV4_64.match(t) for t in plan), plan
            assert torch.equal(ops.ext_attn_edits(dq, dk, dv, h, D_HEAD ** -0.5, True, E, **kw), ref), (E, kw)


def _compact(t, mask, E):
    """[source | the (uncond, cond) slots of the edits that do not inject, ascending]"""
    keep = [0] + [b for e in range(E) if not (mask >> e) & 1 for b in (1 + 2 * e, 2 + 2 * e)]
    return t[keep].contiguous()


@pytest.mark.parametrize("K,S,h", SHAPES)
@pytest.mark.parametrize("E,mask", [(2, 0b11), (3, 0b101)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_part_call_bank(K, S, h, E, mask, dtype):
    """`ext_attn_edits_views(part="bank", multi_v64=True)`, dense and compact q / k: the masked call's bank branches bit for
    bit; slab 0 of the output is never written."""
    ops = _ops()
    B, D = 1 + 2 * E, h * D_HEAD
    dq, dk, dv = _device_inputs(K, S, h, dtype, "randn", E)
    want = ops.ext_attn_edits(dq, dk, dv, h, D_HEAD ** -0.5, False, E, inject_mask=mask, multi_v64=True).view(B, K, S, D)
    q4, k4, v4 = (t.view(B, K, S, D) for t in (dq, dk, dv))
    for compact in (False, True):
        plan = ops.attn_edits_part_plan(K, K, S, h, D_HEAD, E, mask, part="bank", qk_compact=compact, dtype=dtype,
                                        multi_v64=True)
        assert sum(1 for t in plan if MV4_64.match(t)) == 1, plan
        qq, kk = (_compact(t, mask, E) if compact else t for t in (q4, k4))
        out = torch.full((B, K, S, D), POISON, dtype=dtype, device="cuda")
        ops.ext_attn_edits_views(qq, kk, v4[1:], out, h, D_HEAD ** -0.5, E, mask, "bank", compact, branch0=(0, 0, 1, 0),
                                 multi_v64=True)
        assert torch.equal(out[1:], want[1:]), f"compact {compact}: bank part"
        assert bool((out[0] == POISON).all()), f"compact {compact}: the bank part wrote the source slab"
