"""The issue contract (tests/issue_contract.py) of the ragged chunk runs: both entry points of `ops.propagate_chunks_ragged`
under late inputs on a busy side stream (P1), without waiting (P2), captured into a graph and replayed (P3: the chunk
descriptor rides in the kernel arguments, the call copies nothing to the device), and beside itself on two streams (P4), with
a larger run of the same scratch tag behind it."""
import pytest
import torch

from tests import attn_exact as ax
from tests import issue_contract as ic
from tests import ragged_forms as rf

pytestmark = pytest.mark.gpu

F32 = torch.float32
DTYPES = [torch.bfloat16, torch.float16]
CASES = [(45, 320, "rb", [3, 1, 2, 5]), (96, 320, "rbs<TJ=2>", [2, 5, 1, 3, 2]), (45, 1280, "deep", [3, 1, 2, 5])]


def _ops():
    from tokenflow_amd import ops
    return ops


def _randn(shape, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda").to(dtype)


def _full(shape, dtype):
    return lambda: torch.full(tuple(shape), ax.SENTINEL, dtype=dtype, device="cuda")


def _bundle(ops, S, D, frames, dtype, E, mask, slot0, fused_norm, what):
    """Set A: the pool family's targets and pivots; set B: the dense family's, with other cached outputs and another residual."""
    C, F, nb = len(frames), sum(frames), 1 + 2 * E
    K = C + 1
    w = rf.weights(frames).cuda()
    sets = []
    for i, family in enumerate(("pool", "dense")):
        rg = rf.Ragged(frames, S, D, family, seed=S + D + i)
        piv = rg.pivots("cuda", dtype, True)
        sets.append([rg.targets("cuda", dtype), piv, ops.pivot_inv_norm(piv), _randn((nb * K, S, D), dtype, 10 + i),
                     _randn((nb * F, S, D), dtype, 20 + i)])
    norm = None
    if fused_norm:
        norm = (1 + 0.2 * _randn((D,), dtype, 3), 0.1 * _randn((D,), dtype, 4), 1e-5, dtype)

    def call(t, out):
        kw = {"out": out} if norm is None else {"out": out[0], "norm": norm, "norm_out": out[1]}
        ops.propagate_chunks_ragged(t[0], t[1], t[2], t[3], w, frames, slot0, mask, t[4], F32, n_edits=E, **kw)

    shape = (nb * F, S, D)
    make_out = _full(shape, F32) if norm is None else (lambda: (_full(shape, F32)(), _full(shape, dtype)()))
    return ic.Bundle(call, sets[0], sets[1], make_out, what)


def _ws_bytes(ops, bundle):
    inner, seen = ops._workspace, []

    def spy(nbytes, device, tag="attn", stream=None):
        seen.append(int(nbytes))
        return inner(nbytes, device, tag, stream)
    ops._workspace = spy
    try:
        bundle.eager(bundle.A)
    finally:
        ops._workspace = inner
    assert seen
    return max(max(seen), 1 << 20)


@pytest.mark.parametrize("S,D,form,frames", CASES, ids=[f"{c[2]}-S{c[0]}-D{c[1]}" for c in CASES])
@pytest.mark.parametrize("fused_norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_ragged_entry_points(S, D, form, frames, fused_norm, dtype):
    ops = _ops()
    C = len(frames)
    mask, slot0 = rf.masks(C)[1]
    E = 2 if (fused_norm and dtype == torch.float16) else 1       # the multi-edit gather rides along on one combination
    if E > 1:
        mask, slot0 = 1, 0
    plan = ops.propagate_ragged_plan(frames, S, D, mask, E)
    assert plan[0].startswith(form + "[") and plan[0].endswith(",ragged]") and plan[1].endswith(",ragged]"), plan
    what = f"propagate_chunks_ragged {form} {frames} E={E} {'norm ' if fused_norm else ''}{dtype}"
    b = _bundle(ops, S, D, frames, dtype, E, mask, slot0, fused_norm, what)
    longer = frames + [4, 1, 3]
    larger = _bundle(ops, S, D, longer, dtype, E, mask, slot0, fused_norm, what + " (longer run)")
    assert ops.propagate_ragged_plan(longer, S, D, mask, E)[0].endswith(",ragged]")
    ic.check(b, None, None, None, None, drop=ops.drop_workspaces, cache=lambda: ops._ws_cache, ws_bytes=_ws_bytes(ops, b),
             larger=larger)
