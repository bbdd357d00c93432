"""The memory contract (tests/mem_contract.py) of the ragged chunk runs: `ops.propagate_chunks_ragged` through both entry points
(tf_nn_gather_blend_chunks_ragged, tf_nn_gather_blend_chunks_norm_ragged) with ALL its tensors in the NaN-poisoned arena, on
guarded scratch of exactly the size tf_nn_gather_blend_ragged_workspace_bytes reports, held to the exact reference of
tests/ragged_forms.py and bit-identical under the three scratch fills.  A keyframe slot the run does not read holds NaN."""
import ctypes
import math

import pytest
import torch

from tests import attn_exact as ax
from tests import mem_contract as mc
from tests import nn_exact as nx
from tests import ragged_forms as rf

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
F32 = torch.float32
CASES = [(S, D, form, fr) for S, D, form in rf.SMALL for fr in ([3, 1, 2, 5], [2, 5, 1, 3, 2])]


def _ops():
    from tokenflow_amd import ops
    return ops


def _arena(inputs, outputs):
    sizes = [t.numel() * t.element_size() for t in inputs.values()]
    sizes += [math.prod(s) * torch.empty((), dtype=d).element_size() for s, d, _ in outputs.values()]
    arena = mc.Arena("cuda", mc.Arena.footprint(*sizes))
    t = {name: arena.place(name, x) for name, x in inputs.items()}
    t.update({name: arena.place_out(name, s, d, f) for name, (s, d, f) in outputs.items()})
    return arena, t


@pytest.mark.parametrize("S,D,form,frames", CASES, ids=[f"{c[2]}-S{c[0]}-D{c[1]}-{'_'.join(map(str, c[3]))}" for c in CASES])
@pytest.mark.parametrize("fused_norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_ragged(monkeypatch, S, D, form, frames, fused_norm, dtype):
    from tokenflow_amd import _lib
    ops = _ops()
    lib = _lib.load()
    C, F = len(frames), sum(frames)
    K = C + 1
    arr = (ctypes.c_int * C)(*frames)
    want_bytes = lib.tf_nn_gather_blend_ragged_workspace_bytes(arr, C, S, D)
    rg = rf.Ragged(frames, S, D, "pool" if dtype == torch.bfloat16 else "dense")
    g = torch.Generator().manual_seed(D + F)
    gamma, beta = (1 + 0.2 * torch.randn(D, generator=g)).to(dtype), (0.1 * torch.randn(D, generator=g)).to(dtype)
    for E, (mask, slot0) in [(1, m) for m in rf.masks(C)] + [(2, (1, 0))]:
        nb = 1 + 2 * E
        plan = ops.propagate_ragged_plan(frames, S, D, mask, E)
        assert plan[0].startswith(form + "[") and plan[0].endswith(",ragged]"), plan
        kf = torch.randn(nb * K, S, D, generator=g).to(dtype)
        res = torch.randn(nb * F, S, D, generator=g).to(dtype)
        kf[K + 1] = nx.edge_frame(S, D, dtype, 0, huge=not fused_norm)
        ref = rf.reference(kf, frames, slot0, mask, rg.indices(slot0, mask), res, F32, nb)
        piv = rg.pivots("cpu", dtype, True)
        inputs = {"tgt": rg.targets("cpu", dtype), "piv": piv, "inv_norm": ops.pivot_inv_norm(piv.cuda()).cpu(), "kf_out": kf,
                  "w": rf.weights(frames), "residual": res}
        outputs = {"out": ((nb * F, S, D), F32, ax.SENTINEL)}
        if fused_norm:
            inputs.update(gamma=gamma, beta=beta)
            outputs["norm_out"] = ((nb * F, S, D), dtype, ax.SENTINEL)
        arena, t = _arena(inputs, outputs)
        # keyframe slots the run does not read: NaN in the pivots, their inverse norms and every branch of the cached output
        read = {s for ss in rf.slots_of(C, slot0, mask) for s in ss}
        for s in set(range(K)) - read:
            t["piv"][s] = math.nan
            t["inv_norm"][s] = math.nan
            t["kf_out"].view(nb, K, S, D)[:, s] = math.nan
        kw = {"out": t["out"]}
        if fused_norm:
            kw.update(norm=(t["gamma"], t["beta"], 1e-5, dtype), norm_out=t["norm_out"])
        what = f"{form} S{S} D{D} {frames} {dtype} mask {mask:#b} E={E}"
        by_fill = {}
        for fill in mc.FILLS:
            for name in outputs:
                t[name].fill_(ax.SENTINEL)
            snap = arena.snapshot()
            with monkeypatch.context() as mp:
                scratch, spy = mc.Scratch(mp, ops, fill), mc.Spy(mp, ops)
                got = ops.propagate_chunks_ragged(t["tgt"], t["piv"], t["inv_norm"], t["kf_out"], t["w"], frames, slot0, mask,
                                                  t["residual"], F32, n_edits=E, **kw)
                torch.cuda.synchronize()
                mc.verify(arena, snap, list(outputs), scratch, spy)
                assert scratch.requests == [("nn", want_bytes)], (scratch.requests, want_bytes)
            got = got if fused_norm else (got,)
            assert got[0] is t["out"] and (not fused_norm or got[1] is t["norm_out"]), f"{what}: the caller's buffers were not used"
            assert torch.equal(nx.bits(got[0].cpu()), nx.bits(ref)), f"{what} fill {fill:#04x}"
            if fused_norm:
                mc.assert_finite(f"{what} fill {fill:#04x} (norm)", got[1])
            by_fill[fill] = torch.cat([x.float().flatten() for x in got]).clone()
        mc.assert_same_across_fills(what, by_fill)
        del arena, t
