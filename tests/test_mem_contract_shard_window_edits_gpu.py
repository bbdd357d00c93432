"""The memory contract (tests/mem_contract.py) of the calls of a windowed / anchored multi-edit shard pass: `ops.edit_halo_pack`,
both bank-part entry points and the native executor on the loopback transport -- each in the NaN-poisoned arena, on guarded
scratch of exactly the size its size function reports, bit-identical under the three scratch fills.

The loopback transport "receives" the rank's own send rows (a copy of min(send, recv) bytes), so the executor runs at a geometry
whose send rows cover the receive buffer: rank 0 of 2 over K = 5, radius 1 (4 rows out, 4 in; with anchor 0: 5 out, 4 in)."""
import ctypes
import math

import pytest
import torch

from tests import attn_exact as ax
from tests import mem_contract as mc

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


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


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ns,nq", [(7, 3), (32, 0)])
def test_contract_edit_halo_pack(monkeypatch, dtype, ns, nq):
    """Strided slab views (frame stride != S * ld, ld > D) and strided q slabs: torch indexing, bit for bit; nothing else moves."""
    ops = _ops()
    Kl, S, D = 3, 3, 8
    g = torch.Generator().manual_seed(3 + ns)
    buf = torch.randn(ns, Kl + 1, S + 2, 3 * D, generator=g).to(dtype)
    qbuf = torch.randn(3, Kl, S + 1, 2 * D, generator=g).to(dtype)
    for masks in ([0b000, 0b111, 0b101], [0b010, 0b010, 0b011, 0b110], [0b100]):
        frames = [f for m in masks for f in ax.members(m)]
        outs = {"out": ((len(frames), ns, S, D), dtype, ax.SENTINEL)}
        if nq:
            outs["q_out"] = ((nq, Kl, S, D), dtype, ax.SENTINEL)
        arena, t = _arena({"buf": buf, "qbuf": qbuf}, outs)
        slabs = [t["buf"][i, :Kl, 1:1 + S, D * (i % 3):D * (i % 3) + D] for i in range(ns)]
        qs = [t["qbuf"][i, :, :S, D:] for i in range(nq)]
        snap = arena.snapshot()
        with monkeypatch.context() as mp:
            scratch, spy = mc.Scratch(mp, ops, mc.POISON), mc.Spy(mp, ops)
            got, stage = ops.edit_halo_pack(slabs, masks, qs, out=t["out"], q_out=t.get("q_out"))
            torch.cuda.synchronize()
            mc.verify(arena, snap, list(outs), scratch, spy)
            assert scratch.requests == []      # pure data movement: no scratch
        assert got is t["out"] and torch.equal(got, torch.stack([torch.stack([s[f] for s in slabs]) for f in frames])), masks
        assert (stage is None) if nq == 0 else torch.equal(stage, torch.stack(qs)), masks


@pytest.mark.parametrize("kind", ["win", "set"])
@pytest.mark.parametrize("S,H,Dh", [(64, 2, 40), (320, 2, 64)], ids=["fused", "streaming"])
def test_contract_part_entry_points(monkeypatch, kind, S, H, Dh):
    """The bank part of E = 2 edits with a mixed mask, compact q / k, the rank's 3 query frames of a 7-frame bank: the source
    slab of `out` and every input stay as they were, the scratch request is exactly tf_ext_attn_edits_workspace_bytes, the
    result is finite and does not depend on what the scratch held."""
    from tokenflow_amd import _lib
    ops = _ops()
    dtype, K, Kq, f0, E, mask = torch.bfloat16, 7, 3, 2, 2, 0b01
    B, D = 1 + 2 * E, H * Dh
    g = torch.Generator().manual_seed(S + Dh)
    qc = torch.randn(3, Kq, S, D, generator=g).to(dtype)      # compact: [source | uncond_2 | cond_2]
    kc = torch.randn(3, K, S, D, generator=g).to(dtype)
    v = torch.randn(2 * E, K, S, D, generator=g).to(dtype)    # the source's v is absent
    tab = (ops.bank_windows(K, 1) if kind == "win" else ops.bank_frame_sets(K, 1, (0, 6)))[f0:f0 + Kq]
    view = ops.ext_attn_windows_edits_views if kind == "win" else ops.ext_attn_frame_sets_edits_views
    arena, t = _arena({"q": qc, "k": kc, "v": v}, {"out": ((B, Kq, S, D), dtype, ax.SENTINEL)})
    want_bytes = _lib.load().tf_ext_attn_edits_workspace_bytes(K, S, H, Dh, E, ops._DT[dtype])
    by_fill = {}
    for fill in mc.FILLS:
        t["out"].fill_(ax.SENTINEL)
        snap = arena.snapshot()
        with monkeypatch.context() as mp:
            scratch, spy = mc.Scratch(mp, ops, fill), mc.Spy(mp, ops)
            view(t["q"], t["k"], t["v"], t["out"], H, Dh ** -0.5, E, mask, tab, "bank", True, branch0=(0, 0, 1, 0), q_frame0=f0,
                 no_split=True, multi_v=False)
            torch.cuda.synchronize()
            mc.verify(arena, snap, ["out"], scratch, spy)
            assert [nb for _, nb in scratch.requests] == [want_bytes], (scratch.requests, want_bytes)
        o = t["out"].cpu()
        assert bool((o[0] == ax.SENTINEL).all()), "the bank part wrote the source slab"
        mc.assert_finite(f"{kind} S{S} fill {fill:#04x}", o[1:])
        by_fill[fill] = o.clone()
    mc.assert_same_across_fills(f"{kind} S{S}", by_fill)


def _guarded(nbytes, fill, device):
    payload = max(16, (nbytes + 15) // 16 * 16)
    buf = mc._aligned_bytes(mc.GUARD + payload + max(mc.SCRATCH_REAR_MIN, nbytes), device)
    buf.fill_(mc.POISON)
    ws = buf[mc.GUARD:mc.GUARD + payload]
    ws.fill_(fill)
    return buf, ws, payload


@pytest.mark.parametrize("anchors", [(), (0,)], ids=["windows", "anchors"])
@pytest.mark.parametrize("S,H,Dh", [(64, 2, 40), (320, 2, 64)], ids=["fused", "streaming"])
def test_contract_executor_on_the_loopback_transport(anchors, S, H, Dh):
    """ONE tf_rank_pivotal_frame_sets_edits call of rank 0 of 2 (K = 5, radius 1, E = 2, a mixed mask, TF_RANK_INV_NORM) on a
    workspace of exactly the reported size between guard bands: q, k, v and the pivots stay as they were, only the local slots
    of the attention output and of the inverse norms are written, the guards stay POISON, the result is finite and the same
    under the three fills."""
    from tokenflow_amd import _lib, sharded
    from tokenflow_amd.comm import HipComm
    ops = _ops()
    lib = _lib.load()
    dtype, K, R, E, mask = torch.bfloat16, 5, 1, 2, 0b01
    B, D = 1 + 2 * E, H * Dh
    sh = sharded.NativeEditShard(K, HipComm.loopback(0, 2), HipComm.loopback(0, 2), window_edits=True)
    Kl = sh.Kl
    pl = sharded.frame_set_halo_plan(K, 2, 0, R, anchors)
    assert sum(pl.send_rows) >= pl.F      # the loopback copy fills the whole receive buffer
    g = torch.Generator().manual_seed(S + Dh + len(anchors))
    q, k, v = (torch.randn(B * Kl, S, D, generator=g).to(dtype) for _ in range(3))
    piv = torch.randn(Kl + 1, S, D, generator=g).to(dtype)
    arena, t = _arena({"q": q, "k": k, "v": v, "piv": piv},
                      {"inv": ((Kl + 1, S), torch.float32, ax.SENTINEL), "kfo": ((B, Kl + 1, S, D), dtype, ax.SENTINEL)})
    anc = (ctypes.c_int * max(len(anchors), 1))(*anchors)
    dt = ops._DT[dtype]
    nbytes = lib.tf_rank_pivotal_frame_sets_edits_workspace_bytes(sh._rk, S, H, Dh, dt, R, ctypes.cast(anc, ctypes.c_void_p),
                                                                  len(anchors), E)
    assert nbytes >= lib.tf_rank_pivotal_frame_sets_workspace_bytes(sh._rk, S, H, Dh, dt, R, ctypes.cast(anc, ctypes.c_void_p),
                                                                    len(anchors))
    assert nbytes >= lib.tf_rank_pivotal_edits_workspace_bytes(sh._rk, S, H, Dh, E, dt) > 0
    by_fill = {}
    for fill in mc.FILLS:
        t["kfo"].fill_(ax.SENTINEL)
        t["inv"].fill_(ax.SENTINEL)
        buf, ws, payload = _guarded(nbytes, fill, t["q"].device)
        sh._news[(S, H, Dh, dt, t["q"].device, E, "window", R, tuple(anchors))] = ws      # the executor's scratch: exact, guarded
        snap = arena.snapshot()
        _pe, ie, ke, reqs = sh.pivotal_block(t["q"], t["k"], t["v"], H, Dh ** -0.5, False, (t["piv"], t["inv"], t["kfo"]),
                                             inv_norm=True, n_edits=E, inject_mask=mask, window=R, anchors=anchors or None)
        sh.halo_wait(reqs)
        torch.cuda.synchronize()
        mc.verify(arena, snap, ["kfo", "inv"])
        assert bool((buf[:mc.GUARD] == mc.POISON).all()) and bool((buf[mc.GUARD + payload:] == mc.POISON).all()), \
            f"fill {fill:#04x}: the executor wrote outside its {nbytes}-byte workspace"
        kfo, inv = t["kfo"].cpu(), t["inv"].cpu()
        assert bool((kfo[:, 0] == ax.SENTINEL).all()) and bool((inv[0] == ax.SENTINEL).all()), "rank 0 has no left neighbour"
        mc.assert_finite(f"executor fill {fill:#04x}", kfo[:, 1:])
        assert torch.equal(inv[1:], (1.0 / t["piv"][1:].float().norm(dim=-1)).cpu()) or torch.allclose(
            inv[1:], (1.0 / t["piv"][1:].float().norm(dim=-1)).cpu(), rtol=1e-5)
        by_fill[fill] = kfo.clone()
    mc.assert_same_across_fills(f"executor anchors={anchors} S{S}", by_fill)
    # the source slices are what the single-process source part computes on the rank's own frames (they need no exchange)
    want = torch.full((B, Kl, S, D), ax.SENTINEL, dtype=dtype, device="cuda")
    q4, k4, v4 = (t[n].view(B, Kl, S, D) for n in ("q", "k", "v"))
    ops.ext_attn_edits_views(q4[0:1], k4[0:1], v4[0:1], want[0:1], H, Dh ** -0.5, E, mask, "source", no_split=True)
    assert torch.equal(by_fill[mc.FILLS[0]][0, 1:], want[0].cpu())
    sh.close()
