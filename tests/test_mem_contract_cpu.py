"""tests/mem_contract.py proven on mutants, on the CPU: a fake op computes census attention in torch on arena views with a fake
scratch, through a fake `ops` (its `_workspace` and `_launch` are what `Scratch` and `Spy` replace).  `mc.check_census_call` -- the
very function tests/test_mem_contract_gpu.py runs per call: Scratch + Spy, the call, `mc.verify`, sentinel, finiteness, the
project's census tolerance, the fill comparison -- passes the honest op and fails, with the tensor's name and the byte offset,
on every mutant:

  (a) one element written past `out`        (b) one element written before `out`
  (c) a write into a gap column of k        (d) q modified in place
  (e) a write one byte, and nbytes - 1 bytes, past the scratch payload
  (f) an output that reads a scratch word the call did not write (fill comparison; under the NaN fill also finiteness)
  (g) a masked key row past the end of v multiplied by zero (0 x NaN)
  (h) a wrapper that copied q (the pointer lies outside the arena)
"""
import types

import pytest
import torch

from tests import attn_exact as ax
from tests import mem_contract as mc

SPEC = ax.Spec(3, 2, 5, 2, 8, inject=True, owned=[1, 2])
SPAD = 8                      # the fake scratch holds V as fp32 [nbr*K, SPAD, D]; rows S .. SPAD-1 are never written
DTYPES = [torch.bfloat16, torch.float16]


def fake_ops():
    ops = types.SimpleNamespace()
    ops._workspace = lambda nbytes, device, tag="attn", stream=None: torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8)
    ops._launch = lambda dev, what, fn, *args, stream=None: fn(*args, 0)
    return ops


def _past(t, n):
    """n elements starting right behind the last element of the dense tensor t (same storage)."""
    return torch.as_strided(t, (n,), (1,), t.storage_offset() + t.numel())


def fake_ext_attn(ops, q, k, v, out, spec, mutant=None):
    """Census attention (fp64 softmax over the key lists) the way a wrapper and its kernel split the work: the wrapper asks
    for scratch and launches; the "kernel" packs V as fp32 into the scratch and computes from there."""
    nbr, K, Kq, S, H, d, D = spec.nbr, spec.K, spec.Kq, spec.S, spec.H, spec.d, spec.D
    if mutant == "h":
        q = q.clone()
    nbytes = nbr * K * SPAD * D * 4
    ws = ops._workspace(nbytes, q.device)

    def kernel(qp, kp, vp, op, wsp, ws_bytes, stream):
        assert ws_bytes >= nbytes
        vt = ws[:nbytes].view(torch.float32).view(nbr * K, SPAD, D)
        for b in spec.owned:
            vt[b * K:(b + 1) * K, :S] = v[b * K:(b + 1) * K].float()
        for b in spec.owned:
            qb = spec.qk_branch(b)
            for qi in range(Kq):
                fr = spec.key_frames(b, qi)
                kmat = torch.cat([k[qb * K + f] for f in fr]).double().view(-1, H, d)
                rows = SPAD if mutant == "g" else S
                if mutant == "g":      # the key rows of every frame padded to SPAD, the pad rows masked: P = 0 times whatever lies there
                    vrows = [torch.as_strided(v, (SPAD, D), (v.stride(1), 1), v[b * K + f].storage_offset()).double() for f in fr]
                    vmat = torch.cat(vrows).view(-1, H, d)
                    kmat = torch.cat([torch.cat([k[qb * K + f].double(), torch.zeros(SPAD - S, D, dtype=torch.float64)]) for f in fr]).view(-1, H, d)
                else:
                    vmat = torch.cat([vt[b * K + f, :S] for f in fr]).double().view(-1, H, d)
                s = torch.einsum("qhc,khc->hqk", q[qb * Kq + qi].double().view(S, H, d), kmat) * spec.scale
                if mutant == "g":
                    s[:, :, (torch.arange(s.shape[-1]) % rows) >= S] = -float("inf")
                o = torch.einsum("hqk,khc->qhc", torch.softmax(s, -1), vmat).reshape(S, D)
                if mutant == "f" and qi == 0:
                    o[0, 0] += float(vt[b * K, SPAD - 1, 0])      # a pad word of the scratch
                if mutant == "fs" and qi == 0:                      # the same, scaled to one fp32 ulp of the branch channel
                    o[0, 1] += float(vt[b * K, SPAD - 1, 0]) * 2.0 ** -150
                out[b * Kq + qi] = o.to(out.dtype)
        one = torch.tensor(3.0, dtype=out.dtype)
        if mutant == "a":
            _past(out, 1)[0] = one
        elif mutant == "b":
            torch.as_strided(out, (1,), (1,), out.storage_offset() - 1)[0] = one
        elif mutant == "c":
            torch.as_strided(k, (1,), (1,), k[1, 2].storage_offset() + D)[0] = one      # frame 1 row 2, the first column behind the values
        elif mutant == "d":
            q[1, 2, 3] = one
        elif mutant == "e1":
            _past(ws, 1)[0] = 0
        elif mutant == "e2":
            _past(ws, nbytes)[nbytes - 1] = 0
    ops._launch(q.device, "fake_ext_attn", kernel, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def _setup(dtype, out_dtype=None):
    spec = SPEC
    v, ones = ax.census_v(spec)
    c, n = ax.census_expected(spec, v)
    q, k = ax.census_qk(spec, "flat", 3)
    out_dtype = dtype if out_dtype is None else out_dtype
    D, ld = spec.D, spec.D + 16
    es = 2
    arena = mc.Arena("cpu", mc.Arena.footprint(*[t.shape[0] * spec.S * ld * es for t in (q, k, v)], q.numel() * 4))
    t = {"q": arena.place("q", q.to(dtype), ld=ld, col0=8), "k": arena.place("k", k.to(dtype), ld=ld, col0=8),
         "v": arena.place("v", v.to(dtype), ld=ld, col0=8),
         "out": arena.place_out("out", (spec.nbr * spec.Kq, spec.S, D), out_dtype, ax.SENTINEL)}
    return spec, arena, t, (c, n, ones, out_dtype)


def _run(monkeypatch, dtype, mutant, fills=mc.FILLS, out_dtype=None):
    spec, arena, t, expect = _setup(dtype, out_dtype)
    ops = fake_ops()
    return mc.check_census_call(monkeypatch, ops, lambda out: fake_ext_attn(ops, t["q"], t["k"], t["v"], out, spec, mutant), arena,
                                t["out"], "out", spec, expect, fills)


@pytest.mark.parametrize("dtype", DTYPES)
def test_honest_op_passes(monkeypatch, dtype):
    reqs = _run(monkeypatch, dtype, None)
    assert reqs == [("attn", SPEC.nbr * SPEC.K * SPAD * SPEC.D * 4)] * 3


ES = 2
MUTANTS = {
    "a": r"byte changed 0 bytes past the end of 'out'",
    "b": rf"byte changed {ES} bytes before 'out'",
    "c": rf"byte changed in a gap column, byte {(8 + SPEC.D) * ES} of 'k' row {1 * SPEC.S + 2} ",
    "d": rf"byte changed at byte {((1 * SPEC.S + 2) * SPEC.D + 3) * ES} inside \(not writable\) 'q'",
    "e1": r"byte changed 0 bytes past the end of 'scratch request 0 \('attn', 3072 bytes\)'",
    "e2": r"byte changed 3071 bytes past the end of 'scratch request 0 \('attn', 3072 bytes\)'",
    "f": r"not finite",
    "g": r"not finite",
    "h": r"fake_ext_attn: pointer argument 0 .* lies outside the arena",
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_mutants_fail_with_name_and_offset(monkeypatch, dtype, mutant):
    assert SPEC.nbr * SPEC.K * SPAD * SPEC.D * 4 == 3072
    with pytest.raises(AssertionError, match=MUTANTS[mutant]):
        _run(monkeypatch, dtype, mutant)


@pytest.mark.parametrize("dtype", DTYPES)
def test_stale_scratch_is_caught_by_the_fill_comparison_alone(monkeypatch, dtype):
    """(f) without the NaN fill, the stale word scaled to one ulp of an fp32 output: every output is finite and inside the
    census tolerance, each run alone could be right -- only the comparison tells.  Under the NaN fill it is not finite."""
    with pytest.raises(AssertionError, match=r"depends on what the scratch held on entry \(fill 0x7f against 0x00\)"):
        _run(monkeypatch, dtype, "fs", fills=(0x00, 0x7F), out_dtype=torch.float32)
    with pytest.raises(AssertionError, match="not finite"):
        _run(monkeypatch, dtype, "fs", fills=(0xFF,), out_dtype=torch.float32)
    _run(monkeypatch, dtype, "f", fills=(0x00,))      # and under the zero fill alone even the plain mutant passes: the fill matters


def test_masked_row_mutant_is_invisible_with_finite_neighbours(monkeypatch):
    """(g) in a dense, finite neighbourhood -- the suite's usual placement -- computes 0 x finite = 0 and passes: the poison
    is what turns the read into a failure."""
    spec = SPEC
    v, ones = ax.census_v(spec)
    c, n = ax.census_expected(spec, v)
    q, k = ax.census_qk(spec, "flat", 3)
    dt = torch.bfloat16
    pad = torch.zeros(8, spec.S, spec.D, dtype=dt)
    dq, dk, dv = q.to(dt), k.to(dt), torch.cat([v.to(dt), pad])[:v.shape[0]]
    out = torch.full((spec.nbr * spec.Kq, spec.S, spec.D), ax.SENTINEL, dtype=dt)
    fake_ext_attn(fake_ops(), dq, dk, dv, out, spec, "g")
    o = out.view(spec.nbr, spec.Kq, spec.S, spec.D)[spec.owned]
    assert ax.census_violation(o, c.view(spec.nbr, spec.Kq, 1, -1)[spec.owned], n.view(spec.nbr, spec.Kq, 1, 1)[spec.owned], "flat", dt) <= 1


# ------------------------------------------------------------------------------------------------ the helper's own facts
def test_poison_reads_as_nan_and_minus_one():
    raw = torch.full((64,), mc.POISON, dtype=torch.uint8)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert bool(torch.isnan(raw.view(dt)).all()), dt
    assert bool((raw.view(torch.int32) == -1).all())
    huge = torch.full((64,), 0x7F, dtype=torch.uint8)
    for dt in (torch.bfloat16, torch.float32):      # (0x7F7F is one more NaN as f16)
        assert bool(torch.isfinite(huge.view(dt)).all()) and float(huge.view(dt)[0]) > 3e38, dt


def test_placement_alignment_gaps_and_guards():
    arena = mc.Arena("cpu", mc.Arena.footprint(3 * 7 * 40 * 2, 5 * 4, 3 * 7 * 24 * 4, 11 * 4))
    a = arena.place("a", torch.ones(3, 7, 24, dtype=torch.bfloat16), ld=40, col0=8)
    i = arena.place("i", torch.arange(5, dtype=torch.int32))
    o = arena.place_out("o", (3, 7, 24), torch.float32, 7.0)
    w = arena.place("w", torch.ones(11), None)
    base = arena.buf.data_ptr()
    assert base % mc.ALIGN == 0
    slabs = list(arena.slabs.values())
    assert all(s.off % mc.ALIGN == 0 for s in slabs)
    assert slabs[0].off >= mc.GUARD and arena.buf.numel() - slabs[-1].end >= mc.GUARD
    assert all(b.off - a_.end >= mc.GAP for a_, b in zip(slabs, slabs[1:]))
    assert a.data_ptr() == base + slabs[0].off + 8 * 2 and a.data_ptr() % 16 == 0
    assert a.stride() == (7 * 40, 40, 1) and a.shape == (3, 7, 24) and bool((a == 1).all())
    assert i.data_ptr() % mc.ALIGN == 0 and o.data_ptr() % mc.ALIGN == 0 and w.data_ptr() % mc.ALIGN == 0
    assert o.is_contiguous() and bool((o == 7).all()) and i.tolist() == [0, 1, 2, 3, 4]
    # every gap column is NaN, the neighbours of the int32 tensor are -1
    full = torch.as_strided(a, (21, 40), (40, 1), a.storage_offset() - 8)
    assert bool(torch.isnan(full[:, :8]).all()) and bool(torch.isnan(full[:, 32:]).all())
    assert int(torch.as_strided(i, (1,), (1,), i.storage_offset() - 1)[0]) == -1 and int(mc_past(i)) == -1
    with pytest.raises(AssertionError, match="multiples of 8"):
        arena.place("bad", torch.ones(2, 24, dtype=torch.bfloat16), ld=36, col0=8)
    with pytest.raises(AssertionError, match="multiples of 8"):
        arena.place("bad2", torch.ones(2, 24, dtype=torch.bfloat16), ld=40, col0=4)
    snap = arena.snapshot()
    assert arena.damage(snap) is None
    o[0, 0, 0] = 1.0
    assert arena.damage(snap, ["o"]) is None and str(arena.damage(snap)) == "byte changed at byte 2 inside (not writable) 'o' (row 0)"


def mc_past(t):
    return _past(t, 1)[0]


def test_scratch_is_exact_aligned_and_guarded(monkeypatch):
    ops = fake_ops()
    sc = mc.Scratch(monkeypatch, ops, 0x7F)
    for nbytes, payload in ((0, 16), (1, 16), (4097, 4112), (3 << 20, 3 << 20)):
        ws = ops._workspace(nbytes, torch.device("cpu"), "nn")
        assert ws.numel() == payload and ws.data_ptr() % mc.ALIGN == 0 and bool((ws == 0x7F).all())
        buf, _ = sc.bufs[-1]
        assert buf.numel() == mc.GUARD + payload + max(1 << 20, nbytes)
        assert bool((buf[:mc.GUARD] == mc.POISON).all()) and bool((buf[mc.GUARD + payload:] == mc.POISON).all())
    assert sc.requests == [("nn", 0), ("nn", 1), ("nn", 4097), ("nn", 3 << 20)] and sc.check() is None
    torch.as_strided(sc.bufs[2][0], (1,), (1,), sc.bufs[2][0].storage_offset() + mc.GUARD - 3)[0] = 0
    d = sc.check()
    assert (d.where, d.offset) == ("before", -3) and "request 2 ('nn', 4097 bytes)" in d.name
