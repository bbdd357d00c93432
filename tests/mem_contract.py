"""The memory contract of a call, made checkable: a call reads its inputs only inside their rows and columns, writes only
the rows of `out` it owns and the scratch it asked for, and its result does not depend on what the scratch held on entry.

  * `Arena`: ONE uint8 allocation filled with POISON in which every tensor of a call is placed, at least 4 KiB apart, with
    64 KiB of guard at both ends.  A byte that changed outside the tensors named writable is damage; `damage()` names the
    nearest tensor and the byte offset relative to it.  Inputs are not writable: "q and k are not modified" is an assertion.
  * `Scratch`: replaces `ops._workspace` for one test.  Every request gets a buffer of its own, guard | payload | guard, the
    payload of EXACTLY the size asked for (rounded up to 16 bytes) and filled with a byte of the test's choice; the rear guard
    is at least as large as the payload, so a size function that under-reports by up to a factor of two lands in memory the
    test owns and fails an assertion.
  * `Spy`: wraps `ops._launch` and records the pointer arguments of every entry-point call; `assert_inside` fails where a
    wrapper copied a tensor (a test that ran on a copy has tested nothing).

POISON = 0xFF is NaN as bf16, f16 and fp32 and -1 as int32 (an invalid row index, an invalid slot count).
tests/test_mem_contract_cpu.py proves on mutated ops that `verify` and the fill comparison have teeth; tests/test_mem_contract_gpu.py
runs the kernels under them.  Nothing here imports the GPU package.
"""
import math

import torch

from tests import attn_exact as ax

POISON = 0xFF
FILLS = (0xFF, 0x00, 0x7F)      # NaN | zero | huge finite (0x7F7F.. is 3.39e38 as bf16 and fp32; as f16 it is one more NaN)
ALIGN = 256
GAP = 4 << 10
GUARD = 64 << 10
SCRATCH_REAR_MIN = 1 << 20


def _up(n, a):
    return (n + a - 1) // a * a


def _aligned_bytes(nbytes, device):
    """A uint8 tensor of nbytes whose data_ptr() is a multiple of ALIGN."""
    raw = torch.empty(nbytes + ALIGN, dtype=torch.uint8, device=device)
    off = (-raw.data_ptr()) % ALIGN
    return raw[off:off + nbytes]


class Damage:
    """The first byte a call changed that was not its to change: `name` the nearest tensor (or scratch request), `where`
    one of "before" | "after" | "gap" | "inside", `offset` in bytes: the distance in front of the tensor's first byte
    (before, negative), past its last byte (after, 0 = the very next byte), inside its slab (gap, inside)."""

    def __init__(self, name, where, offset, detail=""):
        self.name, self.where, self.offset, self.detail = name, where, offset, detail

    def __str__(self):
        place = {"before": f"{-self.offset} bytes before", "after": f"{self.offset} bytes past the end of",
                 "gap": f"in a gap column, byte {self.offset} of", "inside": f"at byte {self.offset} inside (not writable)"}
        return f"byte changed {place[self.where]} '{self.name}'{' ' + self.detail if self.detail else ''}"


class _Slab:
    def __init__(self, name, off, rows, row_bytes, ld_bytes, col0_bytes):
        self.name, self.off, self.rows, self.row_bytes, self.ld_bytes, self.col0_bytes = name, off, rows, row_bytes, ld_bytes, col0_bytes
        self.extent = rows * ld_bytes

    @property
    def end(self):
        return self.off + self.extent


class Arena:
    """One POISON-filled uint8 allocation of `capacity` bytes on `device` (`Arena.footprint` sizes it)."""

    def __init__(self, device, capacity=8 << 20):
        self.device = torch.device(device)
        self.buf = _aligned_bytes(capacity, self.device)
        self.buf.fill_(POISON)
        self.slabs = {}
        self.top = GUARD

    @staticmethod
    def footprint(*nbytes):
        """Capacity for slabs of these sizes (rows x ld x element size for a strided one)."""
        return 2 * GUARD + sum(_up(n, ALIGN) + GAP for n in nbytes)

    # ---- placement
    def _reserve(self, name, shape, dtype, ld, col0):
        assert name not in self.slabs, name
        es = torch.empty((), dtype=dtype).element_size()
        cols = shape[-1] if len(shape) else 1
        rows = math.prod(shape[:-1]) if len(shape) > 1 else 1
        if ld is None:
            assert col0 == 0
            ld = cols
        else:
            assert ld % 8 == 0 and col0 % 8 == 0, "token stride and first column: multiples of 8 elements (16-byte pieces)"
        assert 0 <= col0 and col0 + cols <= ld
        slab = _Slab(name, _up(self.top, ALIGN), rows, cols * es, ld * es, col0 * es)
        assert slab.end + GUARD <= self.buf.numel(), f"arena too small for '{name}' ({slab.end + GUARD} > {self.buf.numel()})"
        self.top = slab.end + GAP
        self.slabs[name] = slab
        full = self.buf[slab.off:slab.end].view(dtype).view(rows, ld)
        view = full[:, col0:col0 + cols]
        if len(shape) == 1:
            return view[0]
        return view.unflatten(0, tuple(shape[:-1])) if len(shape) > 2 else view

    def place(self, name, t, ld=None, col0=0):
        """Copy the CPU tensor `t` in at an ALIGN-ed offset; returns the view on it: dense, or (ld) with a stride of `ld`
        elements between the rows of the last dim, the values in columns col0 .. of every row, the other columns POISON."""
        view = self._reserve(name, tuple(t.shape), t.dtype, ld, col0)
        view.copy_(t)
        return view

    def place_out(self, name, shape, dtype, fill):
        """A dense output of `shape` filled with `fill` (the sentinel of the project's tests)."""
        view = self._reserve(name, tuple(shape), dtype, None, 0)
        view.fill_(fill)
        return view

    def contains(self, ptr):
        base = self.buf.data_ptr()
        return base <= ptr < base + self.buf.numel()

    # ---- damage
    def snapshot(self):
        return self.buf.clone()

    def _mask(self, writable):
        m = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.device)
        for name in writable:
            s = self.slabs[name]
            m[s.off:s.end].view(s.rows, s.ld_bytes)[:, s.col0_bytes:s.col0_bytes + s.row_bytes] = True
        return m

    def locate(self, pos):
        """The Damage record of arena byte `pos`."""
        for s in self.slabs.values():
            if s.off <= pos < s.end:
                r, c = divmod(pos - s.off, s.ld_bytes)
                if s.col0_bytes <= c < s.col0_bytes + s.row_bytes:
                    return Damage(s.name, "inside", r * s.row_bytes + c - s.col0_bytes, f"(row {r})")
                return Damage(s.name, "gap", c, f"row {r} (the values start at byte {s.col0_bytes} of a row of {s.ld_bytes})")
        best = None
        dist = lambda d: d.offset + 1 if d.where == "after" else -d.offset      # noqa: E731
        for s in self.slabs.values():
            d = Damage(s.name, "before", pos - s.off) if pos < s.off else Damage(s.name, "after", pos - s.end)
            if best is None or dist(d) < dist(best):
                best = d
        return best if best is not None else Damage("arena", "inside", pos)

    def damage(self, snapshot, writable=()):
        """None, or the Damage of the first byte that differs from `snapshot` outside the values of the `writable` tensors."""
        changed = (self.buf != snapshot) & ~self._mask(writable)
        if not bool(changed.any()):
            return None
        return self.locate(int(changed.nonzero()[0]))


class Scratch:
    """`ops._workspace` replaced for a test: exact, guarded, `fill`-ed buffers, one per request."""

    def __init__(self, monkeypatch, ops, fill):
        self.fill, self.requests, self.bufs = fill, [], []
        monkeypatch.setattr(ops, "_workspace", self._workspace)

    def _workspace(self, nbytes, device, tag="attn", stream=None):
        nbytes = int(nbytes)
        payload = max(16, _up(nbytes, 16))
        rear = max(SCRATCH_REAR_MIN, nbytes)
        buf = _aligned_bytes(GUARD + payload + rear, device)
        buf.fill_(POISON)
        ws = buf[GUARD:GUARD + payload]
        ws.fill_(self.fill)
        assert ws.numel() == payload and ws.data_ptr() % ALIGN == 0
        self.requests.append((tag, nbytes))
        self.bufs.append((buf, payload))
        return ws

    def contains(self, ptr):
        return any(b.data_ptr() <= ptr < b.data_ptr() + b.numel() for b, _ in self.bufs)

    def check(self):
        """None, or the Damage of the first guard byte that is no longer POISON (offset: distance from the payload)."""
        for i, ((buf, payload), (tag, nbytes)) in enumerate(zip(self.bufs, self.requests)):
            name = f"scratch request {i} ('{tag}', {nbytes} bytes)"
            bad = buf[GUARD + payload:] != POISON
            if bool(bad.any()):
                return Damage(name, "after", int(bad.nonzero()[0]))
            bad = buf[:GUARD] != POISON
            if bool(bad.any()):
                return Damage(name, "before", int(bad.nonzero()[-1]) - GUARD)
        return None


class Spy:
    """`ops._launch` wrapped: records (entry point, pointer arguments) of every call.  A pointer argument is a plain int at
    or above 2^32 (sizes, flags and masks stay below; tables travel as ctypes pointers and are host memory)."""

    def __init__(self, monkeypatch, ops):
        self.calls = []
        inner = ops._launch

        def launch(dev, what, fn, *args, **kw):
            self.calls.append((what, [(i, a) for i, a in enumerate(args) if type(a) is int and a >= 1 << 32]))
            return inner(dev, what, fn, *args, **kw)
        monkeypatch.setattr(ops, "_launch", launch)

    def assert_inside(self, arena, scratch=None):
        assert self.calls, "no entry point was called"
        for what, ptrs in self.calls:
            for i, p in ptrs:
                if not (arena.contains(p) or (scratch is not None and scratch.contains(p))):
                    raise AssertionError(f"{what}: pointer argument {i} ({p:#x}) lies outside the arena: the wrapper ran on a copy")


def verify(arena, snapshot, writable, scratch=None, spy=None):
    """The contract of the call(s) made since `snapshot`; raises AssertionError naming the first violation."""
    if spy is not None:
        spy.assert_inside(arena, scratch)
    d = arena.damage(snapshot, writable)
    assert d is None, str(d)
    if scratch is not None:
        d = scratch.check()
        assert d is None, str(d)


def assert_finite(what, t):
    bad = ~torch.isfinite(t.float())
    if bool(bad.any()):
        pos = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} values are not finite; first at {pos} (a read of unwritten scratch or of a "
                             "row / column past the end)")


def assert_same_across_fills(what, by_fill):
    """by_fill: {scratch fill byte: result tensor}: all bit-equal."""
    fills = list(by_fill)
    ref = by_fill[fills[0]]
    for f in fills[1:]:
        got = by_fill[f]
        same = torch.equal(got.contiguous().view(torch.uint8), ref.contiguous().view(torch.uint8))
        if not same:
            ne = (got != ref) | (torch.isnan(got.float()) != torch.isnan(ref.float())) if got.is_floating_point() else got != ref
            pos = tuple(int(x) for x in ne.nonzero()[0]) if bool(ne.any()) else ()
            raise AssertionError(f"{what}: the result depends on what the scratch held on entry (fill {f:#04x} against "
                                 f"{fills[0]:#04x}); first difference at {pos}")


def check_census_call(monkeypatch, ops, call, arena, out, out_name, spec, expect, fills=FILLS, what="census"):
    """One census call under every scratch fill, held to the whole contract.  call(out): the call under test; `expect` the
    census (c, N, ones mask, out dtype).  Returns the scratch requests seen."""
    c, n, ones, out_dtype = expect
    c4, n4 = c.view(spec.nbr, spec.Kq, 1, -1)[spec.owned], n.view(spec.nbr, spec.Kq, 1, 1)[spec.owned]
    by_fill, requests = {}, []
    for fill in fills:
        out.fill_(ax.SENTINEL)
        snap = arena.snapshot()
        with monkeypatch.context() as mp:
            scratch, spy = Scratch(mp, ops, fill), Spy(mp, ops)
            call(out)
            verify(arena, snap, [out_name], scratch, spy)
            requests += scratch.requests
        o = out.cpu().view(spec.nbr, spec.Kq, spec.S, spec.D)
        for b in range(spec.nbr):
            if b not in spec.owned:
                assert bool((o[b] == ax.SENTINEL).all()), f"{what}: branch {b} is not the call's to write"
        assert_finite(f"{what} fill {fill:#04x}", o[spec.owned])
        viol = ax.census_violation(o[spec.owned], c4, n4, "flat", out_dtype)
        assert viol <= 1.0, f"{what} fill {fill:#04x}: {viol:.3g} x the census tolerance"
        if out_dtype != torch.float32:
            assert bool((o[spec.owned][..., ones] == 1).all()), f"{what} fill {fill:#04x}: the ones channel is not exactly 1"
        by_fill[fill] = o.clone()
    assert_same_across_fills(what, by_fill)
    return requests
