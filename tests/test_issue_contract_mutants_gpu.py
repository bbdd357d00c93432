"""The issue-contract checker has teeth: a torch-only fake op on the GPU (no library kernel), two stages through a scratch tensor,

    scratch = x * 2 ;  out = scratch + y

behind a wrapper shaped like the real ones (scratch cached per stream, graph-owned while a capture runs).  The honest op passes
P1-P4 of tests/issue_contract.py; every mutant breaks the issue discipline in one way and must fail `check` with the message of
exactly the protocol that is there to catch it:

  (a) stage 1 on the default stream                                           P1
  (b) stage 2 on a private side stream, no event edge back                    P1
  (c) a private side stream behind a STALE edge (an event of the last call)   P1
  (d) stream.synchronize() inside the wrapper                                 P2
  (e) x.sum().item() inside the wrapper                                       P2
  (f) one scratch tensor shared by all streams                                P4
  (g) a host-side value read from the inputs by the last eager call, baked    P3
  (h) scratch from a module-level cache while capturing, not from the capture P3 (the 0x7F buffers)

(d) and (e) never run under a capture and (g) reads back only outside one; no mutant touches memory the checker did not hand
it: they compute wrong values or wait.  (b) and (f) keep their stream busy for a few milliseconds between the stages, which
makes the order of events the same in every run.
"""
import pytest
import torch

from tests import issue_contract as ic

pytestmark = pytest.mark.gpu

WS_MIN = 3 << 20        # no other tensor of these tests has this size: a dropped scratch is the block the next request gets


class FakeOps:
    def __init__(self, mutant=None):
        self.mutant = mutant
        self.cache = {}
        self._shared = self._side = self._ev = self._keep = None
        self._baked = 0.0

    def drop_workspaces(self):
        self.cache.clear()

    def _workspace(self, nbytes):
        n = max(nbytes, WS_MIN)
        if self.mutant == "f":
            if self._shared is None or self._shared.numel() < n:
                self._shared = torch.empty(n, dtype=torch.uint8, device="cuda")
            return self._shared
        if self.mutant == "h":       # one cache for everybody, kept in the default stream's pool, capture or not
            ws = self.cache.get("all")
            if ws is None or ws.numel() < n:
                with torch.cuda.stream(torch.cuda.default_stream()):
                    ws = self.cache["all"] = torch.empty(n, dtype=torch.uint8, device="cuda")
            return ws
        if torch.cuda.is_current_stream_capturing():
            return torch.empty(n, dtype=torch.uint8, device="cuda")
        key = torch.cuda.current_stream().cuda_stream
        ws = self.cache.get(key)
        if ws is None or ws.numel() < n:
            ws = self.cache[key] = torch.empty(n, dtype=torch.uint8, device="cuda")
        return ws

    def op(self, x, y, out):
        m = self.mutant
        cur = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream()
        side = self._side
        nbytes = x.numel() * x.element_size()
        if m == "d":
            cur.synchronize()
        if m == "e":
            x.sum().item()
        if m == "g" and not torch.cuda.is_current_stream_capturing():
            self._baked = float(x[0, 0].item())
        if m == "a":
            with torch.cuda.stream(torch.cuda.default_stream()):
                ws = self._workspace(nbytes)
                scratch = ws[:nbytes].view(x.dtype).view_as(x)
                torch.mul(x, 2, out=scratch)
            torch.add(scratch, y, out=out)
        elif m == "b":
            ws = self._workspace(nbytes)
            scratch = ws[:nbytes].view(x.dtype).view_as(x)
            torch.mul(x, 2, out=scratch)
            e = torch.cuda.Event()
            e.record(cur)
            side.wait_event(e)
            ic.Delay(side, ms=5.0)
            with torch.cuda.stream(side):
                torch.add(scratch, y, out=out)
        elif m == "c":
            if self._ev is not None:
                side.wait_event(self._ev)       # the edge of the LAST call
            with torch.cuda.stream(side):
                ws = self._workspace(nbytes)
                scratch = ws[:nbytes].view(x.dtype).view_as(x)
                torch.mul(x, 2, out=scratch)
                torch.add(scratch, y, out=out)
            done = torch.cuda.Event()
            done.record(side)
            cur.wait_event(done)
            self._ev = torch.cuda.Event()
            self._ev.record(cur)
        else:
            ws = self._workspace(nbytes)
            scratch = ws[:nbytes].view(x.dtype).view_as(x)
            torch.mul(x, 2, out=scratch)
            if m == "g":
                scratch[0, 0].fill_(self._baked * 2)
            if m == "f":
                ic.Delay(cur, ms=5.0)
            torch.add(scratch, y, out=out)
        if m in ("a", "b"):     # a scratch in use on another stream is not handed back under it: the mutants stay inside their own memory
            self._keep = ws
        return out


def _bundle(fake, rows=64, cols=512, seed=0):
    g = torch.Generator().manual_seed(seed)
    A = [torch.randn(rows, cols, generator=g).cuda() for _ in range(2)]
    B = [torch.randn(rows, cols, generator=g).cuda() for _ in range(2)]
    return ic.Bundle(lambda t, out: fake.op(t[0], t[1], out), A, B,
                     lambda: torch.full((rows, cols), 7.0, device="cuda"), f"fake op{' (' + fake.mutant + ')' if fake.mutant else ''} {rows}x{cols}")


def _check(fake, protocols, cache=True):
    b = _bundle(fake)
    larger = _bundle(fake, 1024, 1024, seed=1)      # 4 MiB of scratch: the cached 3 MiB are outgrown
    ic.check(b, None, None, None, None, protocols=protocols, drop=fake.drop_workspaces, cache=(lambda: fake.cache) if cache else None,
             ws_bytes=WS_MIN, larger=larger)


def test_honest_op_passes():
    _check(FakeOps(), ic.ALL)


@pytest.mark.parametrize("mutant,protocols,want,text", [
    ("a", ("P1", "P2"), "P1", "late inputs on a busy side stream"),
    ("b", ("P1", "P2"), "P1", "late inputs on a busy side stream"),
    ("c", ("P1", "P2"), "P1", "EARLIER inputs"),
    ("d", ("P1", "P2"), "P2", "the call waited"),
    ("e", ("P1", "P2"), "P2", "the call waited"),
    ("f", ("P1", "P2", "P4"), "P4", "state shared across streams"),
    ("g", ("P1", "P3", "P4"), "P3", "graph replay 1 (set B) differs"),
    ("h", ("P1", "P2", "P3"), "P3", "0x7F buffer"),
])
def test_mutant_fails_its_protocol(mutant, protocols, want, text):
    """(g) reads back on every eager call, so P2 -- which (e) covers -- is left out for it; (h)'s cache is also visible to the
    `cache` probe of P3, which is switched off here so that only the 0x7F step can name it."""
    with pytest.raises(ic.ContractError) as e:
        _check(FakeOps(mutant), protocols, cache=mutant != "h")
    assert e.value.failed == [want], str(e.value)
    assert f"{want}: " in str(e.value) and text in str(e.value), str(e.value)


def test_cache_probe_sees_scratch_cached_during_capture():
    """The S1 probe of P3: a wrapper that caches what it allocated while a capture ran is named."""
    with pytest.raises(ic.ContractError, match="P3: scratch requested while the capture ran was cached"):
        _check(FakeOps("h"), ("P3",))


def test_delay_is_long_enough():
    s = torch.cuda.Stream()
    d = ic.Delay(s)
    s.synchronize()
    assert d.verify("delay") >= ic.MIN_DELAY_MS
