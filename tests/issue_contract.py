"""The issue contract of a call, made checkable: every launch of a call goes to the stream the caller is on (or behind an
event edge from it), the call returns without waiting for the GPU, it can be captured into a HIP graph and replayed, and two
calls on two streams do not share state (include/tokenflow_hip.h: "never allocates, never synchronises, keeps no global
mutable state (re-entrant per stream)"; "all launches are asynchronous on that stream").

Tests that issue on the default stream and check after a device-wide synchronise cannot see any of this: a launch on the
wrong stream, a missing event edge and a hidden host synchronise all give correct results there.  `check` runs a call under
protocols in which they do not:

  P1  late inputs on a busy side stream: the tensors hold set A, a fresh stream is kept busy by `Delay`, set B is copied in
      BEHIND the delay, the call is issued; the result -- as the caller's stream sees it -- must be that of set B.  Any piece of
      the call that went to another stream without an edge from the caller's has run at once and has read A.
  P2  the call does not wait: when it returns in P1 the stream is still busy and the delay's own end event has not passed (a
      wrapper that waited and then queued its kernels leaves the stream busy for a moment, but the delay behind it).
  P3  graph replay: captured once (after an eager warm-up on a side stream and `drop`), replayed with A, B, A.  Before the replays
      the eager scratch is dropped and buffers of its size are filled with 0x7F: a graph that points at eager scratch computes
      into them.  Nothing may be cached while the capture runs.  Afterwards the case and a larger one run eagerly.
  P4  beside itself: the case on A and on B on two streams at once (two streams that a short probe showed to run side by side;
      the two delays must end within OVERLAP_MS of each other); then the case and a larger one of the same scratch tag back to
      back on one busy stream (the cached scratch grows while the first call is still queued).

The expected value of a call on set X is the same call issued eagerly on the default stream with X, followed by a synchronise
(the arithmetic is held to exact references elsewhere); everything is compared bit for bit.  The eager results of A and B must
differ in every output row the call writes, otherwise an early read could not be told from a late one.

A stimulus that did not take place -- a delay shorter than MIN_DELAY_MS, two calls that did not overlap -- is reported with
pytest.fail("... not exercised"), never as a pass or a skip.  tests/test_issue_contract_mutants_gpu.py proves on torch-only
mutants that every protocol bites.  Nothing here imports the GPU package.
"""
import pytest
import torch

DELAY_MS = 50.0
MIN_DELAY_MS = 20.0
OVERLAP_MS = 2.0        # P4: the two streams' delays must end this close together
JUNK = 0x7F
ALL = ("P1", "P2", "P3", "P4")


class ContractError(AssertionError):
    """`failed`: the protocols that failed, in order, e.g. ["P1"]; the message names each."""

    def __init__(self, what, failures):
        self.failed = list(dict.fromkeys(p for p, _ in failures))
        super().__init__(f"{what}: " + "; ".join(f"{p}: {msg}" for p, msg in failures))


# --------------------------------------------------------------------------------------------------------------- Delay
class Delay:
    """A busy wait of about `ms` milliseconds enqueued on `stream`, between two events; `measured()` (after the stream was
    synchronised) is what it took.  Calibrated once per process on an idle stream."""
    _rate = None        # units (cycles of torch.cuda._sleep, or matrix products) per millisecond
    _mm = None

    @classmethod
    def _spin(cls, units):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(int(units))
        else:       # a chain of large products on tensors that belong to no test
            if cls._mm is None:
                cls._mm = [torch.ones(2048, 2048, device="cuda") for _ in range(2)]
            for _ in range(max(1, int(units))):
                torch.mm(cls._mm[0], cls._mm[0], out=cls._mm[1])

    @classmethod
    def rate(cls):
        if cls._rate is None:
            torch.cuda.synchronize()
            s = torch.cuda.Stream()
            units = 1_000_000 if hasattr(torch.cuda, "_sleep") else 4
            with torch.cuda.stream(s):
                cls._spin(units)        # first launch: module loading is not timed
                s.synchronize()
                for _ in range(12):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    cls._spin(units)
                    e1.record(s)
                    s.synchronize()
                    ms = e0.elapsed_time(e1)
                    if ms >= 5.0:
                        break
                    units *= 4
            if ms < 5.0:
                pytest.fail(f"Delay: not exercised: {units} units of busy wait took {ms:.3f} ms, no rate to calibrate")
            cls._rate = units / ms
        return cls._rate

    def __init__(self, stream, ms=DELAY_MS):
        units = self.rate() * ms
        self.t0, self.t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.t0.record(stream)
            self._spin(units)
            self.t1.record(stream)

    def measured(self):
        return self.t0.elapsed_time(self.t1)

    def verify(self, what):
        ms = self.measured()
        if ms < MIN_DELAY_MS:
            pytest.fail(f"{what}: not exercised: the delay took {ms:.1f} ms, less than {MIN_DELAY_MS} ms")
        return ms


# ------------------------------------------------------------------------------------------------------------- helpers
def _flat(out):
    if isinstance(out, torch.Tensor):
        return (out,)
    return tuple(out)


def bits(t):
    """The raw bytes of a tensor, [rows, bytes of a row] (a row: the last dim; a 1-D tensor is one row)."""
    t = t.contiguous()
    last = t.shape[-1] if t.dim() else 1
    return t.view(torch.uint8).reshape(-1, last * t.element_size())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _first_diff(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if not same_bits(g, w):
            rows = (bits(g) != bits(w)).any(dim=1).nonzero().flatten()
            return f"output {i}: {rows.numel()} of {bits(g).shape[0]} rows differ, first row {int(rows[0])}"
    return None


def _fill(work, src):
    for t, x in zip(work, src):
        t.copy_(x)


def _snap(out):
    return tuple(t.clone() for t in _flat(out))


class Bundle:
    """A call with its two input sets and its outputs: `call(tensors, out)`, `A`, `B` (lists of device tensors of the same
    shapes and dtypes), `make_out()` (fresh sentinel-filled outputs: a tensor or a tuple of tensors).  The eager references
    are computed on first use and kept."""

    def __init__(self, call, A, B, make_out, what):
        self.call, self.A, self.B, self.make_out, self.what = call, list(A), list(B), make_out, what
        assert len(self.A) == len(self.B) and all(a.shape == b.shape and a.dtype == b.dtype and a.is_cuda and b.is_cuda
                                                  for a, b in zip(self.A, self.B)), f"{what}: A and B must match"
        self._ref = None

    def work(self, src=None):
        w = [a.clone() for a in self.A]
        if src is not None:
            _fill(w, src)
        return w

    def eager(self, src):
        """The call issued on the default stream with the set `src`, synchronised."""
        out, work = self.make_out(), self.work(src)
        torch.cuda.synchronize()            # the inputs are complete and the device is idle
        self.call(work, out)
        torch.cuda.synchronize()
        return _snap(out)

    def ref(self):
        """(eager(A), eager(B)); asserts that they differ in every row the call writes."""
        if self._ref is None:
            ra, rb = self.eager(self.A), self.eager(self.B)
            blank = _snap(self.make_out())
            n_owned = 0
            for i, (a, b, z) in enumerate(zip(ra, rb, blank)):
                owned = (bits(a) != bits(z)).any(dim=1) | (bits(b) != bits(z)).any(dim=1)
                differ = (bits(a) != bits(b)).any(dim=1)
                n_owned += int(owned.sum())
                same = owned & ~differ
                assert not bool(same.any()), (f"{self.what}: precondition: eager(A) and eager(B) agree in row "
                                              f"{int(same.nonzero()[0])} of output {i}: choose A and B so that every row differs")
            assert n_owned > 0, f"{self.what}: precondition: the call wrote nothing"
            self._ref = (ra, rb)
        return self._ref


# --------------------------------------------------------------------------------------------------------------- check
def _p1_p2(b, protocols, fail):
    ra, rb = b.ref()
    work = b.work(b.A)
    out = b.make_out()
    b.eager(b.A)                            # the eager warm-up: library and module loading are not counted in P2
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = Delay(s)
        _fill(work, b.B)
        b.call(work, out)
        pending = not s.query() and not d.t1.query()    # (the delay's own end event: work queued behind a hidden wait does not count)
        seen = _snap(out)                   # the result as the caller's stream sees it
    s.synchronize()
    torch.cuda.synchronize()
    ms = d.verify(f"{b.what} P1")
    if "P1" in protocols:
        diff = _first_diff(seen, rb)
        if diff is not None:
            early = _first_diff(seen, ra) is None
            fail("P1", f"late inputs on a busy side stream: the result is not that of the inputs copied in behind the delay ({diff})"
                       + ("; it is that of the EARLIER inputs: a piece of the call ran ahead of the caller's stream" if early else ""))
    if "P2" in protocols and not pending:
        fail("P2", f"the call waited: the stream was idle when the call returned, behind a delay of {ms:.0f} ms")


def _junk(ws_bytes, streams):
    """Two buffers of the eager scratch's size per stream, filled with 0x7F."""
    bufs = []
    for s in streams:
        with torch.cuda.stream(s):
            for _ in range(2):
                t = torch.empty(max(int(ws_bytes), 256), dtype=torch.uint8, device="cuda")
                t.fill_(JUNK)
                bufs.append(t)
    torch.cuda.synchronize()
    return bufs


def _p3(b, fail, drop, cache, ws_bytes, larger, label="P3"):
    ra, rb = b.ref()
    work = b.work(b.A)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        b.call(work, b.make_out())
    cur.wait_stream(side)
    torch.cuda.synchronize()
    drop()
    out = b.make_out()
    blank = _snap(out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.call(work, out)
    if cache is not None and len(cache()):
        fail(label, f"scratch requested while the capture ran was cached for later eager calls: {sorted(cache(), key=str)}")
    drop()
    junk = _junk(ws_bytes, (cur, side)) if ws_bytes else []
    for n, (name, src, want) in enumerate((("A", b.A, ra), ("B", b.B, rb), ("A", b.A, ra))):
        _fill(work, src)
        _fill(_flat(out), blank)
        graph.replay()
        torch.cuda.synchronize()
        diff = _first_diff(_flat(out), want)
        if diff is not None:
            fail(label, f"graph replay {n} (set {name}) differs from the eager result of that set ({diff})")
            break
    for j in junk:
        if not bool((j == JUNK).all()):
            fail(label, "graph replay wrote into a 0x7F buffer allocated after the capture: the graph points at eager scratch, "
                        "not at scratch it owns")
            break
    del junk
    for bb in (b,) + ((larger,) if larger is not None else ()):     # eager calls after the capture (what a cached buffer would serve)
        diff = _first_diff(bb.eager(bb.B), bb.ref()[1])
        if diff is not None:
            fail(label, f"an eager call of {bb.what} after the capture differs from its reference ({diff})")
    del graph


def _stream_pair(what, tries=8, ms=4.0):
    """Two fresh streams whose work runs side by side: two streams that share a hardware queue run one after the other, and P4
    would exercise nothing on them.  A pair is probed with two short delays and taken when these end together."""
    for _ in range(tries):
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        d1, d2 = Delay(s1, ms), Delay(s2, ms)
        s1.synchronize()
        s2.synchronize()
        if abs(d1.t1.elapsed_time(d2.t1)) < ms / 4:
            return s1, s2
    pytest.fail(f"{what}: not exercised: no two of {2 * tries} fresh streams ran side by side")


def _p4(b, fail, drop, larger):
    ra, rb = b.ref()
    # The stimulus is the overlap.  Now and then two streams that ran a short probe side by side still run the long delays one
    # after the other (hardware queues are shared among streams); that says nothing about the call, so the stimulus is set up
    # again on other streams, three times at the most, and only a run that overlapped is judged.
    for attempt in range(3):
        w1, w2, o1, o2 = b.work(b.A), b.work(b.B), b.make_out(), b.make_out()
        torch.cuda.synchronize()
        s1, s2 = _stream_pair(f"{b.what} P4")
        d1, d2 = Delay(s1), Delay(s2)
        for s, w, o in ((s1, w1, o1), (s2, w2, o2)):
            with torch.cuda.stream(s):
                b.call(w, o)
        seen = []
        for s, o in ((s1, o1), (s2, o2)):
            with torch.cuda.stream(s):
                seen.append(_snap(o))
        s1.synchronize()
        s2.synchronize()
        torch.cuda.synchronize()
        d1.verify(f"{b.what} P4")
        d2.verify(f"{b.what} P4")
        # both delays were enqueued before either call: the calls start together when the delays ran side by side and ended together
        apart = abs(d1.t1.elapsed_time(d2.t1))
        if apart <= OVERLAP_MS:
            break
        print(f"{b.what} P4: attempt {attempt}: the two streams' delays ended {apart:.1f} ms apart; setting the stimulus up again")
    else:
        pytest.fail(f"{b.what} P4: not exercised: the two streams' delays ended {apart:.1f} ms apart (they did not run side by side)")
    for n, (got, want) in enumerate(((seen[0], ra), (seen[1], rb))):
        diff = _first_diff(got, want)
        if diff is not None:
            fail("P4", f"beside itself: the call on stream {n + 1} of two differs from its eager result ({diff}): state shared "
                       "across streams")
            return
    if larger is None:
        return
    drop()
    w1, w2, o1, o2 = b.work(b.A), larger.work(larger.B), b.make_out(), larger.make_out()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = Delay(s)
        b.call(w1, o1)
        larger.call(w2, o2)
        seen = (_snap(o1), _snap(o2))
    s.synchronize()
    torch.cuda.synchronize()
    d.verify(f"{b.what} P4")
    for got, want, name in ((seen[0], ra, b.what), (seen[1], larger.ref()[1], larger.what)):
        diff = _first_diff(got, want)
        if diff is not None:
            fail("P4", f"back to back on one stream ({b.what}, then {larger.what}): {name} differs from its eager result ({diff}): "
                       "scratch replaced under a queued launch")
            return


def check(call, inputs_A, inputs_B, make_out, what, protocols=ALL, drop=None, cache=None, ws_bytes=0, larger=None):
    """Run `call(tensors, out)` under `protocols`; raises ContractError naming every protocol that failed.
    drop(): forget the wrapper's cached scratch (ops.drop_workspaces); cache(): the wrapper's scratch cache (a container that
    must stay empty while a capture runs); ws_bytes: the eager scratch of the call; larger: a Bundle of a larger case of the
    same scratch tag (P3's eager calls after the capture, P4's back-to-back run).  `call` may also be a Bundle."""
    b = call if isinstance(call, Bundle) else Bundle(call, inputs_A, inputs_B, make_out, what)
    drop = drop if drop is not None else (lambda: None)
    failures = []

    def fail(p, msg):
        failures.append((p, msg))

    assert set(protocols) <= set(ALL), protocols
    b.ref()
    if "P1" in protocols or "P2" in protocols:
        _p1_p2(b, protocols, fail)
    if "P3" in protocols:
        _p3(b, fail, drop, cache, ws_bytes, larger)
    if "P4" in protocols:
        _p4(b, fail, drop, larger)
    torch.cuda.synchronize()
    if failures:
        raise ContractError(b.what, failures)
