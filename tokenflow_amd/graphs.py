"""HIP-graph replay of launch-bound passes of the hot path.

A UNet pass through the hooks issues dozens of short kernels per transformer block (norm, projections, the
HIP ops, residual adds); at the coarse levels (S <= 256) and on the small configurations every one of them is
shorter than the ~3.5 us it takes the host to issue it, so the step is bound by Python and the launch path, not
by the GPU (cfg2 through the hooks: 16 ms of 33 ms is host issue time; cfg1: 2.3 ms of launches for 0.3 ms of
work).  Nothing in a pass depends on host-side data once its per-module state (`pivotal_pass`, `batch_idx`, `t`)
is fixed, so the whole pass is captured ONCE into a HIP graph and replayed: one host call per pass.

Every `tf_*` entry point is capture-safe (asynchronous on the caller's stream, no allocation, no
synchronisation; `ops._workspace` hands out graph-owned scratch while a capture is running), so a capture taken
through `torch.cuda.graph` contains the library's kernels next to torch's own.  tests/test_issue_contract_gpu.py
captures and replays every single-stream entry point -- attention in all its forms (windows, frame sets, edits,
segments, runs, the `_views` / `_part` forms, `stream=` the capturing stream included), the NN search, the
propagation family, the small kernels and the halo packs -- and found none that is not capturable.  The `streams=`
form of the run wrappers and the rank executors fork streams of their own and are not captured there.

    cache = GraphCache()
    y = cache.run(("chunk", batch_idx, injecting), unet_pass, x)       # captures on first use, replays after

Contract (that of HIP graphs): the callable must do the same launches for the same key -- shapes, dtypes and
every Python-side branch (`t in schedule`, `pivotal_pass`, `batch_idx`) are baked in, which is why they belong in
the key; inputs are COPIED into the capture's static tensors on every replay and the returned tensors are the
capture's static outputs (valid until the next replay of the same key).  Module state assigned inside the
callable (`pivot_hidden_states`, `kf_attn_output`) points at graph-owned tensors that the replay refreshes in
place, which is exactly what the propagation passes of the same step then read.
"""
from typing import Any, Callable, Dict, Hashable, Tuple

import torch

__all__ = ["GraphCache"]


def _flatten(out) -> Tuple[torch.Tensor, ...]:
    if isinstance(out, torch.Tensor):
        return (out,)
    if out is None:
        return ()
    return tuple(t for o in out for t in _flatten(o))


class _Entry:
    __slots__ = ("graph", "static_in", "out")

    def __init__(self, graph, static_in, out):
        self.graph, self.static_in, self.out = graph, static_in, out


class GraphCache:
    """key -> captured HIP graph of `fn(*inputs)`.  One instance per model / stream.

    Every graph gets its OWN memory pool by default: a propagation-pass graph has the addresses of the pivotal
    pass's cached tensors baked in, and those tensors live in the pivotal graph's pool -- with a shared pool a
    later capture could be handed that memory once Python drops its last reference to it (an eager pass
    re-assigning `kf_attn_output`, say).  `share_pool=True` trades that safety for footprint when all passes are
    captured back to back and only ever replayed."""

    def __init__(self, warmup: int = 1, share_pool: bool = False):
        self._entries: Dict[Hashable, _Entry] = {}
        self._pool = None
        self._share_pool = share_pool
        self._warmup = warmup
        self._side = None          # ONE warm-up stream per cache (ops._workspace caches scratch per stream)

    def __len__(self):
        return len(self._entries)

    def clear(self):
        self._entries.clear()
        self._pool = None

    def inputs(self, key: Hashable) -> Tuple[torch.Tensor, ...]:
        """The capture's static input tensors of `key`: a producer that writes its results straight into them (and
        passes them back to `run`) pays no input copy per replay -- inside a real UNet the block inputs are produced
        by the preceding layers of the same graph and are never copied either."""
        return self._entries[key].static_in

    def run(self, key: Hashable, fn: Callable[..., Any], *inputs: torch.Tensor):
        e = self._entries.get(key)
        if e is None:
            e = self._capture(fn, inputs)
            self._entries[key] = e
            return e.out
        for dst, src in zip(e.static_in, inputs):
            if dst.shape != src.shape or dst.dtype != src.dtype:
                raise ValueError(f"GraphCache: input {tuple(src.shape)}/{src.dtype} does not match the capture "
                                 f"{tuple(dst.shape)}/{dst.dtype} of this key")
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        e.graph.replay()
        return e.out

    def _capture(self, fn, inputs) -> _Entry:
        if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in inputs):
            raise TypeError("GraphCache: inputs must be CUDA tensors (everything else belongs in the key)")
        static_in = tuple(t.clone() for t in inputs)
        # eager warm-up on a side stream (lazy initialisation, autotuning, workspace growth must not be captured)
        if self._side is None:
            self._side = torch.cuda.Stream()
        side = self._side
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(self._warmup):
                fn(*static_in)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        from . import ops
        ops.drop_workspaces(side)      # the warm-up's scratch (tens of MB at level 0) is not needed again
        graph = torch.cuda.CUDAGraph()
        pool = None
        if self._share_pool:
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            pool = self._pool
        with torch.cuda.graph(graph, pool=pool):
            out = fn(*static_in)
        _flatten(out)       # outputs must be tensors (or nests of tensors)
        graph.replay()      # the capture itself executes nothing: produce this call's results
        return _Entry(graph, static_in, out)
