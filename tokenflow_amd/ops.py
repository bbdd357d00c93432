"""Torch-tensor wrappers over the C ABI.  PyTorch supplies device memory and the
current HIP stream; all arithmetic happens in the HIP kernels.  No fallbacks."""
import ctypes
import os
from typing import Optional, Sequence

import torch

from . import _lib

_DT = {torch.bfloat16: _lib.TF_BF16, torch.float16: _lib.TF_F16, torch.float32: _lib.TF_F32}


def _need_gpu(*ts):
    """All tensors on ONE GPU (no CPU fallback, no cross-device launches)."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.TokenflowHipError(
                "tokenflow_amd ops run on MI355X only: got a CPU tensor (there is no CPU fallback)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise _lib.TokenflowHipError(f"tokenflow_amd ops: tensors on different devices ({dev} and {t.device})")
    return dev


def _launch(dev, what: str, fn, *args, stream: Optional[int] = None):
    """Call a C-ABI entry point whose last argument is the stream: the launch goes to the CURRENT stream OF THE
    TENSORS' DEVICE (or to `stream`, a raw HIP stream of that device, when the caller orders its own streams), with
    that device made current for the duration of the call when it is not already (a kernel enqueued on another
    device's stream with foreign pointers faults or corrupts memory)."""
    if dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            rc = fn(*args, torch.cuda.current_stream(dev).cuda_stream if stream is None else stream)
    else:
        rc = fn(*args, torch.cuda.current_stream(dev).cuda_stream if stream is None else stream)
    if rc != 0:
        _lib.check(rc, what)


# 16-bit type fp32 tensors are rounded to at the op boundary (an fp32 model run WITHOUT autocast; under autocast the
# projections already arrive in the autocast dtype).  bf16 (default) cannot overflow; TOKENFLOW_FP32_AS=f16 keeps 11
# significand bits instead of 8 -- the reference's own GPU dtype (run_tokenflow_pnp.py:47, 220) -- for models whose
# activations stay inside f16's range.
def _fp32_as_from_env() -> torch.dtype:
    name = os.environ.get("TOKENFLOW_FP32_AS", "bf16").strip().lower()
    table = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "f16": torch.float16, "fp16": torch.float16,
             "float16": torch.float16, "half": torch.float16}
    if name not in table:
        raise ValueError(f"TOKENFLOW_FP32_AS={name!r}: must be 'bf16' or 'f16' (aliases: bfloat16, fp16, float16, half)")
    return table[name]


# f16 has no overflow guard: an fp32 activation above 65504 becomes inf in q / k / v / the pivots
FP32_AS = _fp32_as_from_env()


def compute_dtype(t: torch.Tensor) -> torch.dtype:
    """16-bit MFMA input type used for a tensor of dtype t.dtype (fp32 inputs are rounded to `FP32_AS`)."""
    return t.dtype if t.dtype in (torch.bfloat16, torch.float16) else FP32_AS


def _caller_buffer(what: str, name: str, buf: Optional[torch.Tensor], shape, dtype: torch.dtype, device) -> torch.Tensor:
    """A result tensor: a fresh one, or the caller's `buf` -- contiguous, of exactly this shape, dtype and device."""
    shape = tuple(shape)
    if buf is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(buf.shape) != shape or buf.dtype != dtype or not buf.is_contiguous() or buf.device != device:
        raise ValueError(f"{what}: `{name}` must be a contiguous {list(shape)} tensor of {dtype} on {device}")
    return buf


_ws_cache = {}
_attn_ws_bytes = {}   # (K, S, H, Dh, dtype) -> scratch bytes of tf_ext_attn_fwd (a pure function of the shape)


def _scratch(nbytes: int, device, key) -> torch.Tensor:
    """`_workspace` with the launch's stream (of the tensors' device) current."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _ws_cache[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    return ws


def _workspace(nbytes: int, device, tag: str = "attn", stream: Optional[int] = None) -> torch.Tensor:
    """Scratch for one launch, cached per (purpose, device, stream).  While a HIP graph is being captured the
    buffer comes from the graph's private pool and must live and die with that graph: never cached.
    stream: the raw HIP stream the launch goes to when that is not torch's current one.  Capture state and allocation are
    then THAT stream's: the buffer is allocated with `stream` current, so torch's allocator ties the block to it and --
    dropped or outgrown -- hands it out again in that stream's order only, never to the current stream while launches
    on `stream` that use it are still queued."""
    cur = torch.cuda.current_stream(device)
    other_device = device.index != torch.cuda.current_device()      # capture state is a property of the TENSORS' device's stream
    if stream is None or stream == cur.cuda_stream:
        if other_device:
            with torch.cuda.device(device):
                return _scratch(nbytes, device, (tag, device.index, cur.cuda_stream))
        return _scratch(nbytes, device, (tag, device.index, cur.cuda_stream))
    ext = torch.cuda.ExternalStream(stream, device=device)
    if other_device:
        with torch.cuda.stream(ext):
            return _scratch(nbytes, device, (tag, device.index, stream))
    torch.cuda.set_stream(ext)      # (the context manager costs several microseconds more per call)
    try:
        return _scratch(nbytes, device, (tag, device.index, stream))
    finally:
        torch.cuda.set_stream(cur)


def drop_workspaces(stream=None) -> None:
    """Forget the cached scratch of `stream` (a torch.cuda.Stream; None = every stream): the memory goes back to
    torch's allocator once the launches that used it have run."""
    if stream is None:
        _ws_cache.clear()
        return
    for key in [k for k in _ws_cache if k[2] == stream.cuda_stream]:
        del _ws_cache[key]


# TOKENFLOW_FOLD_SCALE=1: at head dim 40 fold the softmax scale into q (rounded to the input dtype): several % faster,
# 3-12x outside the parity bound on peaked logits (profiles/r02_fold_accuracy.txt).  Default: fp32 scaling of the scores.
FOLD_SCALE = os.environ.get("TOKENFLOW_FOLD_SCALE", "0") not in ("", "0")
# TOKENFLOW_ATTN_NO_SPLIT=1: never split a bank problem over workgroups.  By default small grids (a sharded rank, the
# 16x16 level) split the bank into runs of frames and merge; the merge re-associates fp32 sums, so results then
# depend on the grid size in the last bits.  With the flag the arithmetic of a (query, head) is the same everywhere.
NO_SPLIT = os.environ.get("TOKENFLOW_ATTN_NO_SPLIT", "0") not in ("", "0")


def _attn_flags(inject: bool, part: str, out_f32: bool, fold_scale: Optional[bool], no_split: Optional[bool],
                fused: Optional[bool], hints: int) -> int:
    """The TF_ATTN_* bit mask of an ext_attn / ext_attn_views / attn_plan call."""
    flags = (1 if inject else 0) | (_lib.TF_ATTN_FOLD_SCALE if (FOLD_SCALE if fold_scale is None else fold_scale) else 0)
    if out_f32:
        flags |= _lib.TF_ATTN_OUT_F32
    flags |= {"all": 0, "bank": _lib.TF_ATTN_BANK_ONLY, "source": _lib.TF_ATTN_SOURCE_ONLY}[part]
    if NO_SPLIT if no_split is None else no_split:
        flags |= _lib.TF_ATTN_NO_SPLIT
    return flags | int(hints) | (0 if fused is None else _lib.TF_ATTN_FUSED if fused else _lib.TF_ATTN_NO_FUSED)


def _plan_tokens(what: str, fn, *args) -> list:
    buf = ctypes.create_string_buffer(4096)
    n = fn(*args, buf, len(buf))
    if n < 0:
        _lib.check(n, what)
    toks = buf.value.decode().split(";") if n else []
    assert len(toks) == n, (toks, n)
    return toks


def attn_plan(K: int, Kq: int, S: int, heads: int, dh: int, inject: bool, dtype: torch.dtype = torch.bfloat16,
              part: str = "all", out_dtype: Optional[torch.dtype] = None, fold_scale: Optional[bool] = None,
              no_split: Optional[bool] = None, fused: Optional[bool] = None, hints: int = 0) -> list:
    """The launches `ext_attn` makes for dense [3K,S,heads*dh] / [3Kq,S,heads*dh] tensors with these arguments, as
    tokens (tf_ext_attn_plan: e.g. ['vt_pack', 'il<40,8,ALL,4,3>']).  Host only: needs no GPU."""
    flags = _attn_flags(inject, part, out_dtype == torch.float32, fold_scale, no_split, fused, hints)
    return _plan_tokens("tf_ext_attn_plan", _lib.load().tf_ext_attn_plan, K, Kq, S, heads, dh, flags, _DT[dtype])


def attn_run_plan(K: int, Kq: int, run_n: int, n_runs: int, S: int, heads: int, dh: int, inject: bool,
                  dtype: torch.dtype = torch.bfloat16, bank_only: bool = False, out_dtype: Optional[torch.dtype] = None,
                  fold_scale: Optional[bool] = None, no_split: bool = False, hints: int = 0) -> list:
    """The launches of ONE run call of `ext_attn_runs` over run_n of the bank's K frames, followed by the merge of n_runs
    runs, as tokens (tf_ext_attn_run_plan: e.g. ['vt_pack', 'il<40,8,ALL,4,2,run>', 'merge[runs=3]']).  Host only."""
    flags = _run_flags(inject, bank_only, out_dtype == torch.float32, fold_scale, no_split, hints)
    return _plan_tokens("tf_ext_attn_run_plan", _lib.load().tf_ext_attn_run_plan, K, Kq, run_n, n_runs, S, heads, dh, flags,
                        _DT[dtype])


def _multi_v_bits(multi_v: Optional[bool], multi_v64: Optional[bool] = None) -> int:
    """multi_v: the four-bank form at head dim 40 forced on / off; False switches the form off at EVERY head dim.
    multi_v64: True forces the form on at head dim 64 (TF_ATTN_MULTI_V64); None / False leave it to the library's measured
    rule.
    multi_v=False with multi_v64=True is the library's TF_ERR_SHAPE."""
    bits = 0 if multi_v is None else _lib.TF_ATTN_MULTI_V if multi_v else _lib.TF_ATTN_NO_MULTI_V
    return bits | (_lib.TF_ATTN_MULTI_V64 if multi_v64 else 0)


def _edit_mask(what: str, mask, n_edits: int, inject: bool = False) -> int:
    """A per-edit mask (bit e = edit e, 0-based) checked against the number of edits; it excludes the shared `inject`."""
    E, m = int(n_edits), int(mask)
    if not 1 <= E <= _lib.TF_MAX_EDITS:
        raise ValueError(f"{what}: n_edits={n_edits} (1 .. {_lib.TF_MAX_EDITS})")
    if inject:
        raise ValueError(f"{what}: inject=True beside a mask (the mask is the injection state)")
    if m < 0 or m >> E:
        raise ValueError(f"{what}: mask {m:#x} has bits outside the {E} edits")
    return m


def attn_edits_plan(K: int, Kq: int, S: int, heads: int, dh: int, inject: bool, n_edits: int,
                    dtype: torch.dtype = torch.bfloat16, out_dtype: Optional[torch.dtype] = None,
                    fold_scale: Optional[bool] = None, no_split: Optional[bool] = None, fused: Optional[bool] = None,
                    multi_v: Optional[bool] = None, hints: int = 0, inject_mask: Optional[int] = None,
                    multi_v64: Optional[bool] = None) -> list:
    """The launches `ext_attn_edits` makes for dense [(1+2E)K,S,heads*dh] tensors, as tokens (tf_ext_attn_edits_plan: the
    tokens of `attn_plan`; the four-bank launch of a pair of edits is 'one<40,1,4,MV4,2,fq0>', at head dim 64 with
    multi_v64=True 'one<64,1,8,MV4,2,fq1>').  Host only: needs no GPU.
    inject_mask: the per-edit injection state of `ext_attn_edits` (tf_ext_attn_edits_masked_plan); `inject` must be False."""
    flags = _attn_flags(inject, "all", out_dtype == torch.float32, fold_scale, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    if inject_mask is not None:
        mask = _edit_mask("attn_edits_plan", inject_mask, n_edits, inject)
        return _plan_tokens("tf_ext_attn_edits_masked_plan", _lib.load().tf_ext_attn_edits_masked_plan, K, Kq, S, heads, dh,
                            int(n_edits), mask, flags, _DT[dtype])
    return _plan_tokens("tf_ext_attn_edits_plan", _lib.load().tf_ext_attn_edits_plan, K, Kq, S, heads, dh, int(n_edits), flags,
                        _DT[dtype])


def propagate_edits_plan(n: int, n_chunks: int, S: int, D: int, first_single: bool, n_edits: int) -> list:
    """The launches of `propagate_chunks_edits`: the search tokens of `nn_plan` (no finalize: the gather merges the splits)
    followed by ONE gather over all 1 + 2E branches, 'gather[branches=B]'.  Host only."""
    return _plan_tokens("tf_nn_gather_blend_edits_plan", _lib.load().tf_nn_gather_blend_edits_plan, int(n), int(n_chunks), S, D,
                        1 if first_single else 0, int(n_edits))


def _segments(what: str, segments, K: int):
    """The keyframes per segment of a pass as a ctypes int array: 1 .. TF_MAX_SEGMENTS segments of >= 1 keyframes, sum K."""
    seg = [int(x) for x in segments]
    if not 1 <= len(seg) <= _lib.TF_MAX_SEGMENTS or any(x < 1 for x in seg):
        raise ValueError(f"{what}: segments {seg} (1 .. {_lib.TF_MAX_SEGMENTS} segments of >= 1 keyframes)")
    if sum(seg) != K:
        raise ValueError(f"{what}: the segments {seg} hold {sum(seg)} keyframes, the pass {K}")
    return (ctypes.c_int * len(seg))(*seg)


def attn_segments_plan(K: int, segments: Sequence[int], S: int, heads: int, dh: int, inject: bool,
                       dtype: torch.dtype = torch.bfloat16, out_dtype: Optional[torch.dtype] = None,
                       fold_scale: Optional[bool] = None, no_split: Optional[bool] = None, fused: Optional[bool] = None,
                       hints: int = 0) -> list:
    """The launches `ext_attn_segments` makes for dense [3K,S,heads*dh] tensors, as tokens (tf_ext_attn_segments_plan: the
    tokens of `attn_plan`; the joint launch of the fused segments is 'fused[..,sets=N]').  Host only: needs no GPU."""
    seg = _segments("attn_segments_plan", segments, K)
    flags = _attn_flags(inject, "all", out_dtype == torch.float32, fold_scale, no_split, fused, hints)
    return _plan_tokens("tf_ext_attn_segments_plan", _lib.load().tf_ext_attn_segments_plan, K, len(seg), seg, S, heads, dh,
                        flags, _DT[dtype])


def bank_windows(K: int, radius: int) -> list:
    """The clamped symmetric windows of a sliding-window bank: keyframe i attends to the keyframes max(0, i - radius) ..
    min(K - 1, i + radius), as [(first frame, frames)] per keyframe.  radius >= K - 1 gives K full windows."""
    K, R = int(K), int(radius)
    if K < 1 or R < 0:
        raise ValueError(f"bank_windows: K={K} radius={R} (K >= 1, radius >= 0)")
    return [(max(0, i - R), min(K - 1, i + R) - max(0, i - R) + 1) for i in range(K)]


def _windows(what: str, windows, K: int, Kq: int, q_frame0: int = 0):
    """The window table of a call as two ctypes int arrays (first frames, frame counts): one window per query frame, inside
    the bank, holding its own frame."""
    win = [(int(lo), int(n)) for lo, n in windows]
    if len(win) != Kq or not 1 <= Kq <= _lib.TF_MAX_WINDOW_FRAMES:
        raise ValueError(f"{what}: {len(win)} windows for {Kq} query frames (one each, at most {_lib.TF_MAX_WINDOW_FRAMES})")
    for i, (lo, n) in enumerate(win):
        if n < 1 or lo < 0 or lo + n > K:
            raise ValueError(f"{what}: window {i} = [{lo}, {lo + n}) (>= 1 frames inside the {K}-frame bank)")
        if not lo <= q_frame0 + i < lo + n:
            raise ValueError(f"{what}: window {i} = [{lo}, {lo + n}) does not hold its own frame {q_frame0 + i}")
    return (ctypes.c_int * Kq)(*[w[0] for w in win]), (ctypes.c_int * Kq)(*[w[1] for w in win])


def attn_windows_plan(K: int, windows, S: int, heads: int, dh: int, inject: bool, dtype: torch.dtype = torch.bfloat16,
                      out_dtype: Optional[torch.dtype] = None, no_split: Optional[bool] = None,
                      fused: Optional[bool] = None, hints: int = 0) -> list:
    """The launches `ext_attn_windows` makes for dense [3K,S,heads*dh] tensors, as tokens (tf_ext_attn_windows_plan: the
    tokens of `attn_plan` with ',win' appended to the windowed launch, e.g. ['vt_pack', 'il<40,8,ALL,4,2>,win'] or
    ['fused[qw=1,kw=4,qb=1,prec=1,win]']; K full windows give `attn_plan(K, K, ...)`).  Host only: needs no GPU."""
    lo, n = _windows("attn_windows_plan", windows, K, K)
    flags = _attn_flags(inject, "all", out_dtype == torch.float32, False, no_split, fused, hints)
    return _plan_tokens("tf_ext_attn_windows_plan", _lib.load().tf_ext_attn_windows_plan, K, K, 0, S, heads, dh, flags,
                        _DT[dtype], ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p))


def attn_windows_part_plan(K: int, Kq: int, q_frame0: int, windows, S: int, heads: int, dh: int, inject: bool,
                           dtype: torch.dtype = torch.bfloat16, part: str = "bank", out_dtype: Optional[torch.dtype] = None,
                           no_split: Optional[bool] = None, fused: Optional[bool] = None, hints: int = 0) -> list:
    """The launches `ext_attn_windows_views` makes for dense tensors, as tokens (tf_ext_attn_windows_part_plan): Kq query frames
    from bank frame q_frame0 on, one window each, over a bank of K frames; part "bank" (TF_ATTN_BANK_ONLY: what a frame-sharded
    rank runs over its halo-extended bank) or "all" (= `attn_windows_plan` for Kq = K).  The bank launch's token carries ',win'.
    The source part of a windowed pass is window-free: `attn_plan(Kq, Kq, ..., part="source")`.  Host only: needs no GPU."""
    if part not in ("bank", "all"):
        raise ValueError(f"attn_windows_part_plan: part {part!r} (\"bank\" or \"all\": the source part is window-free)")
    lo, n = _windows("attn_windows_part_plan", windows, K, Kq, int(q_frame0))
    flags = _attn_flags(inject, part, out_dtype == torch.float32, False, no_split, fused, hints)
    return _plan_tokens("tf_ext_attn_windows_part_plan", _lib.load().tf_ext_attn_windows_part_plan, K, Kq, int(q_frame0), S,
                        heads, dh, flags, _DT[dtype], ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p))


def attn_windows_edits_plan(K: int, windows, S: int, heads: int, dh: int, n_edits: int, inject_mask: int,
                            dtype: torch.dtype = torch.bfloat16, out_dtype: Optional[torch.dtype] = None,
                            no_split: Optional[bool] = None, fused: Optional[bool] = None, multi_v: Optional[bool] = None,
                            multi_v64: Optional[bool] = None, hints: int = 0) -> list:
    """The launches `ext_attn_windows_edits` makes for dense [(1+2E)K,S,heads*dh] tensors, as tokens
    (tf_ext_attn_windows_edits_plan: the tokens of `attn_edits_plan` with ',win' appended to every windowed bank launch; the
    windowed four-bank launch of a pair of injecting edits is 'one<40,1,4,MV4,2,fq0>,win' / 'one<64,1,8,MV4,2,fq1>,win').
    n_edits = 1 gives `attn_windows_plan`, K full windows `attn_edits_plan(inject_mask=...)`.  Host only: needs no GPU."""
    lo, n = _windows("attn_windows_edits_plan", windows, K, K)
    mask = _edit_mask("attn_windows_edits_plan", inject_mask, n_edits)
    flags = _attn_flags(False, "all", out_dtype == torch.float32, False, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    return _plan_tokens("tf_ext_attn_windows_edits_plan", _lib.load().tf_ext_attn_windows_edits_plan, K, K, 0, S, heads, dh,
                        int(n_edits), mask, flags, _DT[dtype], ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p))


def bank_frame_sets(K: int, radius: int, anchors=()) -> list:
    """The frame sets of an anchored sliding-window bank, one int mask per keyframe: bit j of mask i = keyframe i attends to
    keyframe j.  Mask i is window i of `bank_windows(K, radius)` plus every anchor (global keyframes that all keyframes see;
    0 <= a < K, duplicates are fine).  No anchors give the windows as masks; radius >= K - 1 gives K full sets."""
    K = int(K)
    anc = 0
    for a in anchors:
        if isinstance(a, bool) or int(a) != a or not 0 <= int(a) < K:
            raise ValueError(f"bank_frame_sets: anchor {a!r} (keyframe indices 0 <= a < {K})")
        anc |= 1 << int(a)
    return [(((1 << n) - 1) << lo) | anc for lo, n in bank_windows(K, radius)]


def _frame_sets(what: str, sets, K: int, Kq: int, q_frame0: int = 0):
    """The set table of a call as a ctypes uint64 array: one non-empty mask per query frame, inside the bank, holding its own
    frame."""
    masks = [int(m) for m in sets]
    if K > 64:
        raise ValueError(f"{what}: K={K} (a set is a 64-bit mask: at most 64 bank frames)")
    if len(masks) != Kq or not 1 <= Kq <= _lib.TF_MAX_WINDOW_FRAMES:
        raise ValueError(f"{what}: {len(masks)} sets for {Kq} query frames (one each, at most {_lib.TF_MAX_WINDOW_FRAMES})")
    for i, m in enumerate(masks):
        if m <= 0 or m >> K:
            raise ValueError(f"{what}: set {i} = {m:#x} (>= 1 frames inside the {K}-frame bank)")
        if not (m >> (q_frame0 + i)) & 1:
            raise ValueError(f"{what}: set {i} = {m:#x} does not hold its own frame {q_frame0 + i}")
    return (ctypes.c_uint64 * Kq)(*masks)


def attn_frame_sets_plan(K: int, sets, S: int, heads: int, dh: int, inject: bool, dtype: torch.dtype = torch.bfloat16,
                         out_dtype: Optional[torch.dtype] = None, no_split: Optional[bool] = None,
                         fused: Optional[bool] = None, hints: int = 0) -> list:
    """The launches `ext_attn_frame_sets` makes for dense [3K,S,heads*dh] tensors, as tokens (tf_ext_attn_frame_sets_plan: the
    tokens of `attn_plan` with ',set' appended to the launch that walks the sets, e.g. ['vt_pack', 'il<40,8,ALL,4,2>,set'] or
    ['fused[qw=1,kw=4,qb=1,prec=1,set]']; sets that are all contiguous ranges give `attn_windows_plan`, K full sets
    `attn_plan(K, K, ...)`).  Host only: needs no GPU."""
    tab = _frame_sets("attn_frame_sets_plan", sets, K, K)
    flags = _attn_flags(inject, "all", out_dtype == torch.float32, False, no_split, fused, hints)
    return _plan_tokens("tf_ext_attn_frame_sets_plan", _lib.load().tf_ext_attn_frame_sets_plan, K, K, 0, S, heads, dh, flags,
                        _DT[dtype], ctypes.cast(tab, ctypes.c_void_p))


def attn_frame_sets_part_plan(K: int, Kq: int, q_frame0: int, sets, S: int, heads: int, dh: int, inject: bool,
                              dtype: torch.dtype = torch.bfloat16, part: str = "bank", out_dtype: Optional[torch.dtype] = None,
                              no_split: Optional[bool] = None, fused: Optional[bool] = None, hints: int = 0) -> list:
    """The launches `ext_attn_frame_sets_views` makes for dense tensors, as tokens (tf_ext_attn_frame_sets_part_plan): Kq query
    frames from bank frame q_frame0 on, one set each, over a bank of K <= 64 frames (on a shard the rank's extended bank); part
    "bank" (TF_ATTN_BANK_ONLY: what a frame-sharded rank runs over its anchor-extended bank) or "all" (= `attn_frame_sets_plan`
    for Kq = K).  The bank launch's token carries ',set' (',win' where every set is a range: `attn_windows_part_plan`).  The
    source part of a frame-set pass is set-free: `attn_plan(Kq, Kq, ..., part="source")`.  Host only: needs no GPU."""
    if part not in ("bank", "all"):
        raise ValueError(f"attn_frame_sets_part_plan: part {part!r} (\"bank\" or \"all\": the source part is set-free)")
    tab = _frame_sets("attn_frame_sets_part_plan", sets, K, Kq, int(q_frame0))
    flags = _attn_flags(inject, part, out_dtype == torch.float32, False, no_split, fused, hints)
    return _plan_tokens("tf_ext_attn_frame_sets_part_plan", _lib.load().tf_ext_attn_frame_sets_part_plan, K, Kq, int(q_frame0), S,
                        heads, dh, flags, _DT[dtype], ctypes.cast(tab, ctypes.c_void_p))


def attn_frame_sets_edits_plan(K: int, sets, S: int, heads: int, dh: int, n_edits: int, inject_mask: int,
                               dtype: torch.dtype = torch.bfloat16, out_dtype: Optional[torch.dtype] = None,
                               no_split: Optional[bool] = None, fused: Optional[bool] = None, multi_v: Optional[bool] = None,
                               multi_v64: Optional[bool] = None, hints: int = 0) -> list:
    """The launches `ext_attn_frame_sets_edits` makes for dense [(1+2E)K,S,heads*dh] tensors, as tokens
    (tf_ext_attn_frame_sets_edits_plan: the tokens of `attn_edits_plan` with ',set' appended to every bank launch that walks
    the sets; the frame-set four-bank launch of a pair of injecting edits is 'one<40,1,4,MV4,2,fq0>,set' /
    'one<64,1,8,MV4,2,fq1>,set').  n_edits = 1 gives `attn_frame_sets_plan`, sets that are all contiguous ranges
    `attn_windows_edits_plan`, K full sets `attn_edits_plan(inject_mask=...)`.  Host only: needs no GPU."""
    tab = _frame_sets("attn_frame_sets_edits_plan", sets, K, K)
    mask = _edit_mask("attn_frame_sets_edits_plan", inject_mask, n_edits)
    flags = _attn_flags(False, "all", out_dtype == torch.float32, False, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    return _plan_tokens("tf_ext_attn_frame_sets_edits_plan", _lib.load().tf_ext_attn_frame_sets_edits_plan, K, K, 0, S, heads,
                        dh, int(n_edits), mask, flags, _DT[dtype], ctypes.cast(tab, ctypes.c_void_p))


def _single_mask(what: str, mask, C: int) -> int:
    m = int(mask)
    if not 1 <= C <= 64 or m < 0 or m >> C:
        raise ValueError(f"{what}: single_mask {m:#x} over {C} chunks (1 .. 64 chunks, no bit at or above them)")
    return m


def propagate_segments_plan(n: int, n_chunks: int, S: int, D: int, single_mask: int) -> list:
    """The launches of `propagate_chunks_segments` for n_chunks > 1: the search tokens of `nn_plan(n*S, S, D, 2, n_chunks)`
    (no finalize: the gather merges the splits) followed by 'gather[branches=3]'.  Host only."""
    return _plan_tokens("tf_nn_gather_blend_segments_plan", _lib.load().tf_nn_gather_blend_segments_plan, int(n),
                        int(n_chunks), S, D, _single_mask("propagate_segments_plan", single_mask, int(n_chunks)))


def _chunk_frames(what: str, chunk_frames):
    """The frames per chunk of a ragged run as (list, ctypes int array): 1 .. 64 chunks of >= 1 frames."""
    fr = [int(x) for x in chunk_frames]
    if not 1 <= len(fr) <= 64 or any(x < 1 for x in fr):
        raise ValueError(f"{what}: chunk_frames {fr} (1 .. 64 chunks of >= 1 frames)")
    return fr, (ctypes.c_int * len(fr))(*fr)


def propagate_ragged_plan(chunk_frames, S: int, D: int, single_mask: int = 0, n_edits: int = 1) -> list:
    """The launches of `propagate_chunks_ragged` (tf_nn_gather_blend_ragged_plan).  Equal frame counts: the tokens of
    `propagate_segments_plan` (n_edits = 1) or `propagate_edits_plan`.  Otherwise the search token of the form the rule
    picks -- `nn_plan(ceil(sum(frames) * S / C), S, D, 2, C)`'s, the split taken on the real panel count -- with ',ragged'
    in its brackets, then 'gather[branches=B,ragged]'.  Host only."""
    fr, arr = _chunk_frames("propagate_ragged_plan", chunk_frames)
    return _plan_tokens("tf_nn_gather_blend_ragged_plan", _lib.load().tf_nn_gather_blend_ragged_plan, arr, len(fr), S, D,
                        _single_mask("propagate_ragged_plan", single_mask, len(fr)), int(n_edits))


def nn_plan(n_tgt: int, S: int, D: int, P: int, C: int = 1) -> list:
    """The search launches of `nn_search` (C = 1) or of `propagate_chunks` over C > 1 chunks of n_tgt targets (P = 2),
    as tokens (tf_nn_search_plan: e.g. ['glds[splits=2]', 'finalize']).  Host only: needs no GPU."""
    return _plan_tokens("tf_nn_search_plan", _lib.load().tf_nn_search_plan, int(n_tgt), S, D, P, C)


def ext_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float,
             inject: bool, out: Optional[torch.Tensor] = None, q_frame0: int = 0,
             fold_scale: Optional[bool] = None, part: str = "all",
             out_dtype: Optional[torch.dtype] = None, no_split: Optional[bool] = None,
             fused: Optional[bool] = None, hints: int = 0) -> torch.Tensor:
    """Extended attention core (tokenflow_utils.py:124-197).  k,v: [3K,S,D] bf16/f16 (the bank),
    q: [3Kq,S,D] = the queries of keyframes q_frame0..q_frame0+Kq-1 (Kq = K on one GPU); last dim
    contiguous, equal token stride (q, k, v may be column slabs of one fused projection output).
    Returns [3Kq,S,D] in the same dtype, or in fp32 with out_dtype=torch.float32 (the normalised fp32
    accumulator, no 16-bit output rounding).
    part = "bank": only the uncond/cond branches are computed (the source slabs of v and out, and those
    of q, k that the call does not read, are never touched); part = "source": only the source branch.
    no_split: True = one pass per bank problem whatever the grid (TF_ATTN_NO_SPLIT: arithmetic independent of the
    grid size), False = let small grids split the bank over workgroups and merge; None = the module default.
    fused: None = the library decides (small problems run in ONE fused launch, csrc/ext_attn_fused.hip), False = the
    streaming kernels at every size (TF_ATTN_NO_FUSED), True = the fused kernel at any size it is built for;
    hints: further TF_ATTN_* bits (_lib.attn_hint, TF_ATTN_PRECISE_P ...; measurements and tests)."""
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    B, S, D = k.shape
    Bq = q.shape[0]
    if B % 3 or Bq % 3 or D % heads or q.shape[1:] != k.shape[1:] or v.shape != k.shape:
        raise ValueError(f"ext_attn: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} heads {heads}")
    K, Kq, dh = B // 3, Bq // 3, D // heads
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"ext_attn: q/k/v must share dtype bf16 or f16, got {q.dtype},{k.dtype},{v.dtype}")

    def rows(t):
        if t.stride(-1) != 1 or t.stride(0) != S * t.stride(1):
            t = t.contiguous()
        return t
    q, k, v = rows(q), rows(k), rows(v)
    ld = q.stride(1)
    if k.stride(1) != ld or v.stride(1) != ld:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ld = D
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    if out_dtype not in (q.dtype, torch.float32):
        raise TypeError(f"ext_attn: out_dtype {out_dtype} (the input dtype or float32)")
    if out is None:
        out = torch.empty(Bq, S, D, dtype=out_dtype, device=q.device)
    elif out.dtype != out_dtype or not out.is_contiguous() or out.shape != (Bq, S, D):
        raise ValueError("ext_attn: `out` must be a contiguous [3Kq,S,D] tensor of out_dtype")
    flags = _attn_flags(inject, part, out_dtype == torch.float32, fold_scale, no_split, fused, hints)
    key = (K, S, heads, dh, dt)
    nbytes = _attn_ws_bytes.get(key)
    if nbytes is None:
        nbytes = _attn_ws_bytes[key] = lib.tf_ext_attn_workspace_bytes(K, S, heads, dh, dt)
    ws = _workspace(nbytes, q.device)
    _launch(dev, "tf_ext_attn_fwd", lib.tf_ext_attn_fwd, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
            K, Kq, int(q_frame0), S, heads, dh, ld, float(scale), flags, dt, ws.data_ptr(), ws.numel())
    return out


def ext_attn_segments(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, inject: bool,
                      segments: Sequence[int], out: Optional[torch.Tensor] = None, fold_scale: Optional[bool] = None,
                      out_dtype: Optional[torch.dtype] = None, no_split: Optional[bool] = None,
                      fused: Optional[bool] = None, hints: int = 0) -> torch.Tensor:
    """`ext_attn` for a pass of several scenes or clips (tf_ext_attn_fwd_segments): q, k, v [3K,S,D] as there, `segments` the
    keyframes per segment (consecutive frame windows, sum K).  The slices of a segment are what `ext_attn` computes on that
    segment's tensors alone: a bank branch attends to the keys of its own segment only.  Segments whose own call is a fused
    small-problem launch share ONE fused launch; the others share one V^T pre-pass and are bit-identical to their own
    calls.  A single segment is `ext_attn`.  Arguments as `ext_attn` (no `part`, no q_frame0: every keyframe's queries)."""
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    B, S, D = k.shape
    if B % 3 or D % heads or q.shape != k.shape or v.shape != k.shape:
        raise ValueError(f"ext_attn_segments: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} heads {heads}")
    K, dh = B // 3, D // heads
    seg = _segments("ext_attn_segments", segments, K)
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"ext_attn_segments: q/k/v must share dtype bf16 or f16, got {q.dtype},{k.dtype},{v.dtype}")

    def rows(t):
        if t.stride(-1) != 1 or t.stride(0) != S * t.stride(1):
            t = t.contiguous()
        return t
    q, k, v = rows(q), rows(k), rows(v)
    ld = q.stride(1)
    if k.stride(1) != ld or v.stride(1) != ld:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ld = D
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    if out_dtype not in (q.dtype, torch.float32):
        raise TypeError(f"ext_attn_segments: out_dtype {out_dtype} (the input dtype or float32)")
    if out is None:
        out = torch.empty(B, S, D, dtype=out_dtype, device=q.device)
    elif out.dtype != out_dtype or not out.is_contiguous() or out.shape != (B, S, D):
        raise ValueError("ext_attn_segments: `out` must be a contiguous [3K,S,D] tensor of out_dtype")
    flags = _attn_flags(inject, "all", out_dtype == torch.float32, fold_scale, no_split, fused, hints)
    ws = _workspace(lib.tf_ext_attn_segments_workspace_bytes(K, S, heads, dh, dt), q.device)
    _launch(dev, "tf_ext_attn_fwd_segments", lib.tf_ext_attn_fwd_segments, q.data_ptr(), k.data_ptr(), v.data_ptr(),
            out.data_ptr(), K, len(seg), seg, S, heads, dh, ld, float(scale), flags, dt, ws.data_ptr(), ws.numel())
    return out


def ext_attn_windows(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, inject: bool, windows, *,
                     no_split: Optional[bool] = None, fused: Optional[bool] = None, hints: int = 0,
                     out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`ext_attn` over a sliding-window keyframe bank (tf_ext_attn_fwd_windows): q, k, v [3K,S,D] as there, `windows` one
    (first frame, frames) pair per keyframe (`bank_windows(K, radius)`).  The uncond / cond branches of keyframe i attend to
    the keys of the keyframes of window i only -- under `inject` with the source's q and k -- and the source branch to its own
    frame.  NOT TokenFlow's computation unless every window is the whole bank (then the call is `ext_attn`, bit for bit):
    an opt-in whose cost grows with the window, not with the bank.  One launch for all keyframes; keyframe i's slices are
    what `ext_attn` computes on window i's tensors alone (Kq = 1), bit for bit under no_split wherever both take the same
    kernel form.  Arguments as `ext_attn` (no `part`, no q_frame0, no folded scale)."""
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    B, S, D = k.shape
    if B % 3 or D % heads or q.shape != k.shape or v.shape != k.shape:
        raise ValueError(f"ext_attn_windows: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} heads {heads}")
    K, dh = B // 3, D // heads
    lo, n = _windows("ext_attn_windows", windows, K, K)
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"ext_attn_windows: q/k/v must share dtype bf16 or f16, got {q.dtype},{k.dtype},{v.dtype}")

    def rows(t):
        if t.stride(-1) != 1 or t.stride(0) != S * t.stride(1):
            t = t.contiguous()
        return t
    q, k, v = rows(q), rows(k), rows(v)
    ld = q.stride(1)
    if k.stride(1) != ld or v.stride(1) != ld:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ld = D
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    if out_dtype not in (q.dtype, torch.float32):
        raise TypeError(f"ext_attn_windows: out_dtype {out_dtype} (the input dtype or float32)")
    if out is None:
        out = torch.empty(B, S, D, dtype=out_dtype, device=q.device)
    elif out.dtype != out_dtype or not out.is_contiguous() or out.shape != (B, S, D):
        raise ValueError("ext_attn_windows: `out` must be a contiguous [3K,S,D] tensor of out_dtype")
    flags = _attn_flags(inject, "all", out_dtype == torch.float32, False, no_split, fused, hints)
    key = (K, S, heads, dh, dt)
    nbytes = _attn_ws_bytes.get(key)
    if nbytes is None:
        nbytes = _attn_ws_bytes[key] = lib.tf_ext_attn_workspace_bytes(K, S, heads, dh, dt)
    ws = _workspace(nbytes, q.device)
    fs, ofs = S * ld, S * D   # dense [3, K, S, ld] tensors, out [3, K, S, D]
    strides = (ctypes.c_int64 * 9)(K * fs, fs, K * fs, fs, K * fs, fs, K * ofs, ofs, ld)
    _launch(dev, "tf_ext_attn_fwd_windows", lib.tf_ext_attn_fwd_windows, q.data_ptr(), k.data_ptr(), v.data_ptr(),
            out.data_ptr(), K, K, 0, S, heads, dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale), flags, dt,
            ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p), ws.data_ptr(), ws.numel())
    return out


def ext_attn_frame_sets(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, inject: bool, sets, *,
                        no_split: Optional[bool] = None, fused: Optional[bool] = None, hints: int = 0,
                        out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`ext_attn` over a frame-set keyframe bank (tf_ext_attn_fwd_frame_sets): q, k, v [3K,S,D] as there, `sets` one int mask
    per keyframe (`bank_frame_sets(K, radius, anchors)`: a sliding window plus global anchor keyframes; any other sparsity is
    a table of masks too).  The uncond / cond branches of keyframe i attend to the keys of the keyframes whose bits are set
    in mask i, in ascending order -- under `inject` with the source's q and k -- and the source branch to its own frame.  NOT
    TokenFlow's computation unless every set is the whole bank (then the call is `ext_attn`, bit for bit; sets that are all
    contiguous ranges are `ext_attn_windows`).  One launch for all keyframes; keyframe i's slices are what `ext_attn`
    computes on the member frames of set i gathered next to each other (Kq = 1), bit for bit under no_split wherever both
    take the same kernel form.  Arguments as `ext_attn_windows`, with masks instead of pairs."""
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    B, S, D = k.shape
    if B % 3 or D % heads or q.shape != k.shape or v.shape != k.shape:
        raise ValueError(f"ext_attn_frame_sets: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} heads {heads}")
    K, dh = B // 3, D // heads
    tab = _frame_sets("ext_attn_frame_sets", sets, K, K)
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"ext_attn_frame_sets: q/k/v must share dtype bf16 or f16, got {q.dtype},{k.dtype},{v.dtype}")

    def rows(t):
        if t.stride(-1) != 1 or t.stride(0) != S * t.stride(1):
            t = t.contiguous()
        return t
    q, k, v = rows(q), rows(k), rows(v)
    ld = q.stride(1)
    if k.stride(1) != ld or v.stride(1) != ld:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ld = D
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    if out_dtype not in (q.dtype, torch.float32):
        raise TypeError(f"ext_attn_frame_sets: out_dtype {out_dtype} (the input dtype or float32)")
    if out is None:
        out = torch.empty(B, S, D, dtype=out_dtype, device=q.device)
    elif out.dtype != out_dtype or not out.is_contiguous() or out.shape != (B, S, D):
        raise ValueError("ext_attn_frame_sets: `out` must be a contiguous [3K,S,D] tensor of out_dtype")
    flags = _attn_flags(inject, "all", out_dtype == torch.float32, False, no_split, fused, hints)
    key = (K, S, heads, dh, dt)
    nbytes = _attn_ws_bytes.get(key)
    if nbytes is None:
        nbytes = _attn_ws_bytes[key] = lib.tf_ext_attn_workspace_bytes(K, S, heads, dh, dt)
    ws = _workspace(nbytes, q.device)
    fs, ofs = S * ld, S * D   # dense [3, K, S, ld] tensors, out [3, K, S, D]
    strides = (ctypes.c_int64 * 9)(K * fs, fs, K * fs, fs, K * fs, fs, K * ofs, ofs, ld)
    _launch(dev, "tf_ext_attn_fwd_frame_sets", lib.tf_ext_attn_fwd_frame_sets, q.data_ptr(), k.data_ptr(), v.data_ptr(),
            out.data_ptr(), K, K, 0, S, heads, dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale), flags, dt,
            ctypes.cast(tab, ctypes.c_void_p), ws.data_ptr(), ws.numel())
    return out


def ext_attn_edits(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, inject: bool,
                   n_edits: int, out: Optional[torch.Tensor] = None, q_frame0: int = 0,
                   fold_scale: Optional[bool] = None, out_dtype: Optional[torch.dtype] = None,
                   no_split: Optional[bool] = None, fused: Optional[bool] = None, multi_v: Optional[bool] = None,
                   hints: int = 0, inject_mask: Optional[int] = None, multi_v64: Optional[bool] = None) -> torch.Tensor:
    """`ext_attn` for a multi-edit batch: E = n_edits edits of one source video, B = 1 + 2E branches
    [source | uncond_1 | cond_1 | ... | uncond_E | cond_E].  k, v: [B*K,S,D], q: [B*Kq,S,D]; returns [B*Kq,S,D].
    The slices of edit e (source, uncond_e, cond_e) are what `ext_attn` computes on [source | uncond_e | cond_e]: the
    bank branches equal `ext_attn_views(part="bank")` on that edit's slabs and the source branch `part="source"` bit for
    bit -- except where pairs of edits take the four-bank shared-softmax launch under injection (head dim 40), which is
    held to the oracle within the attention bound.  multi_v: True / False force that form on / off (TF_ATTN_MULTI_V /
    TF_ATTN_NO_MULTI_V), None = the library's measured default.  multi_v64=True forces the form on at head dim 64
    (TF_ATTN_MULTI_V64; multi_v=True selects nothing there, multi_v=False switches it off at every head dim, and the two
    together are an error).  n_edits = 1 is `ext_attn`.  Other arguments as `ext_attn`.
    inject_mask: the injection state PER EDIT (tf_ext_attn_fwd_edits_masked): bit e set = edit e (0-based) uses the source's
    q and k, clear = its own; `inject` must then be False.  Every edit keeps the identity above with its own flag; the
    four-bank form pairs the injecting edits, neighbours or not.  None = the one shared state `inject`, today's call."""
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    E = int(n_edits)
    mask = None if inject_mask is None else _edit_mask("ext_attn_edits", inject_mask, n_edits, inject)
    if not 1 <= E <= _lib.TF_MAX_EDITS:
        raise ValueError(f"ext_attn_edits: n_edits={n_edits} (1 .. {_lib.TF_MAX_EDITS})")
    nbr = 1 + 2 * E
    BK, S, D = k.shape
    Bq = q.shape[0]
    if BK % nbr or Bq % nbr or D % heads or q.shape[1:] != k.shape[1:] or v.shape != k.shape:
        raise ValueError(f"ext_attn_edits: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} heads {heads} "
                         f"for {E} edits ({nbr} branches)")
    K, Kq, dh = BK // nbr, Bq // nbr, D // heads
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"ext_attn_edits: q/k/v must share dtype bf16 or f16, got {q.dtype},{k.dtype},{v.dtype}")

    def rows(t):
        if t.stride(-1) != 1 or t.stride(0) != S * t.stride(1):
            t = t.contiguous()
        return t
    q, k, v = rows(q), rows(k), rows(v)
    ld = q.stride(1)
    if k.stride(1) != ld or v.stride(1) != ld:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ld = D
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    if out_dtype not in (q.dtype, torch.float32):
        raise TypeError(f"ext_attn_edits: out_dtype {out_dtype} (the input dtype or float32)")
    if out is None:
        out = torch.empty(Bq, S, D, dtype=out_dtype, device=q.device)
    elif out.dtype != out_dtype or not out.is_contiguous() or out.shape != (Bq, S, D):
        raise ValueError("ext_attn_edits: `out` must be a contiguous [B*Kq,S,D] tensor of out_dtype")
    flags = _attn_flags(inject, "all", out_dtype == torch.float32, fold_scale, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    nbytes = lib.tf_ext_attn_edits_workspace_bytes(K, S, heads, dh, E, dt)
    ws = _workspace(nbytes, q.device)
    fs = S * ld
    strides = (ctypes.c_int64 * 9)(Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * S * D, S * D, ld)
    if mask is not None:
        _launch(dev, "tf_ext_attn_fwd_edits_masked", lib.tf_ext_attn_fwd_edits_masked, q.data_ptr(), k.data_ptr(),
                v.data_ptr(), out.data_ptr(), K, Kq, int(q_frame0), S, heads, dh, ld, ctypes.cast(strides, ctypes.c_void_p),
                float(scale), flags, dt, E, mask, ws.data_ptr(), ws.numel())
        return out
    _launch(dev, "tf_ext_attn_fwd_edits", lib.tf_ext_attn_fwd_edits, q.data_ptr(), k.data_ptr(), v.data_ptr(),
            out.data_ptr(), K, Kq, int(q_frame0), S, heads, dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale),
            flags, dt, E, ws.data_ptr(), ws.numel())
    return out


def ext_attn_windows_edits(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, inject: bool,
                           n_edits: int, windows, *, inject_mask: Optional[int] = None, multi_v: Optional[bool] = None,
                           multi_v64: Optional[bool] = None, no_split: Optional[bool] = None, fused: Optional[bool] = None,
                           hints: int = 0, out_dtype: Optional[torch.dtype] = None,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`ext_attn_edits` over a sliding-window keyframe bank (tf_ext_attn_fwd_windows_edits): E = n_edits prompts on one long
    video in one pass.  q, k, v [(1+2E)K,S,D] in the layout [source | uncond_1 | cond_1 | ...], `windows` one (first frame,
    frames) pair per keyframe (`bank_windows(K, radius)`).  The uncond / cond branches of every edit attend, for keyframe i, to
    the keyframes of window i only -- an injecting edit with the source's q and k -- and the source branch to its own frame,
    once.  NOT TokenFlow's computation unless every window is the whole bank (then the call is `ext_attn_edits`, bit for bit);
    n_edits = 1 is `ext_attn_windows`.  The slices of edit e are what `ext_attn_windows` computes on [source | uncond_e |
    cond_e] with edit e's injection flag, bit for bit under no_split wherever both take the same kernel form -- except where
    pairs of injecting edits take the windowed four-bank launch (multi_v=True at head dim 40, multi_v64=True at 64;
    multi_v=False switches it off; None = the library's measured rule for windowed calls), each frame of which is bit for bit
    its own four-bank `ext_attn_edits` call on the window's tensors.
    inject_mask: the injection state per edit (bit e = edit e, `inject` must then be False); None = the shared state `inject`."""
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    E = int(n_edits)
    if inject_mask is None:
        if not 1 <= E <= _lib.TF_MAX_EDITS:
            raise ValueError(f"ext_attn_windows_edits: n_edits={n_edits} (1 .. {_lib.TF_MAX_EDITS})")
        mask = (1 << E) - 1 if inject else 0
    else:
        mask = _edit_mask("ext_attn_windows_edits", inject_mask, n_edits, inject)
    nbr = 1 + 2 * E
    BK, S, D = k.shape
    if BK % nbr or D % heads or q.shape != k.shape or v.shape != k.shape:
        raise ValueError(f"ext_attn_windows_edits: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} heads {heads} "
                         f"for {E} edits ({nbr} branches)")
    K, dh = BK // nbr, D // heads
    lo, n = _windows("ext_attn_windows_edits", windows, K, K)
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"ext_attn_windows_edits: q/k/v must share dtype bf16 or f16, got {q.dtype},{k.dtype},{v.dtype}")

    def rows(t):
        if t.stride(-1) != 1 or t.stride(0) != S * t.stride(1):
            t = t.contiguous()
        return t
    q, k, v = rows(q), rows(k), rows(v)
    ld = q.stride(1)
    if k.stride(1) != ld or v.stride(1) != ld:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ld = D
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    if out_dtype not in (q.dtype, torch.float32):
        raise TypeError(f"ext_attn_windows_edits: out_dtype {out_dtype} (the input dtype or float32)")
    if out is None:
        out = torch.empty(BK, S, D, dtype=out_dtype, device=q.device)
    elif out.dtype != out_dtype or not out.is_contiguous() or out.shape != (BK, S, D):
        raise ValueError("ext_attn_windows_edits: `out` must be a contiguous [B*K,S,D] tensor of out_dtype")
    flags = _attn_flags(False, "all", out_dtype == torch.float32, False, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    ws = _workspace(lib.tf_ext_attn_edits_workspace_bytes(K, S, heads, dh, E, dt), q.device)
    fs = S * ld
    strides = (ctypes.c_int64 * 9)(K * fs, fs, K * fs, fs, K * fs, fs, K * S * D, S * D, ld)
    _launch(dev, "tf_ext_attn_fwd_windows_edits", lib.tf_ext_attn_fwd_windows_edits, q.data_ptr(), k.data_ptr(), v.data_ptr(),
            out.data_ptr(), K, K, 0, S, heads, dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale), flags, dt, E, mask,
            ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p), ws.data_ptr(), ws.numel())
    return out


def ext_attn_frame_sets_edits(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, inject: bool,
                              n_edits: int, sets, *, inject_mask: Optional[int] = None, multi_v: Optional[bool] = None,
                              multi_v64: Optional[bool] = None, no_split: Optional[bool] = None, fused: Optional[bool] = None,
                              hints: int = 0, out_dtype: Optional[torch.dtype] = None,
                              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`ext_attn_edits` over a frame-set keyframe bank (tf_ext_attn_fwd_frame_sets_edits): E = n_edits prompts on one long
    video in one pass, with anchor keyframes beside the window.  q, k, v [(1+2E)K,S,D] in the layout [source | uncond_1 |
    cond_1 | ...], `sets` one int mask per keyframe (`bank_frame_sets(K, radius, anchors)`).  The uncond / cond branches of
    every edit attend, for keyframe i, to the keyframes whose bits are set in mask i, in ascending order -- an injecting edit
    with the source's q and k -- and the source branch to its own frame, once.  NOT TokenFlow's computation unless every set is
    the whole bank (then the call is `ext_attn_edits`, bit for bit); n_edits = 1 is `ext_attn_frame_sets`, sets that are all
    contiguous ranges are `ext_attn_windows_edits`.  The slices of edit e are what `ext_attn_frame_sets` computes on [source |
    uncond_e | cond_e] with edit e's injection flag, bit for bit under no_split wherever both take the same kernel form --
    except where pairs of injecting edits take the frame-set four-bank launch (multi_v=True at head dim 40, multi_v64=True at
    64; multi_v=False switches it off; None = the library's measured rule for frame-set calls), each frame of which is bit for
    bit its own four-bank `ext_attn_edits` call on the gathered member frames.
    inject_mask: the injection state per edit (bit e = edit e, `inject` must then be False); None = the shared state `inject`."""
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    E = int(n_edits)
    if inject_mask is None:
        if not 1 <= E <= _lib.TF_MAX_EDITS:
            raise ValueError(f"ext_attn_frame_sets_edits: n_edits={n_edits} (1 .. {_lib.TF_MAX_EDITS})")
        mask = (1 << E) - 1 if inject else 0
    else:
        mask = _edit_mask("ext_attn_frame_sets_edits", inject_mask, n_edits, inject)
    nbr = 1 + 2 * E
    BK, S, D = k.shape
    if BK % nbr or D % heads or q.shape != k.shape or v.shape != k.shape:
        raise ValueError(f"ext_attn_frame_sets_edits: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} heads {heads} "
                         f"for {E} edits ({nbr} branches)")
    K, dh = BK // nbr, D // heads
    tab = _frame_sets("ext_attn_frame_sets_edits", sets, K, K)
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"ext_attn_frame_sets_edits: q/k/v must share dtype bf16 or f16, got {q.dtype},{k.dtype},{v.dtype}")

    def rows(t):
        if t.stride(-1) != 1 or t.stride(0) != S * t.stride(1):
            t = t.contiguous()
        return t
    q, k, v = rows(q), rows(k), rows(v)
    ld = q.stride(1)
    if k.stride(1) != ld or v.stride(1) != ld:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ld = D
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    if out_dtype not in (q.dtype, torch.float32):
        raise TypeError(f"ext_attn_frame_sets_edits: out_dtype {out_dtype} (the input dtype or float32)")
    if out is None:
        out = torch.empty(BK, S, D, dtype=out_dtype, device=q.device)
    elif out.dtype != out_dtype or not out.is_contiguous() or out.shape != (BK, S, D):
        raise ValueError("ext_attn_frame_sets_edits: `out` must be a contiguous [B*K,S,D] tensor of out_dtype")
    flags = _attn_flags(False, "all", out_dtype == torch.float32, False, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    ws = _workspace(lib.tf_ext_attn_edits_workspace_bytes(K, S, heads, dh, E, dt), q.device)
    fs = S * ld
    strides = (ctypes.c_int64 * 9)(K * fs, fs, K * fs, fs, K * fs, fs, K * S * D, S * D, ld)
    _launch(dev, "tf_ext_attn_fwd_frame_sets_edits", lib.tf_ext_attn_fwd_frame_sets_edits, q.data_ptr(), k.data_ptr(),
            v.data_ptr(), out.data_ptr(), K, K, 0, S, heads, dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale), flags,
            dt, E, mask, ctypes.cast(tab, ctypes.c_void_p), ws.data_ptr(), ws.numel())
    return out


def _view_base(t: torch.Tensor, b0: int, S: int, what: str):
    """(base pointer such that branch b lives at base + b*branch_stride, branch stride, frame stride, token stride)
    of a 4-D view [branches b0.., frames, S, D]."""
    if t.dim() != 4 or t.shape[2] != S or t.stride(3) != 1:
        raise ValueError(f"ext_attn_views: {what} must be a [branches, frames, S, D] view with a contiguous last dim")
    bs = t.stride(0) if t.shape[0] > 1 else 0
    return t.data_ptr() - b0 * bs * t.element_size(), bs, t.stride(1), t.stride(2)


def ext_attn_views(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int, scale: float,
                   inject: bool, part: str = "all", branch0=(0, 0, 0, 0), q_frame0: int = 0,
                   fold_scale: Optional[bool] = None, no_split: Optional[bool] = None,
                   stream: Optional[int] = None, fused: Optional[bool] = None, hints: int = 0) -> torch.Tensor:
    """`ext_attn` on strided 4-D views [branches, frames, S, D] (tf_ext_attn_fwd_strided): q, k, v are read where
    a collective left them and `out` is written where the next one sends from -- no re-layout copies.  Each view
    holds the branches `branch0[i] ..` of its tensor (q, k, v, out in that order; e.g. a bank-only call passes the
    uncond/cond slabs with branch0 = 1, and under injection the single source slab of q and k with branch0 = 0).
    Branch and frame strides are free; k and v share one token stride, q has its own, out is dense (= D).
    stream: a raw HIP stream of the tensors' device to launch on instead of torch's current one (the caller orders it
    against the others itself: sharded.py runs the source branch beside the bank exchange)."""
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    S, D = k.shape[2], k.shape[3]
    K, Kq, dh = k.shape[1], q.shape[1], D // heads
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype or D % heads:
        raise TypeError("ext_attn_views: q/k/v must share dtype bf16 or f16")
    qp, q_bs, q_fs, ld_q = _view_base(q, branch0[0], S, "q")
    kp, k_bs, k_fs, ld = _view_base(k, branch0[1], S, "k")
    vp, v_bs, v_fs, ld_v = _view_base(v, branch0[2], S, "v")
    op, o_bs, o_fs, ld_o = _view_base(out, branch0[3], S, "out")
    if ld_v != ld or ld_o != D or out.shape[1] != Kq or v.shape[1] != K:
        raise ValueError("ext_attn_views: k and v need one token stride, out a dense one; frames of v = frames of k")
    if out.dtype not in (q.dtype, torch.float32):
        raise TypeError("ext_attn_views: out dtype")
    flags = _attn_flags(inject, part, out.dtype == torch.float32, fold_scale, no_split, fused, hints)
    key = (K, S, heads, dh, dt)
    nbytes = _attn_ws_bytes.get(key)
    if nbytes is None:
        nbytes = _attn_ws_bytes[key] = lib.tf_ext_attn_workspace_bytes(K, S, heads, dh, dt)
    ws = _workspace(nbytes, q.device, stream=stream)
    strides = (ctypes.c_int64 * 9)(q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, o_fs, ld_q)
    _launch(dev, "tf_ext_attn_fwd_strided", lib.tf_ext_attn_fwd_strided, qp, kp, vp, op, K, Kq, int(q_frame0), S, heads,
            dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale), flags, dt, ws.data_ptr(), ws.numel(),
            stream=stream)
    return out


def ext_attn_windows_views(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int, scale: float,
                           inject: bool, windows, part: str = "bank", branch0=(0, 0, 0, 0), q_frame0: int = 0,
                           no_split: Optional[bool] = None, stream: Optional[int] = None, fused: Optional[bool] = None,
                           hints: int = 0) -> torch.Tensor:
    """`ext_attn_windows` on strided 4-D views [branches, frames, S, D] (tf_ext_attn_fwd_windows_part), shaped like
    `ext_attn_views`: the Kq = q.shape[1] query frames are the bank frames q_frame0 .. of k / v, `windows` holds one
    (first frame, frames) pair per QUERY frame in bank coordinates.  part "bank": only the uncond / cond branches, k and v hold
    only the slabs those read (branch0 as in `ext_attn_views`: under injection k is the source slab with branch0 = 0) -- what a
    frame-sharded rank runs over its halo-extended receive buffer; part "all": the whole windowed call.  The source part of a
    windowed pass is window-free: `ext_attn_views(..., part="source")`.  Both parts together equal `ext_attn_windows` bit for
    bit under no_split wherever the plans name the same kernel form."""
    if part not in ("bank", "all"):
        raise ValueError(f"ext_attn_windows_views: part {part!r} (\"bank\" or \"all\": the source part is window-free)")
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    S, D = k.shape[2], k.shape[3]
    K, Kq, dh = k.shape[1], q.shape[1], D // heads
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype or D % heads:
        raise TypeError("ext_attn_windows_views: q/k/v must share dtype bf16 or f16")
    lo, n = _windows("ext_attn_windows_views", windows, K, Kq, int(q_frame0))
    qp, q_bs, q_fs, ld_q = _view_base(q, branch0[0], S, "q")
    kp, k_bs, k_fs, ld = _view_base(k, branch0[1], S, "k")
    vp, v_bs, v_fs, ld_v = _view_base(v, branch0[2], S, "v")
    op, o_bs, o_fs, ld_o = _view_base(out, branch0[3], S, "out")
    if ld_v != ld or ld_o != D or out.shape[1] != Kq or v.shape[1] != K:
        raise ValueError("ext_attn_windows_views: k and v need one token stride, out a dense one; frames of v = frames of k")
    if out.dtype not in (q.dtype, torch.float32):
        raise TypeError("ext_attn_windows_views: out dtype")
    flags = _attn_flags(inject, part, out.dtype == torch.float32, False, no_split, fused, hints)
    key = (K, S, heads, dh, dt)
    nbytes = _attn_ws_bytes.get(key)
    if nbytes is None:
        nbytes = _attn_ws_bytes[key] = lib.tf_ext_attn_workspace_bytes(K, S, heads, dh, dt)
    ws = _workspace(nbytes, q.device, stream=stream)
    strides = (ctypes.c_int64 * 9)(q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, o_fs, ld_q)
    _launch(dev, "tf_ext_attn_fwd_windows_part", lib.tf_ext_attn_fwd_windows_part, qp, kp, vp, op, K, Kq, int(q_frame0), S,
            heads, dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale), flags, dt, ctypes.cast(lo, ctypes.c_void_p),
            ctypes.cast(n, ctypes.c_void_p), ws.data_ptr(), ws.numel(), stream=stream)
    return out


def ext_attn_frame_sets_views(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int, scale: float,
                              inject: bool, sets, part: str = "bank", branch0=(0, 0, 0, 0), q_frame0: int = 0,
                              no_split: Optional[bool] = None, stream: Optional[int] = None, fused: Optional[bool] = None,
                              hints: int = 0) -> torch.Tensor:
    """`ext_attn_frame_sets` on strided 4-D views [branches, frames, S, D] (tf_ext_attn_fwd_frame_sets_part), shaped like
    `ext_attn_windows_views`: the Kq = q.shape[1] query frames are the bank frames q_frame0 .. of k / v, `sets` holds one int
    mask per QUERY frame over the K = k.shape[1] <= 64 bank frames.  part "bank": only the uncond / cond branches, k and v hold
    only the slabs those read -- what a frame-sharded rank runs over its anchor-extended receive buffer; part "all": the whole
    frame-set call.  The source part of a frame-set pass is set-free: `ext_attn_views(..., part="source")`.  Both parts together
    equal `ext_attn_frame_sets` bit for bit under no_split wherever the plans name the same kernel form; sets that are all
    ranges are `ext_attn_windows_views`."""
    if part not in ("bank", "all"):
        raise ValueError(f"ext_attn_frame_sets_views: part {part!r} (\"bank\" or \"all\": the source part is set-free)")
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    S, D = k.shape[2], k.shape[3]
    K, Kq, dh = k.shape[1], q.shape[1], D // heads
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype or D % heads:
        raise TypeError("ext_attn_frame_sets_views: q/k/v must share dtype bf16 or f16")
    tab = _frame_sets("ext_attn_frame_sets_views", sets, K, Kq, int(q_frame0))
    qp, q_bs, q_fs, ld_q = _view_base(q, branch0[0], S, "q")
    kp, k_bs, k_fs, ld = _view_base(k, branch0[1], S, "k")
    vp, v_bs, v_fs, ld_v = _view_base(v, branch0[2], S, "v")
    op, o_bs, o_fs, ld_o = _view_base(out, branch0[3], S, "out")
    if ld_v != ld or ld_o != D or out.shape[1] != Kq or v.shape[1] != K:
        raise ValueError("ext_attn_frame_sets_views: k and v need one token stride, out a dense one; frames of v = frames of k")
    if out.dtype not in (q.dtype, torch.float32):
        raise TypeError("ext_attn_frame_sets_views: out dtype")
    flags = _attn_flags(inject, part, out.dtype == torch.float32, False, no_split, fused, hints)
    key = (K, S, heads, dh, dt)
    nbytes = _attn_ws_bytes.get(key)
    if nbytes is None:
        nbytes = _attn_ws_bytes[key] = lib.tf_ext_attn_workspace_bytes(K, S, heads, dh, dt)
    ws = _workspace(nbytes, q.device, stream=stream)
    strides = (ctypes.c_int64 * 9)(q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, o_fs, ld_q)
    _launch(dev, "tf_ext_attn_fwd_frame_sets_part", lib.tf_ext_attn_fwd_frame_sets_part, qp, kp, vp, op, K, Kq, int(q_frame0), S,
            heads, dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale), flags, dt, ctypes.cast(tab, ctypes.c_void_p),
            ws.data_ptr(), ws.numel(), stream=stream)
    return out


def ext_attn_edits_views(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int, scale: float,
                         n_edits: int, inject_mask: int, part: str = "all", qk_compact: bool = False,
                         branch0=(0, 0, 0, 0), q_frame0: int = 0, fold_scale: Optional[bool] = None,
                         no_split: Optional[bool] = None, fused: Optional[bool] = None, multi_v: Optional[bool] = None,
                         hints: int = 0, stream: Optional[int] = None, multi_v64: Optional[bool] = None) -> torch.Tensor:
    """The parts of `ext_attn_edits` on strided 4-D views [branches, frames, S, D] (tf_ext_attn_fwd_edits_part), in the manner
    of `ext_attn_views`: E = n_edits edits, v and out addressed as [source | uncond_1 | cond_1 | ...] (1 + 2E branches),
    inject_mask the injection state per edit.  part = "bank": the bank branches of EVERY edit (the source slabs of v and out
    are never touched), "source": the source branch alone, "all": both.
    qk_compact: q and k hold only the branches a launch reads -- slot 0 the source, then (uncond, cond) of every
    NON-injecting edit in ascending order; an injecting edit reads slot 0.  Each view holds the slots / branches
    `branch0[i] ..` of its tensor (a bank part in which no edit injects passes q and k from slot 1 with branch0 = 1).
    Every part that takes the fused small-problem kernel shares ONE launch with the others (bit-identical to the per-edit
    `ext_attn_views` calls under no_split=True; within the attention bound otherwise).  Other arguments as
    `ext_attn_views` / `ext_attn_edits`."""
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    mask = _edit_mask("ext_attn_edits_views", inject_mask, n_edits)
    E = int(n_edits)
    S, D = k.shape[2], k.shape[3]
    K, Kq, dh = k.shape[1], q.shape[1], D // heads
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype or D % heads:
        raise TypeError("ext_attn_edits_views: q/k/v must share dtype bf16 or f16")
    qp, q_bs, q_fs, ld_q = _view_base(q, branch0[0], S, "q")
    kp, k_bs, k_fs, ld = _view_base(k, branch0[1], S, "k")
    vp, v_bs, v_fs, ld_v = _view_base(v, branch0[2], S, "v")
    op, o_bs, o_fs, ld_o = _view_base(out, branch0[3], S, "out")
    if ld_v != ld or ld_o != D or out.shape[1] != Kq or v.shape[1] != K:
        raise ValueError("ext_attn_edits_views: k and v need one token stride, out a dense one; frames of v = frames of k")
    if out.dtype not in (q.dtype, torch.float32):
        raise TypeError("ext_attn_edits_views: out dtype")
    # the branches each view must hold for this part (a view of ONE branch has no branch stride to address others with)
    nbr = 1 + 2 * E
    n_non = E - bin(mask).count("1")
    n_qk = (1 + 2 * n_non) if qk_compact else nbr
    lo_vo, hi_vo = (1, nbr) if part == "bank" else (0, 1) if part == "source" else (0, nbr)
    lo_qk = 0 if (part != "bank" or mask) else 1
    hi_qk = 1 if part == "source" else (n_qk if n_non else 1)
    for t, b0, lo, hi, what in ((q, branch0[0], lo_qk, hi_qk, "q"), (k, branch0[1], lo_qk, hi_qk, "k"),
                                (v, branch0[2], lo_vo, hi_vo, "v"), (out, branch0[3], lo_vo, hi_vo, "out")):
        if b0 > lo or b0 + t.shape[0] < hi:
            raise ValueError(f"ext_attn_edits_views: {what} holds branches [{b0}, {b0 + t.shape[0]}), part '{part}' of "
                             f"{E} edits with mask {mask:#x} reads [{lo}, {hi})")
    flags = _attn_flags(False, part, out.dtype == torch.float32, fold_scale, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    ws = _workspace(lib.tf_ext_attn_edits_workspace_bytes(K, S, heads, dh, E, dt), q.device, stream=stream)
    strides = (ctypes.c_int64 * 9)(q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, o_fs, ld_q)
    _launch(dev, "tf_ext_attn_fwd_edits_part", lib.tf_ext_attn_fwd_edits_part, qp, kp, vp, op, K, Kq, int(q_frame0), S, heads,
            dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale), flags, dt, E, mask, 1 if qk_compact else 0,
            ws.data_ptr(), ws.numel(), stream=stream)
    return out


def attn_edits_part_plan(K: int, Kq: int, S: int, heads: int, dh: int, n_edits: int, inject_mask: int, part: str = "all",
                         qk_compact: bool = False, dtype: torch.dtype = torch.bfloat16,
                         out_dtype: Optional[torch.dtype] = None, fold_scale: Optional[bool] = None,
                         no_split: Optional[bool] = None, fused: Optional[bool] = None, multi_v: Optional[bool] = None,
                         hints: int = 0, multi_v64: Optional[bool] = None) -> list:
    """The launches of `ext_attn_edits_views` for dense tensors, as tokens (tf_ext_attn_edits_part_plan): those of
    `attn_edits_plan(inject_mask=...)` for the part, or -- where every part takes the fused kernel -- ONE token such as
    'fused[qw=1,kw=4,qb=1,prec=1,sets=4]' (',sets=N' for N > 2 tensor sets).  Host only: needs no GPU."""
    flags = _attn_flags(False, part, out_dtype == torch.float32, fold_scale, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    mask = _edit_mask("attn_edits_part_plan", inject_mask, n_edits)
    return _plan_tokens("tf_ext_attn_edits_part_plan", _lib.load().tf_ext_attn_edits_part_plan, K, Kq, S, heads, dh,
                        int(n_edits), mask, 1 if qk_compact else 0, flags, _DT[dtype])


def _edits_table_views(what: str, sym: str, table, q, k, v, out, heads, scale, n_edits, inject_mask, part, qk_compact, branch0,
                       q_frame0, no_split, fused, multi_v, multi_v64, hints, stream):
    """`ext_attn_windows_edits_views` / `ext_attn_frame_sets_edits_views`: the checks of `ext_attn_edits_views` for part "bank"
    or "all", then the entry point `sym` with the table `table(K, Kq)` (a tuple of ctypes arrays) behind qk_compact."""
    if part not in ("bank", "all"):
        raise ValueError(f"{what}: part {part!r} (\"bank\" or \"all\": the source part is table-free, "
                         "`ext_attn_edits_views(..., part=\"source\")`)")
    if part == "all" and qk_compact:
        raise ValueError(f"{what}: qk_compact with part \"all\" (the whole call reads dense q / k)")
    dev = _need_gpu(q, k, v, out)
    lib = _lib.load()
    mask = _edit_mask(what, inject_mask, n_edits)
    E = int(n_edits)
    S, D = k.shape[2], k.shape[3]
    K, Kq, dh = k.shape[1], q.shape[1], D // heads
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or k.dtype != q.dtype or v.dtype != q.dtype or D % heads:
        raise TypeError(f"{what}: q/k/v must share dtype bf16 or f16")
    tab = table(K, Kq)
    qp, q_bs, q_fs, ld_q = _view_base(q, branch0[0], S, "q")
    kp, k_bs, k_fs, ld = _view_base(k, branch0[1], S, "k")
    vp, v_bs, v_fs, ld_v = _view_base(v, branch0[2], S, "v")
    op, o_bs, o_fs, ld_o = _view_base(out, branch0[3], S, "out")
    if ld_v != ld or ld_o != D or out.shape[1] != Kq or v.shape[1] != K:
        raise ValueError(f"{what}: k and v need one token stride, out a dense one; frames of v = frames of k")
    if out.dtype not in (q.dtype, torch.float32):
        raise TypeError(f"{what}: out dtype")
    # the branches each view must hold for this part, as in `ext_attn_edits_views`
    nbr = 1 + 2 * E
    n_non = E - bin(mask).count("1")
    n_qk = (1 + 2 * n_non) if qk_compact else nbr
    lo_vo, hi_vo = (1, nbr) if part == "bank" else (0, nbr)
    lo_qk = 0 if (part != "bank" or mask) else 1
    hi_qk = n_qk if n_non else 1
    for t, b0, lo, hi, name in ((q, branch0[0], lo_qk, hi_qk, "q"), (k, branch0[1], lo_qk, hi_qk, "k"),
                                (v, branch0[2], lo_vo, hi_vo, "v"), (out, branch0[3], lo_vo, hi_vo, "out")):
        if b0 > lo or b0 + t.shape[0] < hi:
            raise ValueError(f"{what}: {name} holds branches [{b0}, {b0 + t.shape[0]}), part '{part}' of {E} edits with mask "
                             f"{mask:#x} reads [{lo}, {hi})")
    flags = _attn_flags(False, part, out.dtype == torch.float32, False, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    ws = _workspace(lib.tf_ext_attn_edits_workspace_bytes(K, S, heads, dh, E, dt), q.device, stream=stream)
    strides = (ctypes.c_int64 * 9)(q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, o_fs, ld_q)
    _launch(dev, sym, getattr(lib, sym), qp, kp, vp, op, K, Kq, int(q_frame0), S, heads, dh, ld,
            ctypes.cast(strides, ctypes.c_void_p), float(scale), flags, dt, E, mask, 1 if qk_compact else 0,
            *[ctypes.cast(t, ctypes.c_void_p) for t in tab], ws.data_ptr(), ws.numel(), stream=stream)
    return out


def ext_attn_windows_edits_views(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int, scale: float,
                                 n_edits: int, inject_mask: int, windows, part: str = "bank", qk_compact: bool = False,
                                 branch0=(0, 0, 0, 0), q_frame0: int = 0, no_split: Optional[bool] = None,
                                 fused: Optional[bool] = None, multi_v: Optional[bool] = None, hints: int = 0,
                                 stream: Optional[int] = None, multi_v64: Optional[bool] = None) -> torch.Tensor:
    """`ext_attn_windows_edits` on strided 4-D views [branches, frames, S, D] (tf_ext_attn_fwd_windows_edits_part): the views,
    n_edits, inject_mask, qk_compact and branch0 of `ext_attn_edits_views`, the `windows` and q_frame0 of
    `ext_attn_windows_views` (one (first frame, frames) pair per QUERY frame in bank coordinates; all edits share them).
    part "bank": the bank branches of EVERY edit over the one table -- where they all take the fused small-problem kernel, in
    ONE launch ('fused[..,sets=E,win]'), bit-identical under no_split=True to the E `ext_attn_windows_views` calls; part "all":
    `ext_attn_windows_edits` on views.  The source part of a windowed pass is window-free:
    `ext_attn_edits_views(..., part="source")`."""
    what = "ext_attn_windows_edits_views"
    return _edits_table_views(what, "tf_ext_attn_fwd_windows_edits_part", lambda K, Kq: _windows(what, windows, K, Kq, int(q_frame0)),
                              q, k, v, out, heads, scale, n_edits, inject_mask, part, qk_compact, branch0, q_frame0, no_split,
                              fused, multi_v, multi_v64, hints, stream)


def ext_attn_frame_sets_edits_views(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int,
                                    scale: float, n_edits: int, inject_mask: int, sets, part: str = "bank",
                                    qk_compact: bool = False, branch0=(0, 0, 0, 0), q_frame0: int = 0,
                                    no_split: Optional[bool] = None, fused: Optional[bool] = None,
                                    multi_v: Optional[bool] = None, hints: int = 0, stream: Optional[int] = None,
                                    multi_v64: Optional[bool] = None) -> torch.Tensor:
    """`ext_attn_frame_sets_edits` on strided 4-D views (tf_ext_attn_fwd_frame_sets_edits_part): as
    `ext_attn_windows_edits_views`, with one int mask per QUERY frame over the K = k.shape[1] <= 64 bank frames; the joint
    fused launch is 'fused[..,sets=E,set]'.  Sets that are all ranges are `ext_attn_windows_edits_views`."""
    what = "ext_attn_frame_sets_edits_views"
    return _edits_table_views(what, "tf_ext_attn_fwd_frame_sets_edits_part",
                              lambda K, Kq: (_frame_sets(what, sets, K, Kq, int(q_frame0)),), q, k, v, out, heads, scale, n_edits,
                              inject_mask, part, qk_compact, branch0, q_frame0, no_split, fused, multi_v, multi_v64, hints, stream)


def attn_windows_edits_part_plan(K: int, Kq: int, q_frame0: int, windows, S: int, heads: int, dh: int, n_edits: int,
                                 inject_mask: int, part: str = "bank", qk_compact: bool = False,
                                 dtype: torch.dtype = torch.bfloat16, out_dtype: Optional[torch.dtype] = None,
                                 no_split: Optional[bool] = None, fused: Optional[bool] = None, multi_v: Optional[bool] = None,
                                 multi_v64: Optional[bool] = None, hints: int = 0) -> list:
    """The launches `ext_attn_windows_edits_views` makes for dense tensors, as tokens (tf_ext_attn_windows_edits_part_plan):
    those of `attn_windows_edits_plan` without the source launches, or -- where every edit's bank part takes the fused kernel --
    ONE token such as 'fused[qw=1,kw=4,qb=1,prec=1,sets=2,win]'.  Host only: needs no GPU."""
    if part not in ("bank", "all"):
        raise ValueError(f"attn_windows_edits_part_plan: part {part!r} (\"bank\" or \"all\": the source part is window-free)")
    lo, n = _windows("attn_windows_edits_part_plan", windows, K, Kq, int(q_frame0))
    mask = _edit_mask("attn_windows_edits_part_plan", inject_mask, n_edits)
    flags = _attn_flags(False, part, out_dtype == torch.float32, False, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    return _plan_tokens("tf_ext_attn_windows_edits_part_plan", _lib.load().tf_ext_attn_windows_edits_part_plan, K, Kq,
                        int(q_frame0), S, heads, dh, int(n_edits), mask, 1 if qk_compact else 0, flags, _DT[dtype],
                        ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p))


def attn_frame_sets_edits_part_plan(K: int, Kq: int, q_frame0: int, sets, S: int, heads: int, dh: int, n_edits: int,
                                    inject_mask: int, part: str = "bank", qk_compact: bool = False,
                                    dtype: torch.dtype = torch.bfloat16, out_dtype: Optional[torch.dtype] = None,
                                    no_split: Optional[bool] = None, fused: Optional[bool] = None,
                                    multi_v: Optional[bool] = None, multi_v64: Optional[bool] = None, hints: int = 0) -> list:
    """The launches `ext_attn_frame_sets_edits_views` makes for dense tensors, as tokens
    (tf_ext_attn_frame_sets_edits_part_plan); the joint fused launch is 'fused[..,sets=E,set]'.  Host only: needs no GPU."""
    if part not in ("bank", "all"):
        raise ValueError(f"attn_frame_sets_edits_part_plan: part {part!r} (\"bank\" or \"all\": the source part is set-free)")
    tab = _frame_sets("attn_frame_sets_edits_part_plan", sets, K, Kq, int(q_frame0))
    mask = _edit_mask("attn_frame_sets_edits_part_plan", inject_mask, n_edits)
    flags = _attn_flags(False, part, out_dtype == torch.float32, False, no_split, fused, hints) | _multi_v_bits(multi_v, multi_v64)
    return _plan_tokens("tf_ext_attn_frame_sets_edits_part_plan", _lib.load().tf_ext_attn_frame_sets_edits_part_plan, K, Kq,
                        int(q_frame0), S, heads, dh, int(n_edits), mask, 1 if qk_compact else 0, flags, _DT[dtype],
                        ctypes.cast(tab, ctypes.c_void_p))


def _run_flags(inject: bool, bank_only: bool, out_f32: bool, fold_scale: Optional[bool], no_split: bool, hints: int) -> int:
    """The TF_ATTN_* bit mask of a run / merge call (the module default TOKENFLOW_ATTN_NO_SPLIT does not apply: a run set is
    a split form by construction; no_split=True only keeps a run from splitting itself further)."""
    return ((1 if inject else 0) | (_lib.TF_ATTN_FOLD_SCALE if (FOLD_SCALE if fold_scale is None else fold_scale) else 0) |
            (_lib.TF_ATTN_OUT_F32 if out_f32 else 0) | (_lib.TF_ATTN_BANK_ONLY if bank_only else 0) |
            (_lib.TF_ATTN_NO_SPLIT if no_split else 0) | int(hints))


def ext_attn_runs_views(q: torch.Tensor, kv_runs: Sequence, out: torch.Tensor, heads: int, scale: float, inject: bool,
                        runs: Sequence, K: int, branch0=(0, 0), q_frame0: int = 0, streams: Optional[Sequence] = None,
                        fold_scale: Optional[bool] = None, no_split: bool = False, hints: int = 0,
                        order: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Extended attention over a K-frame bank held in pieces (tf_ext_attn_run + tf_ext_attn_runs_merge).
    runs: [(f0, n), ...] partitions [0, K); run 0 holds the query frames q_frame0 .. +Kq-1 and computes their source
    branch, the others compute bank branches only.  kv_runs[r] = (k_view, v_view, k_branch0, v_branch0): strided 4-D
    views [branches, n, S, D] of run r's frames only, wherever they live (the caller's own projection output, the
    receive buffer of a collective), holding the branches k_branch0.. / v_branch0.. as in `ext_attn_views`.
    q, out: views [branches, Kq, S, D] with first branches branch0 = (q, out); out dense in its last two dims.
    streams: None, or one entry per run -- a torch.cuda.Stream to issue that run on (None = the current stream); the
    runs are forked behind the current stream and joined in front of the merge, which runs on the current stream.
    order: the order in which the run calls are issued (default 0, 1, ...); the result does not depend on it.
    ONE workspace serves the whole run set."""
    dev = _need_gpu(q, out, *[t for kv in kv_runs for t in kv[:2]])
    lib = _lib.load()
    S, D = q.shape[2], q.shape[3]
    Kq, dh, n_runs = q.shape[1], D // heads, len(runs)
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or D % heads or len(kv_runs) != n_runs:
        raise TypeError("ext_attn_runs_views: q/k/v must share dtype bf16 or f16; one (k, v) pair of views per run")
    if sorted(f for f0, n in runs for f in range(f0, f0 + n)) != list(range(K)) or any(n < 1 for _, n in runs):
        raise ValueError(f"ext_attn_runs_views: runs {list(runs)} do not partition the {K}-frame bank")
    if out.dtype not in (q.dtype, torch.float32) or out.shape[1] != Kq:
        raise TypeError("ext_attn_runs_views: out dtype / frames")
    qp, q_bs, q_fs, ld_q = _view_base(q, branch0[0], S, "q")
    op, o_bs, o_fs, ld_o = _view_base(out, branch0[1], S, "out")
    if ld_o != D:
        raise ValueError("ext_attn_runs_views: out needs a dense token stride")
    out_f32 = out.dtype == torch.float32
    nbytes = lib.tf_ext_attn_runs_workspace_bytes(K, Kq, S, heads, dh, n_runs, dt)
    ws = _workspace(nbytes, q.device, tag="attn_runs")     # one per run SET: keyed by the current stream, not by the runs' streams
    cur = torch.cuda.current_stream(dev)
    fork = None
    used = []
    for r in (range(n_runs) if order is None else order):
        f0, n = runs[r]
        kv, vv, kb0, vb0 = kv_runs[r]
        if kv.dtype != q.dtype or vv.dtype != q.dtype or kv.shape[1] != n or vv.shape[1] != n:
            raise TypeError("ext_attn_runs_views: a run's k / v views hold that run's frames in the dtype of q")
        kp, k_bs, k_fs, ld = _view_base(kv, kb0, S, "k")
        vp, v_bs, v_fs, ld_v = _view_base(vv, vb0, S, "v")
        if ld_v != ld:
            raise ValueError("ext_attn_runs_views: k and v of a run need one token stride")
        es = kv.element_size()
        strides = (ctypes.c_int64 * 9)(q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, o_fs, ld_q)
        flags = _run_flags(inject, r != 0, out_f32, fold_scale, no_split, hints)
        st = streams[r] if streams is not None else None
        if st is not None:
            if fork is None:
                fork = torch.cuda.Event()
                fork.record(cur)
            st.wait_event(fork)
            used.append(st)
        # frame f of the bank at base + f * frame stride: the views start at the run's first frame
        _launch(dev, "tf_ext_attn_run", lib.tf_ext_attn_run, qp, kp - f0 * k_fs * es, vp - f0 * v_fs * es, op, K, Kq,
                int(q_frame0), f0, n, r, n_runs, S, heads, dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale),
                flags, dt, ws.data_ptr(), ws.numel(), stream=None if st is None else st.cuda_stream)
    for st in used:
        ev = torch.cuda.Event()
        ev.record(st)
        cur.wait_event(ev)
    _launch(dev, "tf_ext_attn_runs_merge", lib.tf_ext_attn_runs_merge, op, K, Kq, S, heads, dh, n_runs, o_bs, o_fs,
            _run_flags(inject, False, out_f32, fold_scale, no_split, hints), dt, ws.data_ptr(), ws.numel())
    return out


def ext_attn_runs(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, inject: bool,
                  runs: Sequence, q_frame0: int = 0, out: Optional[torch.Tensor] = None,
                  out_dtype: Optional[torch.dtype] = None, streams: Optional[Sequence] = None,
                  fold_scale: Optional[bool] = None, no_split: bool = False, hints: int = 0,
                  order: Optional[Sequence[int]] = None) -> torch.Tensor:
    """`ext_attn` computed run by run over the bank: k, v [3K,S,D], q [3Kq,S,D] (the queries of keyframes q_frame0 ..),
    runs = [(f0, n), ...] a partition of the K bank frames whose FIRST entry contains the query frames and computes
    the source branch.  Returns [3Kq,S,D] (fp32 with out_dtype=torch.float32).  The result is a function of the runs
    alone (not of `order` or `streams`); it equals the oracle within the attention bound, not `ext_attn` bit for bit:
    the merge re-associates fp32 sums as the split form's does."""
    _need_gpu(q, k, v, out)
    B, S, D = k.shape
    Bq = q.shape[0]
    if B % 3 or Bq % 3 or D % heads or q.shape[1:] != k.shape[1:] or v.shape != k.shape:
        raise ValueError(f"ext_attn_runs: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} heads {heads}")
    K, Kq = B // 3, Bq // 3
    if q.dtype not in (torch.bfloat16, torch.float16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"ext_attn_runs: q/k/v must share dtype bf16 or f16, got {q.dtype},{k.dtype},{v.dtype}")
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    if out_dtype not in (q.dtype, torch.float32):
        raise TypeError(f"ext_attn_runs: out_dtype {out_dtype} (the input dtype or float32)")
    if out is None:
        out = torch.empty(Bq, S, D, dtype=out_dtype, device=q.device)
    elif out.dtype != out_dtype or not out.is_contiguous() or out.shape != (Bq, S, D):
        raise ValueError("ext_attn_runs: `out` must be a contiguous [3Kq,S,D] tensor of out_dtype")
    k4, v4 = k.view(3, K, S, D), v.view(3, K, S, D)
    kv_runs = [(k4[:, f0:f0 + n], v4[:, f0:f0 + n], 0, 0) for f0, n in runs]
    ext_attn_runs_views(q.view(3, Kq, S, D), kv_runs, out.view(3, Kq, S, D), heads, scale, inject, runs, K,
                        q_frame0=q_frame0, streams=streams, fold_scale=fold_scale, no_split=no_split, hints=hints,
                        order=order)
    return out


def _run_multi_v_bit(multi_v: bool) -> int:
    """TF_ATTN_RUN_MULTI_V of the multi-edit run calls (the same in every call of a run set, the merge included)."""
    return _lib.TF_ATTN_RUN_MULTI_V if multi_v else 0


def attn_run_edits_plan(K: int, Kq: int, run_n: int, n_runs: int, S: int, heads: int, dh: int, n_edits: int, inject_mask: int,
                        dtype: torch.dtype = torch.bfloat16, bank_only: bool = False, out_dtype: Optional[torch.dtype] = None,
                        fold_scale: Optional[bool] = None, no_split: bool = False, hints: int = 0,
                        multi_v: bool = False) -> list:
    """The launches of ONE run call of `ext_attn_runs_edits` over run_n of the bank's K frames, followed by the merge, as
    tokens (tf_ext_attn_run_edits_plan): 'vt_pack', per edit -- the injecting ones first, then the others, ascending -- the
    ',run>' tokens of its own bank-only `attn_run_plan`, the source token unless bank_only, 'merge[runs=N,edits=E]'.
    multi_v (TF_ATTN_RUN_MULTI_V, head dims 40 and 64): each pair of injecting edits is ONE ',MV4,...,run>' token in the place
    of its first edit's tokens.  Host only."""
    flags = _run_flags(False, bank_only, out_dtype == torch.float32, fold_scale, no_split, hints) | _run_multi_v_bit(multi_v)
    mask = _edit_mask("attn_run_edits_plan", inject_mask, n_edits)
    return _plan_tokens("tf_ext_attn_run_edits_plan", _lib.load().tf_ext_attn_run_edits_plan, K, Kq, run_n, n_runs, S, heads,
                        dh, int(n_edits), mask, flags, _DT[dtype])


def ext_attn_runs_edits_views(q: torch.Tensor, kv_runs: Sequence, out: torch.Tensor, heads: int, scale: float, n_edits: int,
                              inject_mask: int, runs: Sequence, K: int, branch0=(0, 0), q_frame0: int = 0,
                              q_compact: bool = False, streams: Optional[Sequence] = None,
                              fold_scale: Optional[bool] = None, no_split: bool = False, hints: int = 0,
                              order: Optional[Sequence[int]] = None, multi_v: bool = False) -> torch.Tensor:
    """`ext_attn_runs_views` for a multi-edit batch (tf_ext_attn_run_edits + tf_ext_attn_runs_merge_edits): E = n_edits
    edits, v and out addressed as [source | uncond_1 | cond_1 | ...] (1 + 2E branches), inject_mask the injection state per
    edit.  kv_runs[r] = (k_view, v_view, k_branch0, v_branch0, k_compact): as in `ext_attn_runs_views`, and k_compact says
    that run's k holds only the slots a launch reads (slot 0 the source, then (uncond, cond) of every NON-injecting edit,
    ascending: the layout of `ext_attn_edits_views(qk_compact=True)`) -- a rank's local run reads its own dense k, its remote
    runs the compact k of a receive buffer, all against the same q (q_compact: q is compact too).  Run 0 computes the source
    branch; the others never touch the source slabs of v and out.  For every edit the result equals, bit for bit,
    `ext_attn_runs_views` on [source | uncond_e | cond_e] with the same runs and that edit's flag.  ONE workspace per set.
    multi_v (TF_ATTN_RUN_MULTI_V; head dims 40 and 64, fp32 score scaling, a no-op elsewhere): the injecting edits are paired
    ascending and each pair is ONE four-bank launch per run -- one softmax for both edits.  A paired edit equals the oracle
    within the attention bound instead of its single-edit run set bit for bit; every other edit and the source keep their
    bits."""
    dev = _need_gpu(q, out, *[t for kv in kv_runs for t in kv[:2]])
    lib = _lib.load()
    mask = _edit_mask("ext_attn_runs_edits_views", inject_mask, n_edits)
    E = int(n_edits)
    S, D = q.shape[2], q.shape[3]
    Kq, dh, n_runs = q.shape[1], D // heads, len(runs)
    dt = _DT.get(q.dtype)
    if dt is None or dt == _lib.TF_F32 or D % heads or len(kv_runs) != n_runs:
        raise TypeError("ext_attn_runs_edits_views: q/k/v must share dtype bf16 or f16; one (k, v, ...) entry per run")
    if sorted(f for f0, n in runs for f in range(f0, f0 + n)) != list(range(K)) or any(n < 1 for _, n in runs):
        raise ValueError(f"ext_attn_runs_edits_views: runs {list(runs)} do not partition the {K}-frame bank")
    if out.dtype not in (q.dtype, torch.float32) or out.shape[1] != Kq:
        raise TypeError("ext_attn_runs_edits_views: out dtype / frames")
    qp, q_bs, q_fs, ld_q = _view_base(q, branch0[0], S, "q")
    op, o_bs, o_fs, ld_o = _view_base(out, branch0[1], S, "out")
    if ld_o != D:
        raise ValueError("ext_attn_runs_edits_views: out needs a dense token stride")
    out_f32 = out.dtype == torch.float32
    nbytes = lib.tf_ext_attn_runs_edits_workspace_bytes(K, Kq, S, heads, dh, n_runs, E, dt)
    ws = _workspace(nbytes, q.device, tag="attn_runs")     # one per run SET: keyed by the current stream, not by the runs' streams
    cur = torch.cuda.current_stream(dev)
    fork = None
    used = []
    for r in (range(n_runs) if order is None else order):
        f0, n = runs[r]
        kv, vv, kb0, vb0, k_compact = kv_runs[r]
        if kv.dtype != q.dtype or vv.dtype != q.dtype or kv.shape[1] != n or vv.shape[1] != n:
            raise TypeError("ext_attn_runs_edits_views: a run's k / v views hold that run's frames in the dtype of q")
        kp, k_bs, k_fs, ld = _view_base(kv, kb0, S, "k")
        vp, v_bs, v_fs, ld_v = _view_base(vv, vb0, S, "v")
        if ld_v != ld:
            raise ValueError("ext_attn_runs_edits_views: k and v of a run need one token stride")
        es = kv.element_size()
        strides = (ctypes.c_int64 * 9)(q_bs, q_fs, k_bs, k_fs, v_bs, v_fs, o_bs, o_fs, ld_q)
        flags = _run_flags(False, r != 0, out_f32, fold_scale, no_split, hints) | _run_multi_v_bit(multi_v)
        st = streams[r] if streams is not None else None
        if st is not None:
            if fork is None:
                fork = torch.cuda.Event()
                fork.record(cur)
            st.wait_event(fork)
            used.append(st)
        _launch(dev, "tf_ext_attn_run_edits", lib.tf_ext_attn_run_edits, qp, kp - f0 * k_fs * es, vp - f0 * v_fs * es, op, K, Kq,
                int(q_frame0), f0, n, r, n_runs, S, heads, dh, ld, ctypes.cast(strides, ctypes.c_void_p), float(scale),
                flags, dt, E, mask, (1 if q_compact else 0) | (2 if k_compact else 0), ws.data_ptr(), ws.numel(),
                stream=None if st is None else st.cuda_stream)
    for st in used:
        ev = torch.cuda.Event()
        ev.record(st)
        cur.wait_event(ev)
    _launch(dev, "tf_ext_attn_runs_merge_edits", lib.tf_ext_attn_runs_merge_edits, op, K, Kq, S, heads, dh, n_runs, E, mask,
            o_bs, o_fs, _run_flags(False, False, out_f32, fold_scale, no_split, hints) | _run_multi_v_bit(multi_v), dt,
            ws.data_ptr(), ws.numel())
    return out


def ext_attn_runs_edits(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, n_edits: int,
                        inject_mask: int, runs: Sequence, q_frame0: int = 0, out: Optional[torch.Tensor] = None,
                        out_dtype: Optional[torch.dtype] = None, streams: Optional[Sequence] = None,
                        fold_scale: Optional[bool] = None, no_split: bool = False, hints: int = 0,
                        order: Optional[Sequence[int]] = None, k_compact: bool = False,
                        multi_v: bool = False) -> torch.Tensor:
    """`ext_attn_edits(inject_mask=...)` computed run by run over the bank: k, v [B*K,S,D], q [B*Kq,S,D], B = 1 + 2E, runs as
    in `ext_attn_runs`.  Returns [B*Kq,S,D] (fp32 with out_dtype=torch.float32).  For every edit e the slices (source,
    uncond_e, cond_e) equal `ext_attn_runs` on [source | uncond_e | cond_e] with the same runs and that edit's flag, bit for
    bit; the result is a function of the runs alone and equals the oracle within the attention bound -- not
    `ext_attn_edits` bit for bit.  n_edits = 1 is `ext_attn_runs`.
    k_compact: every run but the first reads k from a compact copy -- the source slot (where an edit injects), then
    (uncond, cond) of every non-injecting edit -- as a rank's remote runs read a receive buffer; the same bits.
    multi_v: pairs of injecting edits share one four-bank launch per run (`ext_attn_runs_edits_views`); the paired edits are
    then held to the oracle bound, not to `ext_attn_runs` bit for bit."""
    _need_gpu(q, k, v, out)
    mask = _edit_mask("ext_attn_runs_edits", inject_mask, n_edits)
    E = int(n_edits)
    nbr = 1 + 2 * E
    BK, S, D = k.shape
    Bq = q.shape[0]
    if BK % nbr or Bq % nbr or D % heads or q.shape[1:] != k.shape[1:] or v.shape != k.shape:
        raise ValueError(f"ext_attn_runs_edits: bad shapes q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} heads {heads} "
                         f"for {E} edits ({nbr} branches)")
    K, Kq = BK // nbr, Bq // nbr
    if q.dtype not in (torch.bfloat16, torch.float16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"ext_attn_runs_edits: q/k/v must share dtype bf16 or f16, got {q.dtype},{k.dtype},{v.dtype}")
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else q.dtype
    if out_dtype not in (q.dtype, torch.float32):
        raise TypeError(f"ext_attn_runs_edits: out_dtype {out_dtype} (the input dtype or float32)")
    if out is None:
        out = torch.empty(Bq, S, D, dtype=out_dtype, device=q.device)
    elif out.dtype != out_dtype or not out.is_contiguous() or out.shape != (Bq, S, D):
        raise ValueError("ext_attn_runs_edits: `out` must be a contiguous [B*Kq,S,D] tensor of out_dtype")
    k4, v4 = k.view(nbr, K, S, D), v.view(nbr, K, S, D)
    kv_runs = [(k4[:, f0:f0 + n], v4[:, f0:f0 + n], 0, 0, False) for f0, n in runs]
    if k_compact:
        slots = ([0] if mask else []) + [b for e in range(E) if not (mask >> e) & 1 for b in (1 + 2 * e, 2 + 2 * e)]
        kc = k4[slots].contiguous()   # (a compact k in which no edit injects starts at slot 1)
        kv_runs[1:] = [(kc[:, f0:f0 + n], v4[:, f0:f0 + n], 0 if mask else 1, 0, True) for f0, n in runs[1:]]
    ext_attn_runs_edits_views(q.view(nbr, Kq, S, D), kv_runs, out.view(nbr, Kq, S, D), heads, scale, E, mask, runs, K,
                              q_frame0=q_frame0, streams=streams, fold_scale=fold_scale, no_split=no_split, hints=hints,
                              order=order, multi_v=multi_v)
    return out


def head_pack(slabs: Sequence[torch.Tensor], W: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """slabs: ns <= 6 * TF_MAX_EDITS tensors [Kl, S, D] (frame stride free, rows dense-strided, same dtype) -> the all-to-all send
    buffer [W, Kl, ns, S, D // W]: head group w of every slab, frame-major (tf_head_pack, one launch)."""
    dev = _need_gpu(*slabs)
    lib = _lib.load()
    Kl, S, D = slabs[0].shape
    ns, hd = len(slabs), D // W
    ld = slabs[0].stride(1)
    if D % W or any(t.shape != (Kl, S, D) or t.stride(2) != 1 or t.stride(1) != ld or t.dtype != slabs[0].dtype
                    for t in slabs):
        raise ValueError("head_pack: slabs must be [Kl, S, D] views sharing dtype and token stride, D divisible by W")
    if out is None:
        out = torch.empty(W, Kl, ns, S, hd, dtype=slabs[0].dtype, device=slabs[0].device)
    send = out
    ptrs = (ctypes.c_void_p * ns)(*[t.data_ptr() for t in slabs])
    fs = (ctypes.c_int64 * ns)(*[t.stride(0) for t in slabs])
    _launch(dev, "tf_head_pack", lib.tf_head_pack, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(fs, ctypes.c_void_p),
            ns, send.data_ptr(), W, Kl, S, hd, ld, slabs[0].element_size())
    return send


def window_halo_pack(slabs: Sequence[torch.Tensor], segments, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """slabs: ns <= 6 tensors [Kl, S, D] (frame stride free, one token stride, one 16-bit dtype); segments: one (first local
    frame, frames) pair per peer, in rank order -> the send buffer [rows, ns, S, D] of ONE row all-to-all, rows = the segments'
    frames one after the other, frame-major [frame][slab][S][D] (tf_window_halo_pack, one launch).  A frame in several segments
    is written to each; an empty segment contributes nothing.  The packing of a windowed frame shard
    (`sharded.window_halo_plan(...).send`)."""
    dev = _need_gpu(*slabs)
    lib = _lib.load()
    Kl, S, D = slabs[0].shape
    ns = len(slabs)
    ld = slabs[0].stride(1)
    dt = _DT.get(slabs[0].dtype)
    if any(t.shape != (Kl, S, D) or t.stride(2) != 1 or t.stride(1) != ld or t.dtype != slabs[0].dtype for t in slabs):
        raise ValueError("window_halo_pack: slabs must be [Kl, S, D] views sharing dtype and token stride")
    seg = [(int(f0), int(n)) for f0, n in segments]
    if not seg or any(n < 0 or f0 < 0 or f0 + n > Kl for f0, n in seg):
        raise ValueError(f"window_halo_pack: segments {seg} (runs of the {Kl} local frames, one per peer)")
    rows = sum(n for _, n in seg)
    if out is None:
        out = torch.empty(rows, ns, S, D, dtype=slabs[0].dtype, device=slabs[0].device)
    elif out.shape != (rows, ns, S, D) or not out.is_contiguous() or out.dtype != slabs[0].dtype:
        raise ValueError(f"window_halo_pack: `out` must be a contiguous [{rows}, {ns}, {S}, {D}] tensor of the slabs' dtype")
    if rows == 0:      # nobody reads this rank's frames: nothing to launch
        return out
    ptrs = (ctypes.c_void_p * ns)(*[t.data_ptr() for t in slabs])
    fs = (ctypes.c_int64 * ns)(*[t.stride(0) for t in slabs])
    f0s, cnt = (ctypes.c_int * len(seg))(*[f0 for f0, _ in seg]), (ctypes.c_int * len(seg))(*[n for _, n in seg])
    _launch(dev, "tf_window_halo_pack", lib.tf_window_halo_pack, ctypes.cast(ptrs, ctypes.c_void_p),
            ctypes.cast(fs, ctypes.c_void_p), ns, out.data_ptr(), len(seg), ctypes.cast(f0s, ctypes.c_void_p),
            ctypes.cast(cnt, ctypes.c_void_p), Kl, S, D, ld, -1 if dt is None else dt)
    return out


def frame_set_halo_pack(slabs: Sequence[torch.Tensor], masks, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`window_halo_pack` where a peer reads a SET of the local frames: masks = one int mask over the Kl <= 64 local frames per
    peer, in rank order -> the send buffer [rows, ns, S, D] of ONE row all-to-all, rows = the members of mask 0 in ascending
    order, then those of mask 1, ... (tf_frame_set_halo_pack, one launch).  A frame in several masks is written to each; an empty
    mask contributes nothing.  The packing of an anchored windowed frame shard (`sharded.frame_set_halo_plan(...).send`)."""
    dev = _need_gpu(*slabs)
    lib = _lib.load()
    Kl, S, D = slabs[0].shape
    ns = len(slabs)
    ld = slabs[0].stride(1)
    dt = _DT.get(slabs[0].dtype)
    if any(t.shape != (Kl, S, D) or t.stride(2) != 1 or t.stride(1) != ld or t.dtype != slabs[0].dtype for t in slabs):
        raise ValueError("frame_set_halo_pack: slabs must be [Kl, S, D] views sharing dtype and token stride")
    ms = [int(m) for m in masks]
    if not ms or Kl > 64 or any(m < 0 or m >> Kl for m in ms):
        raise ValueError(f"frame_set_halo_pack: masks {[hex(m) for m in ms]} (bits below the {Kl} <= 64 local frames, one mask "
                         "per peer)")
    rows = sum(bin(m).count("1") for m in ms)
    if out is None:
        out = torch.empty(rows, ns, S, D, dtype=slabs[0].dtype, device=slabs[0].device)
    elif out.shape != (rows, ns, S, D) or not out.is_contiguous() or out.dtype != slabs[0].dtype:
        raise ValueError(f"frame_set_halo_pack: `out` must be a contiguous [{rows}, {ns}, {S}, {D}] tensor of the slabs' dtype")
    if rows == 0:      # nobody reads this rank's frames: nothing to launch
        return out
    ptrs = (ctypes.c_void_p * ns)(*[t.data_ptr() for t in slabs])
    fs = (ctypes.c_int64 * ns)(*[t.stride(0) for t in slabs])
    tab = (ctypes.c_uint64 * len(ms))(*ms)
    _launch(dev, "tf_frame_set_halo_pack", lib.tf_frame_set_halo_pack, ctypes.cast(ptrs, ctypes.c_void_p),
            ctypes.cast(fs, ctypes.c_void_p), ns, out.data_ptr(), len(ms), ctypes.cast(tab, ctypes.c_void_p), Kl, S, D, ld,
            -1 if dt is None else dt)
    return out


def edit_halo_pack(slabs: Sequence[torch.Tensor], masks, q_slabs: Sequence[torch.Tensor] = (),
                   out: Optional[torch.Tensor] = None, q_out: Optional[torch.Tensor] = None):
    """`frame_set_halo_pack` for a MULTI-EDIT batch (tf_edit_halo_pack, one launch): up to 4 * TF_MAX_EDITS slabs [Kl, S, D] (the
    compact k slots and two value slabs per edit) -> the send buffer [rows, ns, S, D], rows = the members of every peer's mask
    in ascending order; a plain window's ranges are contiguous masks.  q_slabs: up to 1 + 2 * TF_MAX_EDITS [Kl, S, D] views
    (sharing one token stride) copied by extra workgroups of the SAME launch into the dense staging tensor [nq, Kl, S, D] -- the
    compact q of a mixed injection mask.  Returns (send buffer, staging tensor or None)."""
    dev = _need_gpu(*slabs, *q_slabs)
    lib = _lib.load()
    Kl, S, D = slabs[0].shape
    ns, nq = len(slabs), len(q_slabs)
    ld = slabs[0].stride(1)
    dt = _DT.get(slabs[0].dtype)
    if any(t.shape != (Kl, S, D) or t.stride(2) != 1 or t.stride(1) != ld or t.dtype != slabs[0].dtype for t in slabs):
        raise ValueError("edit_halo_pack: slabs must be [Kl, S, D] views sharing dtype and token stride")
    ld_q = q_slabs[0].stride(1) if nq else ld
    if any(t.shape != (Kl, S, D) or t.stride(2) != 1 or t.stride(1) != ld_q or t.dtype != slabs[0].dtype for t in q_slabs):
        raise ValueError("edit_halo_pack: q_slabs must be [Kl, S, D] views of the slabs' dtype sharing one token stride")
    ms = [int(m) for m in masks]
    if not ms or Kl > 64 or any(m < 0 or m >> Kl for m in ms):
        raise ValueError(f"edit_halo_pack: masks {[hex(m) for m in ms]} (bits below the {Kl} <= 64 local frames, one mask per peer)")
    rows = sum(bin(m).count("1") for m in ms)
    out = _caller_buffer("edit_halo_pack", "out", out, (rows, ns, S, D), slabs[0].dtype, slabs[0].device)
    q_out = _caller_buffer("edit_halo_pack", "q_out", q_out, (nq, Kl, S, D), slabs[0].dtype, slabs[0].device) if nq else None
    ptrs = (ctypes.c_void_p * ns)(*[t.data_ptr() for t in slabs])
    fs = (ctypes.c_int64 * ns)(*[t.stride(0) for t in slabs])
    qptrs = (ctypes.c_void_p * max(nq, 1))(*[t.data_ptr() for t in q_slabs])
    qfs = (ctypes.c_int64 * max(nq, 1))(*[t.stride(0) for t in q_slabs])
    tab = (ctypes.c_uint64 * len(ms))(*ms)
    _launch(dev, "tf_edit_halo_pack", lib.tf_edit_halo_pack, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(fs, ctypes.c_void_p),
            ns, out.data_ptr() if rows else slabs[0].data_ptr(), len(ms), ctypes.cast(tab, ctypes.c_void_p),
            ctypes.cast(qptrs, ctypes.c_void_p) if nq else None, ctypes.cast(qfs, ctypes.c_void_p) if nq else None, nq,
            q_out.data_ptr() if nq else None, Kl, S, D, ld, ld_q, -1 if dt is None else dt)
    return out, q_out


def head_unpack(recv: torch.Tensor, dsts: Sequence[torch.Tensor]) -> None:
    """recv [W, Kl, nb, S, hd] (what the second all-to-all delivers) -> dsts[b][f, s, w*hd:(w+1)*hd], nb tensors
    [Kl, S, W*hd], nb <= 6 * TF_MAX_EDITS (tf_head_unpack, one launch)."""
    dev = _need_gpu(recv, *dsts)
    lib = _lib.load()
    W, Kl, nb, S, hd = recv.shape
    ld = dsts[0].stride(1)
    if (len(dsts) != nb or not recv.is_contiguous()
            or any(t.shape != (Kl, S, W * hd) or t.stride(2) != 1 or t.stride(1) != ld or t.dtype != recv.dtype
                   for t in dsts)):
        raise ValueError("head_unpack: bad arguments")
    ptrs = (ctypes.c_void_p * nb)(*[t.data_ptr() for t in dsts])
    fs = (ctypes.c_int64 * nb)(*[t.stride(0) for t in dsts])
    _launch(dev, "tf_head_unpack", lib.tf_head_unpack, recv.data_ptr(), ctypes.cast(ptrs, ctypes.c_void_p),
            ctypes.cast(fs, ctypes.c_void_p), nb, W, Kl, S, hd, ld, recv.element_size())


def pivot_inv_norm(piv: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """1/||row|| for pivots [..., D] (bf16/f16, contiguous) -> fp32 [...] (written into `out` when given: a
    contiguous fp32 tensor of that shape, e.g. slots of a halo-extended buffer)."""
    dev = _need_gpu(piv, out)
    lib = _lib.load()
    piv = piv.contiguous()
    D = piv.shape[-1]
    rows = piv.numel() // D
    if out is None:
        out = torch.empty(piv.shape[:-1], dtype=torch.float32, device=piv.device)
    elif out.dtype != torch.float32 or out.shape != piv.shape[:-1] or not out.is_contiguous():
        raise ValueError("pivot_inv_norm: `out` must be a contiguous fp32 tensor of shape piv.shape[:-1]")
    _launch(dev, "tf_pivot_inv_norm", lib.tf_pivot_inv_norm, piv.data_ptr(), out.data_ptr(), rows, D, _DT[piv.dtype])
    return out


def nn_search(tgt: torch.Tensor, piv: torch.Tensor, inv_norm: torch.Tensor, kf_ids: Sequence[int],
              idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tgt [n*S, D], piv [K, S, D] (same 16-bit dtype), inv_norm fp32 [K, S]; kf_ids = 1 or 2 keyframe
    indices in the reference's order [i, i-1] (tokenflow_utils.py:331-333).  Returns int32 [P, n*S] (written into `idx` when
    given: a contiguous int32 tensor of that shape)."""
    dev = _need_gpu(tgt, piv, inv_norm, idx)
    lib = _lib.load()
    tgt, piv = tgt.contiguous(), piv.contiguous()
    K, S, D = piv.shape
    n_tgt = tgt.shape[0]
    P = len(kf_ids)
    if tgt.dtype != piv.dtype or tgt.shape[1] != D or P not in (1, 2) or any(not 0 <= i < K for i in kf_ids):
        raise ValueError("nn_search: bad arguments")
    idx = _caller_buffer("nn_search", "idx", idx, (P, n_tgt), torch.int32, tgt.device)
    ws = _workspace(lib.tf_nn_search_workspace_bytes(n_tgt, S, D, P), tgt.device, "nn")
    _launch(dev, "tf_nn_search", lib.tf_nn_search, tgt.data_ptr(), piv.data_ptr(), inv_norm.data_ptr(), idx.data_ptr(),
            n_tgt, S, D, P, int(kf_ids[0]), int(kf_ids[1]) if P == 2 else 0, _DT[tgt.dtype], ws.data_ptr(), ws.numel())
    return idx


def gather_blend(kf_out: torch.Tensor, idx: torch.Tensor, w: Optional[torch.Tensor], kf_ids: Sequence[int],
                 n: int, residual: Optional[torch.Tensor], out_dtype: torch.dtype,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kf_out [3K,S,D]; idx int32 [P, n*S]; w fp32 [n] (P == 2); residual [3n,S,D] or None.
    Returns [3n,S,D] of out_dtype (tokenflow_utils.py:362-397), written into `out` when given (contiguous, that shape and
    dtype)."""
    dev = _need_gpu(kf_out, idx, w, residual, out)
    lib = _lib.load()
    kf_out = kf_out.contiguous()
    BK, S, D = kf_out.shape
    K = BK // 3
    P = len(kf_ids)
    if residual is not None:
        residual = residual.contiguous()
    out = _caller_buffer("gather_blend", "out", out, (3 * n, S, D), out_dtype, kf_out.device)
    _launch(dev, "tf_gather_blend", lib.tf_gather_blend, kf_out.data_ptr(), idx.data_ptr(),
            w.data_ptr() if w is not None else 0, residual.data_ptr() if residual is not None else 0, out.data_ptr(),
            K, n, S, D, P, int(kf_ids[0]), int(kf_ids[1]) if P == 2 else 0, _DT[kf_out.dtype],
            _DT[residual.dtype] if residual is not None else 0, _DT[out_dtype])
    return out


def layer_norm(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float,
               out_dtype: torch.dtype, want_inv_norm: bool = False, out: Optional[torch.Tensor] = None,
               inv_out: Optional[torch.Tensor] = None):
    """LayerNorm over the last dim of x [..., D] (fp32 statistics, one rounding to out_dtype) and, on request,
    1/||row||_2 of the rounded output rows (fp32 [...]).  Returns (out, inv_norm or None).
    out / inv_out: contiguous destination tensors of x's shape (out_dtype) / x.shape[:-1] (fp32) to write into -- e.g.
    views of a block's halo-extended propagation state (the sharded hook pass: no staging copy behind the norm)."""
    dev = _need_gpu(x, weight, bias)
    lib = _lib.load()
    x = x.contiguous()
    D = x.shape[-1]
    rows = x.numel() // D
    if weight is not None and bias is not None and weight.dtype != bias.dtype:
        bias = bias.to(weight.dtype)
    wt = weight if weight is not None else bias
    if wt is not None and wt.dtype not in _DT:
        raise TypeError(f"layer_norm: weight dtype {wt.dtype}")
    weight = weight.contiguous() if weight is not None else None
    bias = bias.contiguous() if bias is not None else None
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    elif out.shape != x.shape or out.dtype != out_dtype or not out.is_contiguous() or out.device != x.device:
        raise ValueError("layer_norm: `out` must be a contiguous tensor of x's shape, out_dtype and device")
    inv = None
    if want_inv_norm:
        if inv_out is None:
            inv = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
        elif (inv_out.shape != x.shape[:-1] or inv_out.dtype != torch.float32 or not inv_out.is_contiguous()
              or inv_out.device != x.device):
            raise ValueError("layer_norm: `inv_out` must be a contiguous fp32 tensor of shape x.shape[:-1]")
        else:
            inv = inv_out
    _launch(dev, "tf_layer_norm", lib.tf_layer_norm, x.data_ptr(), weight.data_ptr() if weight is not None else 0,
            bias.data_ptr() if bias is not None else 0, out.data_ptr(), inv.data_ptr() if inv is not None else 0,
            rows, D, float(eps), _DT[x.dtype], _DT[wt.dtype] if wt is not None else 0, _DT[out_dtype])
    return out, inv


def add_layer_norm(a: torch.Tensor, b: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                   eps: float, out_dtype: torch.dtype, total: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None):
    """(a + b, LayerNorm(a + b)) in one pass (tf_add_layer_norm): the sum has torch's promoted dtype and rounding, the
    norm is `layer_norm` of that rounded sum -- bit-identical to the two separate ops.
    total / out: contiguous destination tensors of a's shape (the promoted dtype / out_dtype) to write into."""
    dev = _need_gpu(a, b, weight, bias, total, out)
    lib = _lib.load()
    if a.shape != b.shape:
        raise ValueError("add_layer_norm: a and b must have one shape")
    a, b = a.contiguous(), b.contiguous()
    D = a.shape[-1]
    rows = a.numel() // D
    if weight is not None and bias is not None and weight.dtype != bias.dtype:
        bias = bias.to(weight.dtype)
    wt = weight if weight is not None else bias
    weight = weight.contiguous() if weight is not None else None
    bias = bias.contiguous() if bias is not None else None
    total = _caller_buffer("add_layer_norm", "total", total, a.shape, torch.promote_types(a.dtype, b.dtype), a.device)
    out = _caller_buffer("add_layer_norm", "out", out, a.shape, out_dtype, a.device)
    _launch(dev, "tf_add_layer_norm", lib.tf_add_layer_norm, a.data_ptr(), b.data_ptr(), total.data_ptr(),
            weight.data_ptr() if weight is not None else 0, bias.data_ptr() if bias is not None else 0, out.data_ptr(),
            rows, D, float(eps), _DT[a.dtype], _DT[b.dtype], _DT[total.dtype], _DT[wt.dtype] if wt is not None else 0,
            _DT[out_dtype])
    return total, out


def norm_fusable(kf_out: torch.Tensor, residual: Optional[torch.Tensor], out_dtype: torch.dtype, P: int,
                 norm_dtype: torch.dtype) -> bool:
    """Can `propagate` / `propagate_chunks` carry the block's next LayerNorm (their `norm=` argument)?  The fused
    form covers the hook path's types: a 16-bit cached attention output, a residual and a norm output of that same
    type, the result in fp32 (two keyframes blended) or that type (one keyframe)."""
    dt = kf_out.dtype
    return (dt in (torch.bfloat16, torch.float16) and residual is not None and residual.dtype == dt
            and norm_dtype == dt and out_dtype == (torch.float32 if P == 2 else dt) and kf_out.shape[-1] <= 1536)


def _norm_args(norm, like: torch.Tensor, shape, norm_out: Optional[torch.Tensor] = None):
    """(gamma ptr, beta ptr, eps, w dtype code, norm_out tensor, norm dtype code) of a `norm=(weight, bias, eps,
    dtype)` argument; the norm output goes into the caller's `norm_out` when given."""
    weight, bias, eps, ndt = norm
    if weight is not None and bias is not None and weight.dtype != bias.dtype:
        bias = bias.to(weight.dtype)
    wt = weight if weight is not None else bias
    if wt is not None and wt.dtype not in _DT:
        raise TypeError(f"propagate: norm weight dtype {wt.dtype}")
    weight = weight.contiguous() if weight is not None else None
    bias = bias.contiguous() if bias is not None else None
    nout = _caller_buffer("propagate", "norm_out", norm_out, shape, ndt, like.device)
    return (weight.data_ptr() if weight is not None else 0, bias.data_ptr() if bias is not None else 0, float(eps),
            _DT[wt.dtype] if wt is not None else 0, nout, _DT[ndt], (weight, bias))


def _propagate_begin(what: str, tgt, piv, inv_norm, kf_out, w, residual, out, norm, norm_out):
    """What every propagation wrapper checks first; returns (device, library)."""
    dev = _need_gpu(tgt, piv, inv_norm, kf_out, w, residual, out, norm_out)
    if norm_out is not None and norm is None:
        raise ValueError(f"{what}: `norm_out` without `norm`")
    return dev, _lib.load()


def _propagate_call(what: str, dev, lib, name: str, name_norm: str, tgt, piv, inv_norm, kf_out, w, residual, out_dtype,
                    norm, out, norm_out, *, rows: int, P: int, ws_bytes: int, shape_args: tuple, single_dtype: bool = True,
                    tail: tuple = (), residual_is: Optional[str] = None, codes_first: bool = False):
    """The body of every propagation wrapper behind its own shape check: contiguous inputs, the result of `rows` frames,
    the scratch of `ws_bytes`, then entry point `name`, or `name_norm` with the fused norm of a P-keyframe gather.
    The entry points take: the seven tensors, `shape_args`, the four dtype codes, the dtype of a one-keyframe chunk's own
    pass (`single_dtype`: the chunk forms), `tail`, then the norm's arguments and the scratch.
    residual_is: the shape to name when the residual is not [rows, S, D] (None: the C entry point's business).
    codes_first: the dtype codes are looked up before the fused-norm checks, not behind them (the segments, edits and
    ragged wrappers always did: an unsupported dtype is their KeyError even where the norm would be refused too)."""
    tgt, piv, kf_out = tgt.contiguous(), piv.contiguous(), kf_out.contiguous()
    shape = (rows,) + tuple(piv.shape[1:])
    if residual is not None:
        residual = residual.contiguous()
        if residual_is is not None and residual.shape != shape:
            raise ValueError(f"{what}: residual must be {residual_is}")
    out = _caller_buffer(what, "out", out, shape, out_dtype, kf_out.device)
    ws = _workspace(ws_bytes, tgt.device, "nn")
    # what the reference's single-keyframe pass would emit for a one-keyframe chunk: kf dtype (+ residual), torch promotion
    single = (kf_out.dtype if residual is None else torch.promote_types(kf_out.dtype, residual.dtype),) if single_dtype else ()

    def codes():    # an unsupported dtype is a KeyError here
        return (_DT[tgt.dtype], _DT[kf_out.dtype], _DT[residual.dtype] if residual is not None else 0, _DT[out_dtype],
                *(_DT[dt] for dt in single))

    dts = codes() if codes_first else None
    nout = None
    if norm is not None:
        if not norm_fusable(kf_out, residual, out_dtype, P, norm[3]):
            raise TypeError(f"{what}: these dtypes have no fused-norm form (ops.norm_fusable)")
        g, b, eps, wdt, nout, ndt, _keep = _norm_args(norm, kf_out, shape, norm_out)
        name, tail = name_norm, tail + (g, b, eps, wdt, nout.data_ptr(), ndt)
    _launch(dev, name, getattr(lib, name), tgt.data_ptr(), piv.data_ptr(), inv_norm.data_ptr(), kf_out.data_ptr(),
            w.data_ptr() if w is not None else 0, residual.data_ptr() if residual is not None else 0, out.data_ptr(),
            *shape_args, *(dts or codes()), *tail, ws.data_ptr(), ws.numel())
    return out if nout is None else (out, nout)


def propagate(tgt: torch.Tensor, piv: torch.Tensor, inv_norm: torch.Tensor, kf_ids: Sequence[int],
              kf_out: torch.Tensor, w: Optional[torch.Tensor], n: int, residual: Optional[torch.Tensor],
              out_dtype: torch.dtype, norm=None, out: Optional[torch.Tensor] = None,
              norm_out: Optional[torch.Tensor] = None):
    """nn_search + gather_blend of one chunk in one call (tokenflow_utils.py:329-397): same arguments, same
    results bit for bit, one launch less (the gather merges the search's per-split candidates itself).
    norm = (weight, bias, eps, dtype) of the block's next LayerNorm (see `norm_fusable`): returns
    (result, LayerNorm(result) in `dtype`) from one gather launch -- tf_nn_gather_blend_norm, both bit-identical to
    the separate calls.
    out / norm_out: contiguous destination tensors of the result's shape ([3n,S,D]; out_dtype / the norm's dtype) to write
    into; norm_out needs `norm`."""
    what = "propagate"
    dev, lib = _propagate_begin(what, tgt, piv, inv_norm, kf_out, w, residual, out, norm, norm_out)
    K, S, D = piv.shape
    n_tgt = tgt.shape[0]
    P = len(kf_ids)
    if (tgt.dtype != piv.dtype or tgt.shape[1] != D or P not in (1, 2) or any(not 0 <= i < K for i in kf_ids)
            or n_tgt != n * S or kf_out.shape != (3 * K, S, D)):
        raise ValueError("propagate: bad arguments")
    return _propagate_call(what, dev, lib, "tf_nn_gather_blend", "tf_nn_gather_blend_norm", tgt, piv, inv_norm, kf_out, w,
                           residual, out_dtype, norm, out, norm_out, rows=3 * n, P=P,
                           ws_bytes=lib.tf_nn_gather_blend_workspace_bytes(n_tgt, S, D, P),
                           shape_args=(K, n, S, D, P, int(kf_ids[0]), int(kf_ids[1]) if P == 2 else 0), single_dtype=False)


def propagate_chunks(tgt: torch.Tensor, piv: torch.Tensor, inv_norm: torch.Tensor, kf_out: torch.Tensor,
                     w: torch.Tensor, n: int, n_chunks: int, slot0: int, first_single: bool,
                     residual: Optional[torch.Tensor], out_dtype: torch.dtype, norm=None,
                     out: Optional[torch.Tensor] = None, norm_out: Optional[torch.Tensor] = None):
    """`propagate` for a run of `n_chunks` consecutive chunks of n frames in one call (tf_nn_gather_blend_chunks):
    tgt [n_chunks*n*S, D] chunk-major, residual / result [3*n_chunks*n, S, D]; chunk j matches keyframe slots
    slot0 + j and slot0 + j - 1 of piv / inv_norm / kf_out; first_single: chunk 0 of the run is chunk 0 of the
    video (one keyframe).  Bit-identical to n_chunks calls of `propagate`.  out / norm_out as there."""
    what = "propagate_chunks"
    dev, lib = _propagate_begin(what, tgt, piv, inv_norm, kf_out, w, residual, out, norm, norm_out)
    K, S, D = piv.shape
    C = int(n_chunks)
    if C == 1:
        ids = [slot0] if first_single else [slot0, slot0 - 1]
        return propagate(tgt, piv, inv_norm, ids, kf_out, None if first_single else w, n, residual, out_dtype,
                         norm=norm, out=out, norm_out=norm_out)
    if (tgt.dtype != piv.dtype or tgt.shape != (C * n * S, D) or kf_out.shape != (3 * K, S, D) or w is None
            or slot0 + C > K or slot0 < (0 if first_single else 1)):
        raise ValueError("propagate_chunks: bad arguments")
    return _propagate_call(what, dev, lib, "tf_nn_gather_blend_chunks", "tf_nn_gather_blend_chunks_norm", tgt, piv, inv_norm,
                           kf_out, w, residual, out_dtype, norm, out, norm_out, rows=3 * C * n, P=2,
                           ws_bytes=lib.tf_nn_gather_blend_chunks_workspace_bytes(n * S, S, D, C),
                           shape_args=(K, n, C, S, D, int(slot0), 1 if first_single else 0))


def propagate_chunks_segments(tgt: torch.Tensor, piv: torch.Tensor, inv_norm: torch.Tensor, kf_out: torch.Tensor,
                              w: torch.Tensor, n: int, n_chunks: int, slot0: int, single_mask: int,
                              residual: Optional[torch.Tensor], out_dtype: torch.dtype, norm=None,
                              out: Optional[torch.Tensor] = None, norm_out: Optional[torch.Tensor] = None):
    """`propagate_chunks` for a run of chunks that crosses scene cuts (tf_nn_gather_blend_chunks_segments): bit j of
    `single_mask` = chunk j of the run is the first chunk of a keyframe segment, a one-keyframe chunk matching slot0 + j
    alone (its rows rounded as chunk 0's of a video are); every other chunk j matches slots slot0 + j and slot0 + j - 1.
    One search and one gather for the whole run.  Masks 1 and 0 are `propagate_chunks` with and without first_single; one
    chunk is `propagate`.  out / norm_out as there."""
    C = int(n_chunks)
    m = _single_mask("propagate_chunks_segments", single_mask, C)
    if C == 1:
        return propagate_chunks(tgt, piv, inv_norm, kf_out, w, n, C, slot0, bool(m & 1), residual, out_dtype, norm=norm,
                                out=out, norm_out=norm_out)
    what = "propagate_chunks_segments"
    dev, lib = _propagate_begin(what, tgt, piv, inv_norm, kf_out, w, residual, out, norm, norm_out)
    K, S, D = piv.shape
    if (tgt.dtype != piv.dtype or tgt.shape != (C * n * S, D) or kf_out.shape != (3 * K, S, D) or w is None
            or slot0 + C > K or slot0 < (0 if m & 1 else 1)):
        raise ValueError("propagate_chunks_segments: bad arguments")
    return _propagate_call(what, dev, lib, "tf_nn_gather_blend_chunks_segments", "tf_nn_gather_blend_chunks_norm_segments",
                           tgt, piv, inv_norm, kf_out, w, residual, out_dtype, norm, out, norm_out, rows=3 * C * n, P=2,
                           ws_bytes=lib.tf_nn_gather_blend_chunks_workspace_bytes(n * S, S, D, C),
                           shape_args=(K, n, C, S, D, int(slot0), m), codes_first=True)


def propagate_chunks_edits(tgt: torch.Tensor, piv: torch.Tensor, inv_norm: torch.Tensor, kf_out: torch.Tensor,
                           w: Optional[torch.Tensor], n: int, n_chunks: int, slot0: int, first_single: bool,
                           residual: Optional[torch.Tensor], out_dtype: torch.dtype, n_edits: int, norm=None,
                           out: Optional[torch.Tensor] = None, norm_out: Optional[torch.Tensor] = None):
    """`propagate_chunks` (n_chunks = 1: `propagate`) for a multi-edit batch of B = 1 + 2*n_edits branches: kf_out [B*K,S,D],
    residual / result [B*n_chunks*n, S, D]; tgt (the source branch's rows), piv, inv_norm, w as there.  ONE search -- it
    reads the source branch only -- and one gather over all B branches on the same candidates; every branch of the result
    is bit-identical to the same branch of the single-edit call on [source | uncond_e | cond_e].
    norm=, out / norm_out ([B*n_chunks*n, S, D]) as `propagate`."""
    what = "propagate_chunks_edits"
    dev, lib = _propagate_begin(what, tgt, piv, inv_norm, kf_out, w, residual, out, norm, norm_out)
    E = int(n_edits)
    if not 1 <= E <= _lib.TF_MAX_EDITS:
        raise ValueError(f"propagate_chunks_edits: n_edits={n_edits} (1 .. {_lib.TF_MAX_EDITS})")
    nbr = 1 + 2 * E
    K, S, D = piv.shape
    C = int(n_chunks)
    single = C == 1 and first_single           # the one-keyframe chunk 0 of the video alone: P = 1
    if (tgt.dtype != piv.dtype or tgt.shape != (C * n * S, D) or kf_out.shape != (nbr * K, S, D)
            or (w is None and not single) or slot0 + C > K or slot0 < (0 if first_single else 1)):
        raise ValueError("propagate_chunks_edits: bad arguments")
    return _propagate_call(what, dev, lib, "tf_nn_gather_blend_chunks_edits", "tf_nn_gather_blend_chunks_norm_edits", tgt, piv,
                           inv_norm, kf_out, w, residual, out_dtype, norm, out, norm_out, rows=nbr * C * n,
                           P=1 if single else 2,
                           ws_bytes=max(lib.tf_nn_gather_blend_chunks_workspace_bytes(n * S, S, D, C),
                                        lib.tf_nn_gather_blend_workspace_bytes(n * S, S, D, 1) if single else 0),
                           shape_args=(K, n, C, S, D, int(slot0), 1 if first_single else 0), tail=(E,),
                           residual_is="[B*n_chunks*n, S, D]", codes_first=True)


def propagate_chunks_ragged(tgt: torch.Tensor, piv: torch.Tensor, inv_norm: torch.Tensor, kf_out: torch.Tensor,
                            w: torch.Tensor, chunk_frames, slot0: int, single_mask: int,
                            residual: Optional[torch.Tensor], out_dtype: torch.dtype, n_edits: int = 1, norm=None,
                            out: Optional[torch.Tensor] = None, norm_out: Optional[torch.Tensor] = None):
    """`propagate_chunks_segments` / `propagate_chunks_edits` for a run of chunks of UNEQUAL frame count
    (tf_nn_gather_blend_chunks_ragged): chunk j has chunk_frames[j] frames, F = sum(chunk_frames).  tgt [F*S, D] chunk-major,
    kf_out [B*K, S, D], residual / result [B*F, S, D] with B = 1 + 2*n_edits; slot0 and single_mask as
    `propagate_chunks_segments` (n_edits > 1: bit 0 only).  w: F floats on the device, one per frame of the run -- the blend
    weights of each chunk's own size, concatenated.  The rows of chunk j are what `propagate` computes on that chunk alone
    with n = chunk_frames[j].  ONE search and one gather; equal frame counts issue today's calls.  norm=, out / norm_out as
    `propagate`."""
    what = "propagate_chunks_ragged"
    fr, arr = _chunk_frames(what, chunk_frames)
    C, F = len(fr), sum(fr)
    m = _single_mask(what, single_mask, C)
    E = int(n_edits)
    if not 1 <= E <= _lib.TF_MAX_EDITS:
        raise ValueError(f"{what}: n_edits={n_edits} (1 .. {_lib.TF_MAX_EDITS})")
    if E > 1 and m > 1:
        raise ValueError(f"{what}: single_mask {m:#x} with {E} edits (segments and multi-edit batches do not combine)")
    if C == 1:      # one chunk: today's one-chunk paths
        if E == 1:
            return propagate_chunks(tgt, piv, inv_norm, kf_out, w, fr[0], 1, slot0, bool(m & 1), residual, out_dtype,
                                    norm=norm, out=out, norm_out=norm_out)
        return propagate_chunks_edits(tgt, piv, inv_norm, kf_out, w, fr[0], 1, slot0, bool(m & 1), residual, out_dtype, E,
                                      norm=norm, out=out, norm_out=norm_out)
    dev, lib = _propagate_begin(what, tgt, piv, inv_norm, kf_out, w, residual, out, norm, norm_out)
    nbr = 1 + 2 * E
    K, S, D = piv.shape
    if (tgt.dtype != piv.dtype or tgt.shape != (F * S, D) or kf_out.shape != (nbr * K, S, D) or w is None
            or w.dtype != torch.float32 or w.numel() != F or not w.is_contiguous()
            or slot0 + C > K or slot0 < (0 if m & 1 else 1)):
        raise ValueError(f"{what}: bad arguments")
    return _propagate_call(what, dev, lib, "tf_nn_gather_blend_chunks_ragged", "tf_nn_gather_blend_chunks_norm_ragged", tgt, piv,
                           inv_norm, kf_out, w, residual, out_dtype, norm, out, norm_out, rows=nbr * F, P=2,
                           ws_bytes=lib.tf_nn_gather_blend_ragged_workspace_bytes(arr, C, S, D),
                           shape_args=(K, arr, C, S, D, int(slot0), m), tail=(E,),
                           residual_is="[B*sum(chunk_frames), S, D]", codes_first=True)


def inject_copy_edits_(x: torch.Tensor, n_edits: int, edit_mask: Optional[int] = None) -> torch.Tensor:
    """In place, multi-edit batch of B = 1 + 2*n_edits branches: x[b*n:(b+1)*n] = x[:n] for every b >= 1, n = len(x)//B
    (tokenflow_utils.py:87-91 for every edit).  n_edits = 1 is `inject_copy_`.
    edit_mask: only the uncond and cond branches of the edits whose bit is set take the source (tf_inject_copy_edits_masked:
    one launch, the other branches untouched; 0 launches nothing); None = every edit, today's call."""
    dev = _need_gpu(x)
    lib = _lib.load()
    nbr = 1 + 2 * int(n_edits)
    if not 1 <= int(n_edits) <= _lib.TF_MAX_EDITS or x.shape[0] % nbr or not x.is_contiguous():
        raise ValueError(f"inject_copy_edits_: need a contiguous tensor whose batch is a multiple of {nbr} "
                         f"(n_edits 1 .. {_lib.TF_MAX_EDITS})")
    if edit_mask is not None:
        _launch(dev, "tf_inject_copy_edits_masked", lib.tf_inject_copy_edits_masked, x.data_ptr(), x.numel() // nbr, nbr,
                _edit_mask("inject_copy_edits_", edit_mask, n_edits), x.element_size())
        return x
    _launch(dev, "tf_inject_copy_edits", lib.tf_inject_copy_edits, x.data_ptr(), x.numel() // nbr, nbr, x.element_size())
    return x


def inject_copy_(x: torch.Tensor) -> torch.Tensor:
    """In place: x[n:2n] = x[:n]; x[2n:] = x[:n] with n = len(x)//3 (tokenflow_utils.py:87-91)."""
    dev = _need_gpu(x)
    lib = _lib.load()
    if x.shape[0] % 3 or not x.is_contiguous():
        raise ValueError("inject_copy_: need a contiguous tensor whose batch is a multiple of 3")
    per_branch = x.numel() // 3
    _launch(dev, "tf_inject_copy", lib.tf_inject_copy, x.data_ptr(), per_branch, x.element_size())
    return x


def ddim_step(x: torch.Tensor, eps: torch.Tensor, mu_a: float, sigma_a: float, mu_b: float, sigma_b: float,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = mu_b * ((x - sigma_a*eps) / mu_a) + sigma_b*eps  (preprocess.py:224-225 / 259-260), one launch, the
    reference's per-op rounding.  x, eps: same shape and dtype (f16 / bf16 / f32), contiguous; out may be x."""
    dev = _need_gpu(x, eps, out)
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(x)
    if (eps.shape != x.shape or eps.dtype != x.dtype or out.shape != x.shape or out.dtype != x.dtype
            or x.dtype not in _DT or not (x.is_contiguous() and eps.is_contiguous() and out.is_contiguous())):
        raise ValueError("ddim_step: x, eps, out must be contiguous tensors of one shape and dtype (f16/bf16/f32)")
    _launch(dev, "tf_ddim_step", lib.tf_ddim_step, x.data_ptr(), eps.data_ptr(), out.data_ptr(), x.numel(),
            float(mu_a), float(sigma_a), float(mu_b), float(sigma_b), _DT[x.dtype])
    return out
