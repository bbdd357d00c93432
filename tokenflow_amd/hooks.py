"""The reference's hook API for the per-step hot path, on MI355X kernels.

Same function names, signatures, installation style and per-module state as
omerbt/TokenFlow `tokenflow_utils.py` (paths below are into that repository), so the
reference's `run_tokenflow_pnp.py` / `run_tokenflow_sdedit.py` import this through the
drop-in module `tokenflow_utils.py` at the repo root, unmodified.

What differs from the reference is only *how* the tensors are computed:

* `sa_forward.forward` (114-199 / 224-281): the bank replication, head permutes, per-head
  bmm/softmax/bmm loops and re-layout are one fused HIP launch (`ops.ext_attn`); injection
  (124-130) is pointer aliasing instead of four in-place slice copies.
* `TokenFlowBlock.forward` propagation branch (329-397): cosine similarity + argmax is
  `ops.nn_search` (the similarity matrix is never materialised), gather + blend + residual
  is `ops.gather_blend`.
* `conv_forward.forward` (86-91): the two slice copies are `ops.inject_copy_`, applied by a forward hook on the
  resnet's `conv2` instead of a transcription of diffusers' `ResnetBlock2D.forward` (51-98).
* `t in injection_schedule` on a device tensor (86,124) costs a host sync per call in the
  reference; the schedule is converted to a Python set once at registration.
* `register_pivotal` / `register_batch_idx` (7-17) walk `named_modules()` of the whole
  pipeline on every call in the reference; the matching blocks are cached per model.
* `load_source_latents_t` (43-47) re-reads the file from disk on every call in the
  reference; files are cached by (path, mtime).

There is no CPU / eager fallback: the ops raise on CPU tensors or when the HIP library is
missing.
"""
import collections
import logging
import os
import sys
from typing import Type

import torch

from . import ops

__all__ = [
    "register_pivotal", "register_batch_idx", "register_time", "load_source_latents_t",
    "register_conv_injection", "register_extended_attention_pnp", "register_extended_attention",
    "make_tokenflow_attention_block", "set_tokenflow", "isinstance_str", "batch_cosine_sim",
    "register_frame_shard", "join_frame_shard", "register_edits", "register_segments", "register_chunk_frames",
    "register_bank_window",
]


def isinstance_str(x: object, cls_name: str) -> bool:
    """Class-*name* match over the MRO (util.py:46-58): lets the hooks patch diffusers
    modules without importing diffusers."""
    return any(c.__name__ == cls_name for c in type(x).__mro__)


def batch_cosine_sim(x, y):
    """Public export of util.py:61-69, kept for API compatibility.  The hooks do NOT call
    it: the product path is ops.nn_search, which never materialises this matrix."""
    if type(x) is list:
        x = torch.cat(x, dim=0)
    if type(y) is list:
        y = torch.cat(y, dim=0)
    return (x / x.norm(dim=-1, keepdim=True)) @ (y / y.norm(dim=-1, keepdim=True)).T


# --------------------------------------------------------------------------- state setters
def _tokenflow_blocks(model):
    cache = model.__dict__.get("_tf_block_cache")
    if cache is None:
        cache = [m for _, m in model.named_modules() if isinstance_str(m, "BasicTransformerBlock")]
        model.__dict__["_tf_block_cache"] = cache
    return cache


def register_pivotal(diffusion_model, is_pivotal):
    """tokenflow_utils.py:7-11."""
    for module in _tokenflow_blocks(diffusion_model):
        setattr(module, "pivotal_pass", is_pivotal)


def register_batch_idx(diffusion_model, batch_idx):
    """tokenflow_utils.py:13-17."""
    for module in _tokenflow_blocks(diffusion_model):
        setattr(module, "batch_idx", batch_idx)


def register_frame_shard(diffusion_model, shard):
    """Multi-GPU extension (no counterpart in the single-process reference): one process per GPU, each running the
    SAME driver on ITS run of chunks.  `shard` = `tokenflow_amd.sharded.FrameShard` / `NativeShard` (rank r owns the
    keyframes and chunks shard.kf0 .. shard.kf0 + shard.Kl - 1), or None to go back to one process.  With a shard set:
      * the pivotal pass carries the rank's LOCAL keyframes only ([3*Kl, S, D] per block); `attn1` attends to all K
        keyframes through `shard.pivotal_attention` (frames<->heads all-to-all or the bank all-gather), and the block
        hands its last keyframe's pivots / inverse norms / attention output to rank r+1 (the pivots' half is issued
        before the attention and travels under it);
      * the chunk passes name GLOBAL chunk indices (`register_batch_idx(model, c)`, c owned by this rank; a run of the
        rank's chunks for the one-pass form) and read keyframes c and c-1 (tokenflow_utils.py:331-333) from the
        rank's halo-extended caches, the first one waiting for the neighbour's message.
    Results equal the single-process hooks' in the bit-stable mode (TOKENFLOW_ATTN_NO_SPLIT=1) bit for bit (`FrameShard`'s
    default one-pass attention; against the default single-process mode: within the attention's parity bound); every rank must
    draw the same `pivotal_idx` (run_tokenflow_pnp.py:224).  INTEGRATION.md section 3 shows the driver side.
    With `register_edits(model, E > 1)` the batches are the rank's keyframes / chunks of all 1 + 2E branches and a `FrameShard`
    runs them as ONE multi-edit pass (`supports_edits`: one pack, the same collectives, one unpack, one search per block);
    `NativeShard` runs one edit and raises; `NativeEditShard` is its multi-edit form (one tf_rank_pivotal_edits call per block).
    A world-1 shard (one GPU) runs the bit-stable attention mode too unless it was built with `attn_split=True`: slower
    than the plain single-process hooks by the per-grid kernel choice it gives up (`tools/hooks_bench.py --ranks 1`)."""
    for module in _tokenflow_blocks(diffusion_model):
        module.__dict__["_tf_shard"] = shard
        module.__dict__.pop("_tf_halo", None)
        module.attn1.__dict__["_tf_shard"] = shard


def join_frame_shard(diffusion_model):
    """Order the CURRENT stream behind every neighbour halo of the pivotal pass that is still in flight.  The chunk
    passes do that themselves, block by block, the first time they read a block's halo slot -- which lets the halos
    travel under the rest of the pivotal pass; call this at the end of a pivotal pass that is captured into a HIP
    graph (tokenflow_amd.graphs.GraphCache): a capture must join every stream it forked before it ends, and the chunk
    passes' graphs then contain no wait on another graph's events."""
    for module in _tokenflow_blocks(diffusion_model):
        shard = module.__dict__.get("_tf_shard")
        halo = module.__dict__.get("_tf_halo")
        if shard is not None and halo is not None and halo[3]:
            shard.halo_wait(halo[3])
            module.__dict__["_tf_halo"] = (halo[0], halo[1], halo[2], [])


def _active_shard(module):
    shard = module.__dict__.get("_tf_shard")
    return shard if shard is not None and shard.world > 1 else None


_DOWN = {0: [0, 1], 1: [0, 1], 2: [0, 1]}
_UP = {1: [0, 1, 2], 2: [0, 1, 2], 3: [0, 1, 2]}
_INJECTED_UP = {1: [1, 2], 2: [0, 1, 2], 3: [0, 1, 2]}


def register_time(model, t):
    """tokenflow_utils.py:20-40: `t` on up_blocks[1].resnets[1] and on attn1/attn2 of the 16 blocks."""
    unet = model.unet
    setattr(unet.up_blocks[1].resnets[1], "t", t)
    for res, blocks in _UP.items():
        for b in blocks:
            tb = unet.up_blocks[res].attentions[b].transformer_blocks[0]
            setattr(tb.attn1, "t", t)
            setattr(tb.attn2, "t", t)
    for res, blocks in _DOWN.items():
        for b in blocks:
            tb = unet.down_blocks[res].attentions[b].transformer_blocks[0]
            setattr(tb.attn1, "t", t)
            setattr(tb.attn2, "t", t)
    tb = unet.mid_block.attentions[0].transformer_blocks[0]
    setattr(tb.attn1, "t", t)
    setattr(tb.attn2, "t", t)


def register_edits(model, n_edits):
    """Multi-edit extension (no counterpart in the reference, which runs one prompt per pass): the passes that follow carry
    E = n_edits edits of ONE source video, B = 1 + 2E branches [source | uncond_1 | cond_1 | ... | uncond_E | cond_E]
    instead of [source | uncond | cond].  Sets `n_edits` where `register_time` sets `t`: on the 16 blocks, their `attn1`
    and the injected resnet.  For every op of the path the slices of edit e are what the single-edit pass computes on
    [source | uncond_e | cond_e]; the NN search, the source branch and (under injection) the scores are computed once.
    n_edits = 1 (the default without this call) is the reference's layout and issues exactly the single-edit ops.
    Combines with `register_frame_shard` where the shard type runs multi-edit batches (`FrameShard.supports_edits`): every rank
    then runs one multi-edit pass on its keyframes and chunks.
    Not generalised, ValueError with n_edits > 1: a frame shard without that capability (NativeShard; NativeEditShard has it), the AdaLayerNormZero gated
    path, replay through `tokenflow_amd.graphs.GraphCache` (INTEGRATION.md section 4 shows the driver side)."""
    n_edits = int(n_edits)
    from . import _lib
    if not 1 <= n_edits <= _lib.TF_MAX_EDITS:
        raise ValueError(f"register_edits: n_edits={n_edits} (1 .. {_lib.TF_MAX_EDITS})")
    unet = model.unet
    setattr(unet.up_blocks[1].resnets[1], "n_edits", n_edits)
    tbs = [unet.up_blocks[res].attentions[b].transformer_blocks[0] for res, blocks in _UP.items() for b in blocks]
    tbs += [unet.down_blocks[res].attentions[b].transformer_blocks[0] for res, blocks in _DOWN.items() for b in blocks]
    tbs.append(unet.mid_block.attentions[0].transformer_blocks[0])
    _set_edits(tbs, n_edits)


def _set_edits(blocks, n_edits):
    """`n_edits` on transformer blocks and their `attn1` (register_edits; tools/hooks_bench.py on its bare block list)."""
    for tb in blocks:
        setattr(tb, "n_edits", n_edits)
        setattr(tb.attn1, "n_edits", n_edits)


def _n_edits(module) -> int:
    """Edits of the batch a module sees (register_edits); 1 = the reference's [source | uncond | cond]."""
    E = int(getattr(module, "n_edits", 1))
    if E > 1 and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise ValueError("register_edits: a multi-edit batch (n_edits > 1) cannot be captured for graphs.py replay yet")
    return E


def _hook_blocks(unet):
    """The 16 transformer blocks `register_time` addresses."""
    tbs = [unet.up_blocks[res].attentions[b].transformer_blocks[0] for res, blocks in _UP.items() for b in blocks]
    tbs += [unet.down_blocks[res].attentions[b].transformer_blocks[0] for res, blocks in _DOWN.items() for b in blocks]
    tbs.append(unet.mid_block.attentions[0].transformer_blocks[0])
    return tbs


def register_segments(model, keyframes_per_segment):
    """Keyframe-segment extension (no counterpart in the reference, whose passes are one shot): the passes that follow carry
    V scenes or clips.  `keyframes_per_segment` = [K_0, .., K_{V-1}], 1 <= V <= TF_MAX_SEGMENTS, K_v >= 1: segment v owns K_v
    CONSECUTIVE keyframes of the pivotal pass and the K_v chunks that belong to them; the batch layout stays
    [source | uncond | cond] x frames.  Sets `keyframe_segments` where `register_time` sets `t`: on the 16 blocks and their
    `attn1`.  For every op the slices of segment v are what the single-clip pass computes on segment v's tensors alone:
      * pivotal pass: a keyframe's uncond / cond branches attend to the keyframes of ITS segment (`ops.ext_attn_segments`,
        both attention installers); the pass must carry sum(K_v) keyframes (ValueError otherwise);
      * chunk passes: the first chunk of every segment is a one-keyframe chunk (tokenflow_utils.py:331-333, 390), every other
        chunk c blends keyframes c and c-1.  A one-chunk pass (`register_batch_idx(model, c)`) whose chunk starts a segment is
        the P = 1 `ops.propagate`; its frame count may differ from other passes', so a ragged last chunk of a scene works as it
        does for a single clip.  A run of chunks (`register_batch_idx(model, range(..))`) is ONE
        `ops.propagate_chunks_segments` with the mask of the segment starts inside the run.
    `None` or a single segment goes back to the one-shot path (exactly today's ops).
    Not generalised, ValueError with V > 1: `register_edits(model, E > 1)`, a registered frame shard, the AdaLayerNormZero
    gated path, capture for `tokenflow_amd.graphs.GraphCache` replay (INTEGRATION.md section 5 shows the driver side)."""
    from . import _lib
    segs = None
    if keyframes_per_segment is not None:
        segs = tuple(int(k) for k in keyframes_per_segment)
        if not 1 <= len(segs) <= _lib.TF_MAX_SEGMENTS or any(k < 1 for k in segs):
            raise ValueError(f"register_segments: {list(segs)} (1 .. {_lib.TF_MAX_SEGMENTS} segments of >= 1 keyframes)")
        if len(segs) == 1:
            segs = None
    _set_segments(_hook_blocks(model.unet), segs)


def _set_segments(blocks, segs):
    """`keyframe_segments` on transformer blocks and their `attn1` (register_segments; tools on a bare block list)."""
    for tb in blocks:
        setattr(tb, "keyframe_segments", segs)
        setattr(tb.attn1, "keyframe_segments", segs)


def _segments(module, K=None):
    """The keyframe segments of the passes a module sees (register_segments) or None = one shot; the combinations that are
    not generalised raise."""
    segs = getattr(module, "keyframe_segments", None)
    if segs is None:
        return None
    if int(getattr(module, "n_edits", 1)) > 1:
        raise ValueError("register_segments: keyframe segments in a multi-edit batch (register_edits, n_edits > 1) are not "
                         "supported")
    if module.__dict__.get("_tf_shard") is not None:
        raise ValueError("register_segments: keyframe segments on a registered frame shard are not supported")
    if getattr(module, "use_ada_layer_norm_zero", False):
        raise ValueError("register_segments: keyframe segments through the AdaLayerNormZero gated path are not supported")
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise ValueError("register_segments: a segmented pass cannot be captured for graphs.py replay yet")
    if K is not None and sum(segs) != K:
        raise ValueError(f"register_segments: the segments {list(segs)} hold {sum(segs)} keyframes, the pivotal pass {K}")
    return segs


def register_chunk_frames(model, frames_per_chunk):
    """Ragged chunk runs (no counterpart in the reference, which drops the tail of a video whose length is no multiple of
    batch_size): `frames_per_chunk` = the frame count of EVERY chunk of the video in global chunk order, each >= 1; `None`
    clears.  Opt-in -- without it every path stays as it is, the error for a run whose frames do not split evenly included.
    Sets `chunk_frames` on the 16 blocks.  With it a run pass `register_batch_idx(model, range(c0, c1))` must carry
    sum(frames_per_chunk[c0:c1]) frames per branch (ValueError otherwise) and becomes ONE `ops.propagate_chunks_ragged`: chunk j
    of the run blends with the weights of ITS frame count; it takes the segment-start mask where `register_segments` is
    active and n_edits = E under `register_edits`.  A run whose chunks are of equal size issues today's ops; one-chunk
    passes are untouched (they never needed equal sizes).
    Not generalised, ValueError at a ragged run: a registered frame shard, the AdaLayerNormZero gated path, capture for
    `tokenflow_amd.graphs.GraphCache` replay (and segments together with E > 1, refused as everywhere)."""
    frames = None
    if frames_per_chunk is not None:
        frames = tuple(int(n) for n in frames_per_chunk)
        if not frames or any(n < 1 for n in frames):
            raise ValueError(f"register_chunk_frames: {list(frames)} (the frame count of every chunk, each >= 1)")
    for tb in _hook_blocks(model.unet):
        setattr(tb, "chunk_frames", frames)


def _ragged_run(module, c0: int, n_chunks: int, n_frames: int):
    """The frame counts of the chunks c0 .. c0 + n_chunks - 1 of a run pass when they are registered (register_chunk_frames)
    AND unequal, else None = today's path; the combinations that are not generalised raise."""
    frames = getattr(module, "chunk_frames", None)
    if frames is None or n_chunks == 1:
        return None
    if c0 + n_chunks > len(frames):
        raise ValueError(f"register_chunk_frames: chunks {c0}..{c0 + n_chunks - 1} of a video of {len(frames)} chunks")
    run = frames[c0:c0 + n_chunks]
    if sum(run) != n_frames:
        raise ValueError(f"register_chunk_frames: chunks {c0}..{c0 + n_chunks - 1} hold {sum(run)} frames, the pass carries "
                         f"{n_frames} per branch")
    if len(set(run)) == 1:
        return None
    if n_chunks > 64:
        raise ValueError(f"register_chunk_frames: a ragged run of {n_chunks} chunks (at most 64 per pass)")
    if module.__dict__.get("_tf_shard") is not None:
        raise ValueError("register_chunk_frames: ragged chunk runs on a registered frame shard are not supported")
    if getattr(module, "use_ada_layer_norm_zero", False):
        raise ValueError("register_chunk_frames: ragged chunk runs through the AdaLayerNormZero gated path are not supported")
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise ValueError("register_chunk_frames: a ragged chunk run cannot be captured for graphs.py replay yet")
    return run


def _ragged_weights(run, device) -> torch.Tensor:
    """One blend weight per frame of a ragged run: the cached `_blend_weights(n_j)` of every chunk, concatenated; cached per
    (frames of the run, device)."""
    key = (tuple(run), str(device))
    w = _weights_cache.get(key)
    if w is None:
        w = _weights_cache[key] = torch.cat([_blend_weights(n, device) for n in run]).contiguous()
    return w


def register_bank_window(model, radius, edits=False, anchors=None, anchor_edits=False, shard=False, anchor_shard=False,
                         edit_shard=False):
    """Sliding-window keyframe bank (no counterpart in the reference, where every keyframe attends to the whole bank): in the
    pivotal passes that follow, the uncond / cond branches of keyframe i attend to the keyframes i - radius .. i + radius only
    (clamped to the bank; `ops.bank_windows`), the source branch to its own frame as always.  Consistency stays chained along
    the clip through the overlapping windows, and the pass costs O(K * radius) frame-banks instead of K * K.  This CHANGES
    THE RESULT relative to TokenFlow and is opt-in.  Sets `bank_window` where `register_segments` sets its state: on the 16
    blocks and their `attn1`; both attention installers then call `ops.ext_attn_windows` whenever radius < K - 1.
    `None`, or a radius >= K - 1 (every window is the whole bank), issues exactly today's ops: the reference computation.
    Propagation is untouched: chunk c still blends keyframes c and c - 1.
    edits=True opens the window for a multi-edit batch (`register_edits(model, E > 1)`, with one shared schedule or
    `register_edit_schedules`): the pivotal pass is then ONE `ops.ext_attn_windows_edits` over all 1 + 2E branches -- every
    edit's bank branches attend to the windows, with the per-edit injection mask of the step.  Without the keyword a window
    in a multi-edit batch stays an error, as before.
    anchors adds global ANCHOR keyframes that every keyframe sees beside its window -- a sequence of keyframe indices, or an
    int m >= 1 for every m-th keyframe (0, m, 2m, ...); None or an empty sequence: none.  A purely local window has no global
    reference; with A anchors a keyframe attends to at most 2 radius + 1 + A keyframes, still linear in K.  Stored as
    `bank_window_anchors` beside `bank_window` and resolved against K at the pivotal pass (an index >= K is a ValueError
    there); the installers then call `ops.ext_attn_frame_sets(.., ops.bank_frame_sets(K, radius, anchors))` whenever
    radius < K - 1.  Without anchors the call is `ops.ext_attn_windows` exactly as before; with a covering radius today's
    full-bank ops are issued whatever the anchors.  This, too, is NOT TokenFlow's result.
    anchor_edits=True opens the anchors for a multi-edit batch (beside edits=True): the pivotal pass is then ONE
    `ops.ext_attn_frame_sets_edits` over all 1 + 2E branches -- every edit's bank branches attend to window plus anchors, with
    the per-edit injection mask of the step -- whenever radius < K - 1.  Without the keyword anchors in a multi-edit batch
    (edits=True, E > 1) stay an error: ValueError at the pass.
    Not generalised, ValueError at the call: `register_edits(model, E > 1)` unless edits=True, `register_segments` with several
    segments, a registered frame shard -- there the radius is held against the shard's WHOLE bank (`shard.K`), not the rank's
    local keyframes, and only a radius that covers it passes -- and, as for every multi-edit pass, graph capture
    (INTEGRATION.md section 6 shows the driver side).
    shard=True opens the window on a registered frame shard (`register_frame_shard`; long videos across GPUs): where the
    shard's type reports `K` and takes `window=` (`FrameShard`, `NativeShard`), a radius below `shard.K - 1` passes and the
    attention installers call `shard.pivotal_attention(..., window=radius)` -- every rank fetches only the keyframes within
    `radius` of its own run and computes the windowed attention of its keyframes, the result of the unsharded windowed pass.
    A radius that covers the shard's bank issues today's sharded pass.  On a windowed shard anchors, several segments and
    n_edits > 1 are a ValueError at the pass; a shard type without `window=` raises the frame-shard error above.  Without
    the keyword every refusal stays as it was.
    anchor_shard=True (beside shard=True and anchors=...) opens the anchors on a windowed frame shard: where the shard's type
    reports `supports_window_anchors`, the installers call `shard.pivotal_attention(..., window=radius, anchors=resolved)` --
    every rank fetches the keyframes within `radius` of its own run plus the anchors, at most 64 frames in all, so the cap
    K <= 64 of the single-GPU frame-set call does not hold there.  The anchors resolve against the shard's WHOLE bank: an int
    stride m gives range(0, shard.K, m), an index >= shard.K is a ValueError at the pass.  Without the keyword anchors on a
    windowed shard stay the ValueError they were.
    edit_shard=True (beside shard=True and edits=True; with anchors also anchor_edits=True and anchor_shard=True) opens a
    MULTI-EDIT batch on a windowed frame shard: where the shard's type reports `supports_window_edits` and the shard was built
    with `window_edits=True` (`FrameShard`, `NativeEditShard`), the installers call `shard.pivotal_attention(..., n_edits=E,
    inject_mask=<the step's mask>, window=radius, anchors=resolved)` -- one sharded pass for all prompts, the masks of
    `register_edit_schedules` included.  Without the keyword n_edits > 1 on a windowed shard stays the ValueError it was."""
    if radius is not None:
        radius = int(radius)
        if radius < 0:
            raise ValueError(f"register_bank_window: radius={radius} (>= 0, or None for the whole bank)")
    if anchors is not None and not isinstance(anchors, bool) and isinstance(anchors, int):
        if anchors < 1:
            raise ValueError(f"register_bank_window: anchors={anchors} (every m-th keyframe: m >= 1)")
    elif anchors is not None:
        try:
            anchors = tuple(anchors)
            bad = [a for a in anchors if isinstance(a, bool) or int(a) != a or int(a) < 0]
        except (TypeError, ValueError):
            bad = [anchors]
        if bad:
            raise ValueError(f"register_bank_window: anchors={anchors!r} (keyframe indices >= 0, an int m >= 1 for every m-th "
                             "keyframe, or None)")
        anchors = tuple(int(a) for a in anchors) or None
    _set_bank_window(_hook_blocks(model.unet), radius, bool(edits) and radius is not None,
                     anchors if radius is not None else None, bool(anchor_edits) and radius is not None,
                     bool(shard) and radius is not None, bool(anchor_shard) and radius is not None,
                     bool(edit_shard) and radius is not None)


def _set_bank_window(blocks, radius, edits=False, anchors=None, anchor_edits=False, shard=False, anchor_shard=False,
                     edit_shard=False):
    """`bank_window` (`bank_window_edits`, the multi-edit opt-in, `bank_window_anchors`: a tuple of keyframe indices, an
    int stride or None, and `bank_window_anchor_edits`, the opt-in of anchors in a multi-edit batch) on transformer blocks
    and their `attn1` (register_bank_window; tools on a bare block list)."""
    for tb in blocks:
        for m in (tb, tb.attn1):
            setattr(m, "bank_window", radius)
            setattr(m, "bank_window_edits", edits)
            setattr(m, "bank_window_anchor_edits", anchor_edits)
            setattr(m, "bank_window_anchors", anchors)
            setattr(m, "bank_window_shard", shard)      # the opt-in of a window on a registered frame shard
            setattr(m, "bank_window_anchor_shard", anchor_shard)      # ... and of anchors beside it
            setattr(m, "bank_window_edit_shard", edit_shard)      # ... and of a multi-edit batch on it


def _bank_window(module, K: int):
    """The window radius of the pivotal pass of K keyframes a module sees (register_bank_window), or None = the whole bank;
    the combinations that are not generalised raise.  On a registered frame shard the pass carries the rank's LOCAL keyframes:
    the radius is held against the shard's whole bank (`shard.K`), and refused where that is not known."""
    radius = getattr(module, "bank_window", None)
    if radius is None:
        return None
    shard = _active_shard(module)   # the predicate of the attention path: a world-1 shard is the unsharded pass
    if shard is not None:
        K_all = getattr(shard, "K", None)
        if K_all is not None and radius >= int(K_all) - 1:
            return None
        if K_all is None or not getattr(module, "bank_window_shard", False) or not getattr(shard, "supports_window", False):
            raise ValueError("register_bank_window: a sliding-window bank on a registered frame shard is not supported")
        # the opt-in (register_bank_window(..., shard=True)): the shard runs the windowed pass; what it does not generalise
        if int(getattr(module, "n_edits", 1)) > 1 and not (
                getattr(module, "bank_window_edits", False) and getattr(module, "bank_window_edit_shard", False)
                and getattr(shard, "supports_window_edits", False) and getattr(shard, "window_edits", False)):
            raise ValueError("register_bank_window: a sliding-window bank on a registered frame shard runs one edit "
                             "(register_edits, n_edits > 1 is not supported there)")
        if getattr(module, "bank_window_anchors", None) is not None and not (
                getattr(module, "bank_window_anchor_shard", False) and getattr(shard, "supports_window_anchors", False)):
            raise ValueError("register_bank_window: anchor keyframes on a registered frame shard are not supported (every "
                             "rank would have to hold the anchors)")
        if getattr(module, "keyframe_segments", None) is not None:
            raise ValueError("register_bank_window: a sliding-window bank in a pass of several keyframe segments "
                             "(register_segments) is not supported")
        return radius
    if radius >= K - 1:
        return None
    if int(getattr(module, "n_edits", 1)) > 1 and not getattr(module, "bank_window_edits", False):
        raise ValueError("register_bank_window: a sliding-window bank in a multi-edit batch (register_edits, n_edits > 1) is "
                         "opt-in: register_bank_window(model, radius, edits=True)")
    if getattr(module, "keyframe_segments", None) is not None:
        raise ValueError("register_bank_window: a sliding-window bank in a pass of several keyframe segments "
                         "(register_segments) is not supported")
    return radius


def _bank_anchors(module, K: int):
    """The anchor keyframes of a windowed pivotal pass of K keyframes (register_bank_window(anchors=...)) as a tuple of
    indices, or None: call where `_bank_window(module, K)` has returned a radius.  The combination that is not generalised and
    an index outside the pass raise."""
    anchors = getattr(module, "bank_window_anchors", None)
    if anchors is None:
        return None
    if int(getattr(module, "n_edits", 1)) > 1 and not getattr(module, "bank_window_anchor_edits", False):
        raise ValueError("register_bank_window: anchor keyframes in a multi-edit batch (register_edits, n_edits > 1) are "
                         "opt-in: register_bank_window(model, radius, edits=True, anchors=..., anchor_edits=True)")
    shard = _active_shard(module)
    if shard is not None:      # (register_bank_window(..., anchor_shard=True)): K is the rank's local count; the anchors are global
        K_all = int(shard.K)
        if isinstance(anchors, int):
            return tuple(range(0, K_all, anchors))
        if max(anchors) >= K_all:
            raise ValueError(f"register_bank_window: anchors={list(anchors)} on a frame shard of {K_all} keyframes "
                             f"(indices < {K_all})")
        return anchors
    if isinstance(anchors, int):
        return tuple(range(0, K, anchors))
    if max(anchors) >= K:
        raise ValueError(f"register_bank_window: anchors={list(anchors)} in a pivotal pass of {K} keyframes (indices < {K})")
    return anchors


_latents_cache = collections.OrderedDict()
_LATENTS_CACHE_ENTRIES = 2      # the current timestep's file (+ one): the driver loads the SAME file C+1 times per step


def load_source_latents_t(t, latents_path):
    """tokenflow_utils.py:43-47.  The reference re-reads the file on each of the C+1 calls of a denoising step
    (run_tokenflow_pnp.py:198,221); here the most recent files are kept, keyed by (path, mtime) -- a bounded
    LRU, so nothing but the current timestep's latents stays resident."""
    latents_t_path = os.path.join(latents_path, f"noisy_latents_{t}.pt")
    assert os.path.exists(latents_t_path), f"Missing latents at t {t} path {latents_t_path}"
    key = (latents_t_path, os.path.getmtime(latents_t_path))
    hit = _latents_cache.get(key)
    if hit is None:
        hit = torch.load(latents_t_path)
        _latents_cache[key] = hit
        while len(_latents_cache) > _LATENTS_CACHE_ENTRIES:
            _latents_cache.popitem(last=False)
    else:
        _latents_cache.move_to_end(key)
    return hit


# --------------------------------------------------------------------------- schedules
def _schedule_set(schedule):
    """One-time conversion so that `t in schedule` never syncs the device."""
    if schedule is None:
        return None
    if isinstance(schedule, torch.Tensor):
        return set(schedule.detach().cpu().reshape(-1).tolist())
    return set(float(s) if isinstance(s, torch.Tensor) else s for s in schedule)


def _injecting(module) -> bool:
    """`schedule is not None and (t in schedule or t == 1000)` (tokenflow_utils.py:86,124)."""
    sched = module.__dict__.get("_tf_schedule_set")
    if module.injection_schedule is None or sched is None:
        return False
    t = module.t
    if isinstance(t, torch.Tensor):
        t = t.item()
    return t in sched or t == 1000


def _set_schedule(module, injection_schedule):
    setattr(module, "injection_schedule", injection_schedule)
    module.__dict__["_tf_schedule_set"] = _schedule_set(injection_schedule)
    module.__dict__.pop("_tf_edit_schedule_sets", None)      # an installer starts from the one shared schedule


def _inject_mask(module, n_edits: int) -> int:
    """The edits that inject at the module's `t`, bit e = edit e: with per-edit schedules (register_edit_schedules) each edit's
    own `t in schedule or t == 1000`; without them the one shared state `_injecting(module)` for every edit."""
    sets = module.__dict__.get("_tf_edit_schedule_sets")
    if sets is None:
        return (1 << n_edits) - 1 if _injecting(module) else 0
    if len(sets) != n_edits:
        raise ValueError(f"register_edit_schedules: {len(sets)} schedules on a module that sees {n_edits} edits "
                         "(call it after register_edits)")
    t = module.t
    if isinstance(t, torch.Tensor):
        t = t.item()
    return sum(1 << e for e, sched in enumerate(sets) if sched is not None and (t in sched or t == 1000))


def register_edit_schedules(model, qk_schedules=None, conv_schedules=None):
    """Multi-edit extension: the edits of one pass may differ in their injection thresholds (PnP's pnp_attn_t / pnp_f_t, the
    driver's qk_injection_timesteps / conv_injection_timesteps).  Each argument is a list of n_edits injection schedules in
    the form the installers take (tensor or sequence of timesteps); `[]` or None inside the list = that edit never injects.
    Call it after register_extended_attention_pnp, register_conv_injection and register_edits.
      qk_schedules   -> `attn1` of the 8 decoder blocks that inject (the other blocks keep their empty schedule);
      conv_schedules -> up_blocks[1].resnets[1].
    At a call the hook computes the mask of the edits that inject at `t` (per edit: `t in schedule or t == 1000`, sets
    converted once, no host sync): no edit -> today's call without injection, every edit -> today's call with it, anything
    else -> the same op with `inject_mask=` / `edit_mask=`.  For every op the slices of edit e are what the single-edit op
    computes on [source | uncond_e | cond_e] with edit e's own schedule.  None for an argument removes that kind's per-edit
    schedules (the installer's shared schedule holds again); re-running an installer removes them on the modules it touches;
    the SDEdit installer (register_extended_attention) never injects and ignores them.  On a registered `FrameShard` the
    mask of a call goes to `shard.pivotal_attention(..., n_edits=E, inject_mask=mask)`."""
    unet = model.unet

    def sets_for(what, schedules, module):
        if schedules is None:
            return None
        schedules = list(schedules)
        E = int(getattr(module, "n_edits", 1))
        if len(schedules) != E:
            raise ValueError(f"register_edit_schedules: {len(schedules)} {what} schedules for n_edits={E}")
        sets = [_schedule_set(sch) for sch in schedules]
        return [sch if sch else None for sch in sets]

    def put(module, sets):
        if sets is None:
            module.__dict__.pop("_tf_edit_schedule_sets", None)
        else:
            module.__dict__["_tf_edit_schedule_sets"] = sets

    attns = [unet.up_blocks[res].attentions[b].transformer_blocks[0].attn1 for res, blocks in _INJECTED_UP.items() for b in blocks]
    conv_module = unet.up_blocks[1].resnets[1]
    qk_sets = [sets_for("qk", qk_schedules, m) for m in attns]       # validate everything before anything is set
    conv_sets = sets_for("conv", conv_schedules, conv_module)
    for m, sets in zip(attns, qk_sets):
        put(m, sets)
    put(conv_module, conv_sets)


# --------------------------------------------------------------------------- PnP feature injection
def register_conv_injection(model, injection_schedule):
    """tokenflow_utils.py:49-104.  The reference REPLACES `up_blocks[1].resnets[1].forward` by a transcription of
    diffusers' `ResnetBlock2D.forward` (51-98) with two slice copies behind `conv2` (86-91) -- and inherits that
    version's signature and body.  Here the module keeps ITS OWN forward, whatever diffusers release wrote it, and a
    forward hook on its `conv2` overwrites the uncond / cond activations with the source branch's on conv2's output:
    the same point of the data flow (after conv2, in front of the shortcut add), one broadcast-copy launch
    (`ops.inject_copy_`), same schedule semantics (`t in schedule or t == 1000`, 86).  Installing twice replaces the
    previous hook."""
    conv_module = model.unet.up_blocks[1].resnets[1]

    def after_conv2(_conv2, _inputs, hidden_states):
        E = int(getattr(conv_module, "n_edits", 1))
        mask = _inject_mask(conv_module, E)
        if mask:
            if not hidden_states.is_contiguous():
                hidden_states = hidden_states.contiguous()
            E = _n_edits(conv_module)
            if E == 1:
                ops.inject_copy_(hidden_states)
            elif mask == (1 << E) - 1:   # every edit's uncond and cond branch takes the source branch's activations
                ops.inject_copy_edits_(hidden_states, E)
            else:                        # per-edit schedules that disagree at this step: only the edits that inject
                ops.inject_copy_edits_(hidden_states, E, edit_mask=mask)
        return hidden_states

    prev = conv_module.__dict__.pop("_tf_conv_hook", None)
    if prev is not None:
        prev.remove()
    conv_module.__dict__["_tf_conv_hook"] = conv_module.conv2.register_forward_hook(after_conv2)
    _set_schedule(conv_module, injection_schedule)


# --------------------------------------------------------------------------- extended attention
_announced = False


def _announce():
    """One line on stderr the first time a hook is installed: a run that silently picked up the reference's own
    `tokenflow_utils.py` (the script directory precedes PYTHONPATH on sys.path) never prints it."""
    global _announced
    if _announced:
        return
    _announced = True
    from . import _lib
    lib = _lib.load()                    # fails loudly here, at installation time, if the library is missing
    msg = f"[tokenflow_amd] MI355X HIP hook path active ({_lib.LIB_PATH}, ABI v{lib.tf_abi_version()})"
    logging.getLogger("tokenflow_amd").info(msg)
    if os.environ.get("TOKENFLOW_QUIET", "0") in ("", "0"):
        print(msg, file=sys.stderr, flush=True)


def _fused_qkv(attn, x: torch.Tensor):
    """q, k, v of a self-attention as column slabs of ONE projection `x @ [Wq; Wk; Wv]^T` (row f2 of SURVEY.md
    section 8; tokenflow_utils.py:120-122 issues three Linear calls): one GEMM, one output [3K, S, 3D] that the
    attention kernel reads in place through its row stride, no per-tensor dtype casts.  The concatenated weight is
    cached on the module, keyed by the three weights' storage, version counter and the compute dtype, so an
    optimizer step, a `.to()` or an in-place LoRA merge rebuilds it.  (An edit THROUGH `.data` -- `w.data.add_(d)` --
    bumps no version counter: call `invalidate_fused_qkv(model)` after one.)  Returns None when the three
    projections are not plain bias-compatible `nn.Linear` layers over the same input, or when autograd is recording
    and a weight requires grad (then the caller issues them one by one).
    Returns the [..., 3D] projection output; q, k, v are its three D-wide column slabs."""
    lq, lk, lv = attn.to_q, attn.to_k, attn.to_v
    Linear = torch.nn.Linear
    if not (type(lq) is Linear and type(lk) is Linear and type(lv) is Linear and x.is_cuda):
        return None
    wq, wk, wv = lq.weight, lk.weight, lv.weight
    if not (wq.shape == wk.shape == wv.shape and wq.dtype == wk.dtype == wv.dtype and wq.shape[1] == x.shape[-1]):
        return None
    biases = (lq.bias, lk.bias, lv.bias)
    if any(b is None for b in biases) != all(b is None for b in biases):
        return None
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (wq, wk, wv) + biases):
        return None      # the cached concatenation is built without autograd: training keeps the three Linear calls
    if torch.is_autocast_enabled("cuda"):
        cdt = torch.get_autocast_dtype("cuda")
    else:
        cdt = x.dtype if x.dtype == wq.dtype else None
    if cdt is None:
        return None
    key = (cdt, wq.data_ptr(), wk.data_ptr(), wv.data_ptr(), wq._version, wk._version, wv._version,
           None if biases[0] is None else tuple((b.data_ptr(), b._version) for b in biases))
    cached = attn.__dict__.get("_tf_qkv_cache")
    if cached is None or cached[0] != key:
        with torch.no_grad():
            wcat = torch.cat([wq, wk, wv], dim=0).to(cdt).contiguous()
            bcat = None if biases[0] is None else torch.cat(list(biases), dim=0).to(cdt).contiguous()
        cached = (key, wcat, bcat)
        attn.__dict__["_tf_qkv_cache"] = cached
    _, wcat, bcat = cached
    with torch.autocast("cuda", enabled=False):
        qkv = torch.nn.functional.linear(x.to(cdt), wcat, bcat)
    return qkv


FUSE_QKV = os.environ.get("TOKENFLOW_FUSED_QKV", "1") not in ("", "0")


def invalidate_fused_qkv(model: torch.nn.Module) -> None:
    """Drop every cached [Wq;Wk;Wv] of `model` (needed only after weight edits that bypass the version counters)."""
    for m in model.modules():
        m.__dict__.pop("_tf_qkv_cache", None)


def _make_sa_forward(self, pnp: bool):
    to_out = self.to_out
    if type(to_out) is torch.nn.modules.container.ModuleList:
        to_out = self.to_out[0]          # dropout to_out[1] skipped, as 108-112

    def forward(x, encoder_hidden_states=None, attention_mask=None):
        is_cross = encoder_hidden_states is not None
        qkv = _fused_qkv(self, x) if (FUSE_QKV and not is_cross) else None
        if qkv is not None:
            proj_dtype = qkv.dtype
            cdt = ops.compute_dtype(qkv)
            if proj_dtype != cdt:        # fp32 model without autocast: ONE cast of the fused output
                qkv = qkv.to(cdt)
            D = qkv.shape[-1] // 3
            q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]     # column slabs, row stride 3D
        else:
            encoder_hidden_states = encoder_hidden_states if is_cross else x
            q, k, v = self.to_q(x), self.to_k(encoder_hidden_states), self.to_v(encoder_hidden_states)
            proj_dtype = q.dtype
            cdt = ops.compute_dtype(q)
            if proj_dtype != cdt:
                q, k, v = q.to(cdt), k.to(cdt), v.to(cdt)
        shard = None if is_cross else _active_shard(self)
        E = 1 if is_cross else _n_edits(self)
        # (a window excludes segments, and edits and shards unless opted in; the pass carries q.shape[0] / (1 + 2E) keyframes)
        radius = None if is_cross else _bank_window(self, q.shape[0] // (1 + 2 * E))
        anchors = None if radius is None else _bank_anchors(self, q.shape[0] // (1 + 2 * E))
        segs = None if is_cross else _segments(self, q.shape[0] // 3)
        # the edits that inject (one shared schedule: all or none; register_edit_schedules: each edit's own)
        mask = _inject_mask(self, E) if pnp else 0
        inject = mask != 0
        if shard is not None:     # q, k, v are this rank's keyframes; the bank is everybody's (register_frame_shard)
            if E > 1 and radius is not None:   # register_bank_window(..., edit_shard=True): all prompts in ONE windowed pass
                _need_edit_shard(shard)
                out = shard.pivotal_attention(q, k, v, self.heads, self.scale, False, n_edits=E, inject_mask=mask,
                                              window=radius, anchors=anchors)
            elif E > 1:
                _need_edit_shard(shard)
                out = shard.pivotal_attention(q, k, v, self.heads, self.scale, False, n_edits=E, inject_mask=mask)
            elif radius is not None:   # register_bank_window(..., shard=True): the rank's keyframes against their windows
                if anchors is not None:   # ... plus the global anchors (anchor_shard=True)
                    out = shard.pivotal_attention(q, k, v, self.heads, self.scale, inject, window=radius, anchors=anchors)
                else:
                    out = shard.pivotal_attention(q, k, v, self.heads, self.scale, inject, window=radius)
            else:
                out = shard.pivotal_attention(q, k, v, self.heads, self.scale, inject)
        elif anchors is not None and E > 1:   # ... several prompts with anchors: every edit's bank branches read the frame sets
            out = ops.ext_attn_frame_sets_edits(q, k, v, self.heads, self.scale, False, E,
                                                ops.bank_frame_sets(q.shape[0] // (1 + 2 * E), radius, anchors),
                                                inject_mask=mask)
        elif radius is not None and E > 1:   # ... several prompts on a long video: every edit's bank branches read the windows
            out = ops.ext_attn_windows_edits(q, k, v, self.heads, self.scale, False, E,
                                             ops.bank_windows(q.shape[0] // (1 + 2 * E), radius), inject_mask=mask)
        elif anchors is not None:   # ... and to the global anchor keyframes (E = 1)
            out = ops.ext_attn_frame_sets(q, k, v, self.heads, self.scale, inject,
                                          ops.bank_frame_sets(q.shape[0] // 3, radius, anchors))
        elif radius is not None:  # long videos: a bank branch attends to the neighbouring keyframes only
            out = ops.ext_attn_windows(q, k, v, self.heads, self.scale, inject, ops.bank_windows(q.shape[0] // 3, radius))
        elif segs is not None:    # several scenes or clips: a bank branch attends to the keyframes of its own segment
            out = ops.ext_attn_segments(q, k, v, self.heads, self.scale, inject, segs)
        elif E == 1:
            out = ops.ext_attn(q, k, v, self.heads, self.scale, inject)
        elif mask in (0, (1 << E) - 1):   # [source | uncond_1 | cond_1 | ...]: the source branch and (injecting) the scores once
            out = ops.ext_attn_edits(q, k, v, self.heads, self.scale, inject, E)
        else:                     # per-edit schedules that disagree at this step
            out = ops.ext_attn_edits(q, k, v, self.heads, self.scale, False, E, inject_mask=mask)
        return to_out(out if out.dtype == proj_dtype else out.to(proj_dtype))

    return forward


def register_extended_attention_pnp(model, injection_schedule):
    """tokenflow_utils.py:106-214: every BasicTransformerBlock.attn1 gets the extended
    attention with an empty schedule (203-206); the 8 decoder blocks
    up_blocks[1].attentions[1,2], up_blocks[2,3].attentions[0..2] get the real one (208-214)."""
    _announce()
    for _, module in model.unet.named_modules():
        if isinstance_str(module, "BasicTransformerBlock"):
            module.attn1.forward = _make_sa_forward(module.attn1, pnp=True)
            _set_schedule(module.attn1, [])
    for res, blocks in _INJECTED_UP.items():
        for block in blocks:
            module = model.unet.up_blocks[res].attentions[block].transformer_blocks[0].attn1
            module.forward = _make_sa_forward(module, pnp=True)
            _set_schedule(module, injection_schedule)


def register_extended_attention(model):
    """tokenflow_utils.py:216-294 (SDEdit driver): extended attention, never injects."""
    _announce()
    for _, module in model.unet.named_modules():
        if isinstance_str(module, "BasicTransformerBlock"):
            module.attn1.forward = _make_sa_forward(module.attn1, pnp=False)
    for res, blocks in _INJECTED_UP.items():
        for block in blocks:
            module = model.unet.up_blocks[res].attentions[block].transformer_blocks[0].attn1
            module.forward = _make_sa_forward(module, pnp=False)


# --------------------------------------------------------------------------- TokenFlow block
_weights_cache = {}


def _blend_weights(n: int, device) -> torch.Tensor:
    """w1 of tokenflow_utils.py:375-383.  s - p1 = j - n//2 and s - p2 = j + n - n//2 do not
    depend on the chunk index, so the n-vector is computed once per (n, device) with the
    reference's own torch ops (on the host, so the value is the CPU reference's)."""
    key = (n, str(device))
    w = _weights_cache.get(key)
    if w is None:
        s = torch.arange(0, n)
        d1 = torch.abs(s - n // 2)
        d2 = torch.abs(s + n - n // 2)
        w = torch.sigmoid(d2 / (d1 + d2)).to(device)
        _weights_cache[key] = w
    return w


def _fused_norm_dtype(mod: torch.nn.Module, x: torch.Tensor, in_dtype=None):
    """The 16-bit dtype in which a plain LayerNorm of the block can be produced directly by
    `ops.layer_norm` (one pass instead of torch's autocast sequence cast-up / fp32 norm / cast-down in front
    of the next Linear), or None: keep the module call (fp32 models, AdaLayerNorm, CPU tensors).
    in_dtype: dtype of the norm's input when it is not x's (the residual-add form normalises `a + x`)."""
    D = x.shape[-1]
    in_dtype = x.dtype if in_dtype is None else in_dtype
    if (type(mod) is not torch.nn.LayerNorm or not x.is_cuda or tuple(mod.normalized_shape) != (D,)
            or D % 8 or D > 2048 or in_dtype not in (torch.float32, torch.bfloat16, torch.float16)):
        return None
    if torch.is_autocast_enabled("cuda"):
        dt = torch.get_autocast_dtype("cuda")
        return dt if dt in (torch.bfloat16, torch.float16) else None
    if in_dtype != torch.float32 and (mod.weight is None or mod.weight.dtype == in_dtype):
        return in_dtype
    return None


# Which LayerNorms of a block go through `ops.layer_norm`:  "all" (default) = norm1 -- the producer of the attention
# input, the NN-search rows and the pivots' inverse norms (row f2 of SURVEY.md section 8) -- and also norm2 / norm3,
# whose only consumers are Linear layers (attn2.to_q, the feed-forward): under autocast torch evaluates layer_norm
# in fp32 and the Linear rounds its input to 16 bit, so the kernel's single rounding of the fp32 result IS the value
# the reference's Linear sees (pinned by tests/test_fullsize_gpu.py::test_fused_layer_norm_is_the_autocast_value);
# "norm1" = only norm1; "none" = always the modules.
FUSE_NORMS = os.environ.get("TOKENFLOW_FUSED_NORMS", "all")
# TOKENFLOW_FUSED_GATHER_NORM=0: keep the propagation's gather and the norm behind it as two launches
FUSE_GATHER_NORM = os.environ.get("TOKENFLOW_FUSED_GATHER_NORM", "1") not in ("", "0")
# TOKENFLOW_NORM1_ALL_BRANCHES=1: a propagation pass normalises all three branches as the reference does (323) although
# only the source branch is read (335-343); default: the source branch alone (A/B: profiles/r05_hooks_bench.txt)
NORM1_ALL_BRANCHES = os.environ.get("TOKENFLOW_NORM1_ALL_BRANCHES", "0") not in ("", "0")


def _block_norm(mod: torch.nn.Module, x: torch.Tensor, want_inv_norm: bool = False, which: str = "norm1", dest=None):
    """(LayerNorm(x), 1/||row|| or None) through the fused kernel when it applies, else the module itself.
    dest(dtype) -> (out, inv_out): destination tensors for the fused kernel (the sharded pivotal pass hands out views
    of the block's halo-extended state, so that the norm writes the pivots and their inverse norms in place)."""
    dt = _fused_norm_dtype(mod, x) if (FUSE_NORMS == "all" or FUSE_NORMS == which) else None
    if dt is None:
        return mod(x), None
    out, inv_out = dest(dt) if dest is not None else (None, None)
    return ops.layer_norm(x, mod.weight, mod.bias, mod.eps, dt, want_inv_norm, out=out, inv_out=inv_out)


def _need_edit_shard(shard):
    """A multi-edit batch needs a shard type that runs one (`FrameShard.supports_edits`; the native rank executor's
    tf_rank_pivotal is single-edit)."""
    if not getattr(type(shard), "supports_edits", False):
        raise ValueError(f"register_edits: a multi-edit batch (n_edits > 1) on a registered frame shard of type "
                         f"{type(shard).__name__} is not supported (FrameShard runs one; the native executor does not)")


def _shard_state(block, shard, S: int, D: int, dtype, device, nbr: int = 3):
    """The block's halo-extended propagation state on a sharded rank, allocated ONCE per block and shape and reused
    step after step (a step's chunk passes are done with it before the next pivotal pass writes it):
      (nbr = 3 branches, or the 1 + 2E of a multi-edit batch)
      norm [1 + 3*Kl, S, D]   slot 0 = the left neighbour's last keyframe, then norm1's output of the pivotal pass,
                              branch-major -- so the first Kl + 1 slots ARE the halo-extended pivots, written by the
                              norm itself;
      inv  [1 + 3*Kl, S]      the same for the rows' inverse norms;
      kfo  [3, Kl + 1, S, D]  cached attention output (after to_out) with the neighbour's slot in front."""
    key = (shard.Kl, S, D, dtype, device) if nbr == 3 else (shard.Kl, S, D, dtype, device, nbr)
    st = block.__dict__.get("_tf_shard_state")
    if st is None or st[0] != key:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            # the state outlives any one graph (the pivotal pass writes it, every chunk pass of the step reads it, eager
            # passes reuse it): it must not come from a capture's private pool
            raise RuntimeError("register_frame_shard: the per-block propagation state would be allocated inside a HIP-graph "
                               "capture; run one eager pivotal pass first (GraphCache(warmup >= 1) does)")
        Kl = shard.Kl
        st = (key, torch.empty(1 + nbr * Kl, S, D, dtype=dtype, device=device),
              torch.empty(1 + nbr * Kl, S, dtype=torch.float32, device=device),
              torch.empty(nbr, Kl + 1, S, D, dtype=dtype, device=device))
        block.__dict__["_tf_shard_state"] = st
    return st[1], st[2], st[3]


def _add_norm(mod: torch.nn.Module, a: torch.Tensor, h: torch.Tensor, which: str):
    """(a + h, LayerNorm(a + h)): the residual add of the block and the norm that follows it
    (`hidden_states = attn_output + hidden_states` then norm2 / norm3, tokenflow_utils.py:396-403, 409-414) in one
    pass through `ops.add_layer_norm` when the norm is fusable, else the two torch ops.  Bit-identical either way."""
    if a.shape == h.shape and a.is_cuda and h.is_cuda and (FUSE_NORMS == "all" or FUSE_NORMS == which):
        dt = _fused_norm_dtype(mod, h, torch.promote_types(a.dtype, h.dtype))
        if dt is not None:
            return ops.add_layer_norm(a, h, mod.weight, mod.bias, mod.eps, dt)
    total = a + h
    return total, _block_norm(mod, total, which=which)[0]


def _chunk_run(batch_idx):
    """(first chunk, number of chunks) of a `batch_idx` state.  The reference sets an int (one chunk of
    n = batch_size frames per UNet pass, run_tokenflow_pnp.py:228-231).  Extension for large-memory GPUs: a
    `range` / list of CONSECUTIVE chunk indices means the pass carries all those chunks, frames chunk-major
    inside every branch -- one UNet pass over the whole video instead of C passes."""
    if isinstance(batch_idx, (range, list, tuple)):
        ids = [int(i) for i in batch_idx]
        if not ids or any(b - a != 1 for a, b in zip(ids, ids[1:])):
            raise ValueError(f"batch_idx {batch_idx!r}: need a non-empty run of consecutive chunk indices")
        return ids[0], len(ids)
    return int(batch_idx), 1


def make_tokenflow_attention_block(block_class: Type[torch.nn.Module]) -> Type[torch.nn.Module]:
    """tokenflow_utils.py:296-429."""

    class TokenFlowBlock(block_class):

        @property
        def pivot_hidden_states(self):
            """`norm1` output of the last pivotal pass (tokenflow_utils.py:327), in the dtype the reference caches."""
            st = self.__dict__.get("_tf_pivot_hidden")
            if st is None:
                raise AttributeError("pivot_hidden_states: no pivotal pass has run")
            t, dt = st
            return t if t.dtype == dt else t.to(dt)

        @pivot_hidden_states.setter
        def pivot_hidden_states(self, value):
            self.__dict__["_tf_pivot_hidden"] = (value, value.dtype)

        @property
        def attn_output(self):
            """What the reference leaves in `self.attn_output`: the attention output after a pivotal pass (355-360), the
            SELECTED keyframe outputs `kf_attn_output.view(3, K, S, D)[:, batch_idxs]` after a propagation pass (361-363;
            gated under AdaLayerNormZero, 364-365).  Nothing on the path reads the second form -- the gather indexes the
            cached output in place -- so it is built only if somebody asks."""
            st = self.__dict__.get("_tf_attn_output")
            if st is None:
                raise AttributeError("attn_output: no pass has run")
            if callable(st):
                st = st()
                self.__dict__["_tf_attn_output"] = st
            return st

        @attn_output.setter
        def attn_output(self, value):
            self.__dict__["_tf_attn_output"] = value

        def forward(self, hidden_states, attention_mask=None, encoder_hidden_states=None,
                    encoder_attention_mask=None, timestep=None, cross_attention_kwargs=None,
                    class_labels=None) -> torch.Tensor:
            batch_size, sequence_length, dim = hidden_states.shape
            E = _n_edits(self)
            nbr = 1 + 2 * E         # branches: [source | uncond | cond], or the multi-edit batch of register_edits
            _segments(self)         # register_segments: the combinations that are not generalised raise here
            if E > 1:
                if self.__dict__.get("_tf_shard") is not None:
                    _need_edit_shard(self.__dict__["_tf_shard"])
                if self.use_ada_layer_norm_zero:
                    raise ValueError("register_edits: a multi-edit batch (n_edits > 1) through the AdaLayerNormZero gated path "
                                     "is not supported")
                if batch_size % nbr:
                    raise ValueError(f"register_edits: batch of {batch_size} does not hold {nbr} branches ({E} edits)")
            n_frames = batch_size // nbr
            if not self.pivotal_pass and getattr(self, "chunk_frames", None) is not None:
                _ragged_run(self, *_chunk_run(self.batch_idx), n_frames)   # register_chunk_frames: the refusals, up front
            if self.pivotal_pass:
                # register_bank_window: the combinations that are not generalised raise here
                if _bank_window(self, n_frames) is not None:
                    _bank_anchors(self, n_frames)
            hidden_states = hidden_states.view(nbr, n_frames, sequence_length, dim)

            norm_inv = None
            gate_msa = None
            pending = None          # a residual branch output not yet added to hidden_states (see _add_norm)
            prenorm = None          # (which, tensor): the next norm, already produced by the propagation's gather
            if self.use_ada_layer_norm:
                norm_hidden_states = self.norm1(hidden_states, timestep)
            elif self.use_ada_layer_norm_zero:
                norm_hidden_states, gate_msa, shift_mlp, scale_mlp, gate_mlp = self.norm1(
                    hidden_states, timestep, class_labels, hidden_dtype=hidden_states.dtype)
            else:   # row f2: LayerNorm emits the 16-bit rows the kernels read (+ the pivots' inverse norms)
                dest = None
                shard0 = _active_shard(self) if self.pivotal_pass else None
                if shard0 is not None and n_frames == shard0.Kl and hidden_states.is_cuda:
                    # a neighbour halo of the PREVIOUS pivotal pass may still be in flight if no chunk pass (and no
                    # join_frame_shard) consumed it: its send reads, and its receive writes, the state this pass is
                    # about to overwrite -- order behind it first
                    prev = self.__dict__.get("_tf_halo")
                    if prev is not None and prev[3]:
                        shard0.halo_wait(prev[3])
                        self.__dict__["_tf_halo"] = (prev[0], prev[1], prev[2], [])
                    # sharded pivotal pass: norm1 writes straight into the block's halo-extended state
                    def dest(dt, _s=shard0):
                        nb, ib, _ = _shard_state(self, _s, sequence_length, dim, dt, hidden_states.device, nbr)
                        return nb[1:].view(nbr, n_frames, sequence_length, dim), ib[1:].view(nbr, n_frames, sequence_length)
                if self.pivotal_pass or NORM1_ALL_BRANCHES:
                    norm_hidden_states, norm_inv = _block_norm(self.norm1, hidden_states, bool(self.pivotal_pass), dest=dest)
                else:
                    # a propagation pass reads norm1's output of the SOURCE branch only (the NN-search targets,
                    # 335-343; the reference normalises all three branches at 323 and drops two): one third of the
                    # launch's bytes.  Row-wise op: the rows that are computed are bit-identical.
                    norm_hidden_states, norm_inv = _block_norm(self.norm1, hidden_states[:1])[0], None
            norm_hidden_states = norm_hidden_states.view(-1, n_frames, sequence_length, dim)

            cross_attention_kwargs = cross_attention_kwargs if cross_attention_kwargs is not None else {}
            if self.pivotal_pass:
                # 326-327 + 352-360: cache the normalised features and the attention output
                # the reference caches what norm1 returns (327): fp32 under autocast, where torch evaluates
                # layer_norm in fp32.  The fused norm emitted 16-bit rows; the attribute keeps the reference's
                # dtype and is widened only if somebody reads it (nothing on the path does: the NN search reads
                # _tf_pivots / _tf_pivot_inv_norm)
                self._tf_pivot_hidden = (norm_hidden_states,
                                         torch.float32 if (norm_inv is not None and torch.is_autocast_enabled("cuda"))
                                         else norm_hidden_states.dtype)
                src = norm_hidden_states[0]
                self._tf_pivots = src.to(ops.compute_dtype(src)).contiguous()       # [K,S,D] 16-bit
                self._tf_pivot_inv_norm = (norm_inv.view(nbr, n_frames, sequence_length)[0] if norm_inv is not None
                                           else ops.pivot_inv_norm(self._tf_pivots))   # [K,S] fp32
                shard = _active_shard(self)
                inplace = False
                if shard is not None:
                    if n_frames != shard.Kl:
                        raise ValueError(f"pivotal pass with {n_frames} keyframes per branch on a rank that owns "
                                         f"{shard.Kl} (register_frame_shard)")
                    st = self.__dict__.get("_tf_shard_state")
                    # in place: norm1 has written the pivots and inverse norms into slots 1.. of the halo-extended
                    # state (the fused LayerNorm path); else (AdaLayerNorm, fp32 models) the two-exchange form, whose
                    # pivots' half does not depend on the attention and travels under it
                    inplace = (norm_inv is not None and st is not None
                               and norm_hidden_states.data_ptr() == st[1][1:].data_ptr())
                    if not inplace:
                        halo = shard.halo_start(self._tf_pivots, self._tf_pivot_inv_norm.contiguous())
                self.attn_output = self.attn1(
                    norm_hidden_states.view(batch_size, sequence_length, dim),
                    encoder_hidden_states=encoder_hidden_states if self.only_cross_attention else None,
                    **cross_attention_kwargs)
                self.kf_attn_output = self.attn_output
                if shard is not None and inplace:
                    # ONE grouped exchange per block on the cached state: pivots / inverse norms were written by norm1,
                    # the to_out-projected attention output takes one copy into its slots (to_out is the model's own
                    # Linear: its output tensor is torch's); no allocation, no other copy
                    nb, ib, kfo = st[1], st[2], st[3]
                    Kl = shard.Kl
                    kfo[:, 1:].copy_(self.kf_attn_output.reshape(nbr, Kl, sequence_length, dim))
                    piv_e, inv_e = nb[:Kl + 1], ib[:Kl + 1]
                    reqs = shard.halo_block(piv_e, inv_e, kfo) if E == 1 else shard.halo_block(piv_e, inv_e, kfo, n_edits=E)
                    self.__dict__["_tf_halo"] = (piv_e, inv_e, kfo.view(nbr * (Kl + 1), sequence_length, dim), reqs)
                elif shard is not None:   # (pivots, inverse norms, attention output) with the neighbour's slot in
                    # front, and the pending requests of the exchange: the first chunk pass waits for them
                    kfl = self.kf_attn_output.reshape(batch_size, sequence_length, dim).contiguous()
                    self.__dict__["_tf_halo"] = (shard.halo_finish(halo, kfl, wait=False) if E == 1 else
                                                 shard.halo_finish(halo, kfl, wait=False, n_edits=E))
                if self.use_ada_layer_norm_zero:
                    self.attn_output = gate_msa.unsqueeze(1) * self.attn_output
                attn_output = self.attn_output
                hidden_states = hidden_states.reshape(batch_size, sequence_length, dim)
                pending = attn_output              # `hidden_states = attn_output + hidden_states` (396-397): fused into
            else:                                  # the norm that follows it, below
                c0, n_chunks = _chunk_run(self.batch_idx)
                # chunks with ONE keyframe: chunk 0 of the video, or the first chunk of every keyframe segment
                segs = _segments(self, self.kf_attn_output.shape[0] // nbr)
                starts = {0} if segs is None else {sum(segs[:v]) for v in range(len(segs))}
                first_single = c0 in starts
                # register_chunk_frames: the frame counts of a run of UNEQUAL chunks (None: today's paths)
                run = _ragged_run(self, c0, n_chunks, n_frames)
                if run is None and n_frames % n_chunks:
                    raise ValueError(f"{n_frames} frames per branch do not split into {n_chunks} chunks")
                n = n_frames // n_chunks
                kf = self.kf_attn_output
                piv, inv = self._tf_pivots, self._tf_pivot_inv_norm
                s0 = c0                 # slot of keyframe c0 in kf / piv / inv (one process: the keyframe index itself)
                shard = _active_shard(self)
                if shard is not None:   # this rank's caches: slot 0 = the left neighbour's last keyframe, then its own
                    if not (shard.kf0 <= c0 and c0 + n_chunks <= shard.kf0 + shard.Kl):
                        raise ValueError(f"chunks {c0}..{c0 + n_chunks - 1} are not owned by this rank "
                                         f"({shard.kf0}..{shard.kf0 + shard.Kl - 1})")
                    piv, inv, kf, reqs = self.__dict__["_tf_halo"]
                    if reqs:
                        shard.halo_wait(reqs)
                        self.__dict__["_tf_halo"] = (piv, inv, kf, [])
                    s0 = c0 - shard.kf0 + 1
                K = kf.shape[0] // nbr
                if self.use_ada_layer_norm_zero:
                    # 362-366: the reference gates the SELECTED keyframe outputs before the gather:
                    # `attn_output = gate_msa.unsqueeze(1) * kf_attn_output.view(3,K,S,D)[:, batch_idxs]`.  Same
                    # torch expression here (same broadcasting, same promotion) on the keyframes this pass reads;
                    # the gated copy becomes the gather source, re-indexed from 0.
                    lo = s0 if first_single else s0 - 1
                    sel = kf.view(3, K, sequence_length, dim)[:, lo:s0 + n_chunks]
                    kf = (gate_msa.unsqueeze(1) * sel).reshape(-1, sequence_length, dim)
                    # the attribute in the reference's order [i, i-1] (the gather source keeps ascending keyframes)
                    self.attn_output = lambda g_=kf: g_.view(3, -1, sequence_length, dim).flip(1)
                    kf_base, K = lo, kf.shape[0] // 3
                else:
                    kf_base = 0
                    # 361-363: the reference leaves the selected keyframe outputs, order [i, i-1] (a run of chunks: its
                    # keyframes in descending order); lazily -- the gather below reads the cache in place
                    slots = list(range(s0 + n_chunks - 1, (s0 if first_single else s0 - 1) - 1, -1))
                    self.attn_output = (lambda kf_=kf, K_=K, sl=slots:
                                        kf_.view(nbr, K_, sequence_length, dim)[:, sl])
                # 329-348: nearest neighbours of the SOURCE branch among keyframe c (and c-1), per chunk
                tgt = norm_hidden_states[0].reshape(n_frames * sequence_length, dim).to(self._tf_pivots.dtype)
                # 361-397: gather (same indices for the 3 branches), blend, residual -- fused with the search.
                # dtype follows torch promotion in the reference: the blend is fp32 (w1 is fp32, 385-388),
                # chunk 0 keeps the cached dtype (390); then `attn_output + hidden_states` (397).
                two = n_chunks > 1 or not first_single           # some chunk blends two keyframes (a run: its fp32 form)
                blend_dtype = torch.float32 if two else kf.dtype
                out_dtype = torch.promote_types(blend_dtype, hidden_states.dtype)
                w = (_ragged_weights(run, kf.device) if run is not None else _blend_weights(n, kf.device)) if two else None
                resid = hidden_states.reshape(batch_size, sequence_length, dim)
                if kf_base:      # gated copy holds keyframes kf_base.. only: search the same window of the pivots
                    piv, inv = piv[kf_base:kf_base + K], inv[kf_base:kf_base + K]
                # the norm that consumes this pass's residual stream next (norm2 in front of the cross-attention, else
                # norm3 in front of the feed-forward) rides in the gather's epilogue when it is a plain LayerNorm: the
                # fp32 stream is written once and not re-read by a norm launch (row f1/f2 of SURVEY.md section 8)
                nxt = None
                if self.attn2 is not None:
                    nxt = None if self.use_ada_layer_norm else ("norm2", self.norm2)
                elif not self.use_ada_layer_norm_zero:
                    nxt = ("norm3", self.norm3)
                fuse = None
                if nxt is not None and (FUSE_NORMS == "all" or FUSE_NORMS == nxt[0]) and FUSE_GATHER_NORM:
                    ndt = _fused_norm_dtype(nxt[1], resid, out_dtype)
                    if ndt is not None and ops.norm_fusable(kf, resid, out_dtype, 2 if two else 1, ndt):
                        fuse = (nxt[1].weight, nxt[1].bias, nxt[1].eps, ndt)
                if run is not None:     # chunks of unequal frame count: one ragged search, one ragged gather
                    single_mask = sum(1 << j for j in range(n_chunks) if c0 + j in starts)
                    res = ops.propagate_chunks_ragged(tgt, piv, inv, kf, w, run, s0, single_mask, resid, out_dtype, n_edits=E,
                                                      norm=fuse)
                elif E > 1:     # one search, one gather over all 1 + 2E branches
                    res = ops.propagate_chunks_edits(tgt, piv, inv, kf, w, n, n_chunks, s0 - kf_base, first_single, resid,
                                                     out_dtype, E, norm=fuse)
                elif n_chunks == 1:
                    ids = [s0 - kf_base] if first_single else [s0 - kf_base, s0 - 1 - kf_base]
                    res = ops.propagate(tgt, piv, inv, ids, kf, w, n, resid, out_dtype, norm=fuse)
                elif segs is not None:   # the one-keyframe chunks of the run: the segment starts inside it
                    single_mask = sum(1 << j for j in range(n_chunks) if c0 + j in starts)
                    res = ops.propagate_chunks_segments(tgt, piv, inv, kf, w, n, n_chunks, s0, single_mask, resid, out_dtype,
                                                        norm=fuse)
                else:
                    res = ops.propagate_chunks(tgt, piv, inv, kf, w, n, n_chunks, s0 - kf_base, first_single, resid,
                                               out_dtype, norm=fuse)
                if fuse is not None:
                    hidden_states, prenorm = res[0], (nxt[0], res[1])
                else:
                    hidden_states = res

            if self.attn2 is not None:
                if self.use_ada_layer_norm:
                    if pending is not None:
                        hidden_states, pending = pending + hidden_states, None
                    norm_hidden_states = self.norm2(hidden_states, timestep)
                elif pending is not None:
                    hidden_states, norm_hidden_states = _add_norm(self.norm2, pending, hidden_states, "norm2")
                    pending = None
                elif prenorm is not None and prenorm[0] == "norm2":
                    norm_hidden_states = prenorm[1]
                else:
                    norm_hidden_states = _block_norm(self.norm2, hidden_states, which="norm2")[0]
                pending = self.attn2(norm_hidden_states, encoder_hidden_states=encoder_hidden_states,
                                     attention_mask=encoder_attention_mask, **cross_attention_kwargs)   # + hidden_states (411)

            if self.use_ada_layer_norm_zero:    # the modulation consumes the fp32 norm output: keep the module
                if pending is not None:
                    hidden_states, pending = pending + hidden_states, None
                norm_hidden_states = self.norm3(hidden_states)
                norm_hidden_states = norm_hidden_states * (1 + scale_mlp[:, None]) + shift_mlp[:, None]
            elif pending is not None:
                hidden_states, norm_hidden_states = _add_norm(self.norm3, pending, hidden_states, "norm3")
                pending = None
            elif prenorm is not None and prenorm[0] == "norm3":
                norm_hidden_states = prenorm[1]
            else:
                norm_hidden_states = _block_norm(self.norm3, hidden_states, which="norm3")[0]
            ff_output = self.ff(norm_hidden_states)
            if self.use_ada_layer_norm_zero:
                ff_output = gate_mlp.unsqueeze(1) * ff_output
            return ff_output + hidden_states

    return TokenFlowBlock


def set_tokenflow(model: torch.nn.Module):
    """tokenflow_utils.py:432-448: class-swap every BasicTransformerBlock in place."""
    _announce()
    for _, module in model.named_modules():
        if isinstance_str(module, "BasicTransformerBlock"):
            module.__class__ = make_tokenflow_attention_block(module.__class__)
            if not hasattr(module, "use_ada_layer_norm_zero"):     # older diffusers (444-446)
                module.use_ada_layer_norm = False
                module.use_ada_layer_norm_zero = False
    return model
