"""Drop-in replacement for omerbt/TokenFlow's `tokenflow_utils.py`.

`run_tokenflow_pnp.py` / `run_tokenflow_sdedit.py` of the reference do
`from tokenflow_utils import *` (run_tokenflow_pnp.py:16): put this repository first on
PYTHONPATH and they pick up the MI355X implementation unchanged.
The implementation lives in tokenflow_amd/hooks.py.
"""
from tokenflow_amd.hooks import (  # noqa: F401
    batch_cosine_sim, isinstance_str, load_source_latents_t, make_tokenflow_attention_block,
    register_batch_idx, register_conv_injection, register_extended_attention,
    register_edit_schedules, register_edits, register_segments, register_chunk_frames, register_bank_window, register_extended_attention_pnp, register_frame_shard, register_pivotal, register_time, set_tokenflow)
# register_frame_shard: multi-GPU extension (one process per GPU), not part of the reference's surface
# register_edits: multi-edit extension (several prompts on one source video in one pass), not part of it either;
# register_edit_schedules: the edits' own injection schedules
# register_segments: keyframe-segment extension (several scenes or clips in one pass)
# register_chunk_frames: ragged chunk runs (a run pass over chunks of unequal frame count: video tails, scenes of any length)
# register_bank_window: sliding-window bank extension (a keyframe attends to its neighbouring keyframes only: long videos;
# anchors=... adds global anchor keyframes that every keyframe sees; edits=True / anchor_edits=True open both for several prompts)

# `from tokenflow_utils import *` in the reference also leaks these two names (its module does
# `import torch, os` at top level, tokenflow_utils.py:2-3); keep that surface identical.
import os  # noqa: F401,E402
import torch  # noqa: F401,E402
