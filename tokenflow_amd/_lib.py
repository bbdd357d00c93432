"""ctypes binding of libtokenflow_hip.so (C ABI: include/tokenflow_hip.h)."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# TOKENFLOW_HIP_LIB overrides the library path (kernel A/B experiments, tools/attn_microbench.py)
LIB_PATH = os.environ.get("TOKENFLOW_HIP_LIB") or os.path.join(_HERE, "libtokenflow_hip.so")

TF_BF16, TF_F16, TF_F32 = 0, 1, 2
TF_ATTN_INJECT, TF_ATTN_EXACT_SCALE, TF_ATTN_BANK_ONLY, TF_ATTN_SOURCE_ONLY, TF_ATTN_NO_SPLIT = 1, 2, 4, 8, 16
TF_ATTN_OUT_F32 = 32
TF_ATTN_FOLD_SCALE = 64
TF_ATTN_NO_FUSED, TF_ATTN_FUSED = 128, 1 << 17
TF_ATTN_HINT_QB2, TF_ATTN_PRECISE_P, TF_ATTN_NO_PRECISE_P = 1 << 14, 1 << 15, 1 << 16
TF_ATTN_MULTI_V, TF_ATTN_NO_MULTI_V = 1 << 19, 1 << 20   # ext_attn_edits: the four-bank form for pairs of edits forced on / off
TF_ATTN_MULTI_V64 = 1 << 21                               # ... the form at head dim 64 forced on (TF_ATTN_NO_MULTI_V switches it off too)
TF_ATTN_RUN_MULTI_V = 1 << 22                             # ext_attn_runs_edits: pairs of injecting edits as ONE four-bank run launch (Dh 40, 64)
TF_ATTN_HINT_MIX = 1 << 18   # Dh = 40 streaming kernel: the mixed-MFMA-shape form whatever the launch size (S % 64 == 0, S >= 256)


def attn_hint(qw: int = 0, kw: int = 0, qb: int = 1) -> int:
    """TF_ATTN_HINT_QW / _KW bits of the fused small-problem kernel: qw in {0 (auto), 1 (the wave-private form), 2, 4}
    query waves per workgroup, kw in {0 (auto), 1, 2, 4, 8} key groups."""
    code = {0: 0, 1: 1, 2: 2, 4: 3, 8: 4}
    return (code[qw] << 8) | (code[kw] << 11) | (TF_ATTN_HINT_QB2 if qb == 2 else 0)


ABI_VERSION = 11
TF_MAX_EDITS = 8
TF_MAX_SEGMENTS = 8
TF_MAX_WINDOW_FRAMES = 64
TF_RANK_HEADS, TF_RANK_BANK, TF_RANK_SLOTS, TF_RANK_NO_HALO, TF_RANK_INV_NORM = 0, 1, 64, 16, 32
TF_RANK_BANK_RUNS = 2
TF_RANK_BANK_EDIT_RUNS = 3   # tf_rank_pivotal_edits: the bank in runs for a multi-edit batch
TF_ERR_COMM = -6

_c = ctypes
_SIGNATURES = {
    "tf_abi_version": (_c.c_int, []),
    "tf_last_error": (_c.c_char_p, []),
    "tf_ext_attn_workspace_bytes": (_c.c_size_t, [_c.c_int] * 5),
    # launch plans (host only: no device, no allocation; tests/test_kernel_plan_cpu.py)
    "tf_ext_attn_plan": (_c.c_int, [_c.c_int] * 7 + [_c.c_char_p, _c.c_size_t]),
    "tf_nn_search_plan": (_c.c_int, [_c.c_int64] + [_c.c_int] * 4 + [_c.c_char_p, _c.c_size_t]),
    "tf_ext_attn_fwd": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_float, _c.c_int, _c.c_int,
                                   _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_fwd_strided": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float,
                                           _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    # multi-edit batches (ABI 10)
    "tf_ext_attn_edits_workspace_bytes": (_c.c_size_t, [_c.c_int] * 6),
    "tf_ext_attn_fwd_edits": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float,
                                         _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_edits_plan": (_c.c_int, [_c.c_int] * 8 + [_c.c_char_p, _c.c_size_t]),
    "tf_nn_gather_blend_chunks_edits": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 13 + [_c.c_void_p, _c.c_size_t,
                                                   _c.c_void_p]),
    "tf_nn_gather_blend_chunks_norm_edits": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 13 + [_c.c_void_p, _c.c_void_p,
                                                        _c.c_float, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p,
                                                        _c.c_size_t, _c.c_void_p]),
    "tf_nn_gather_blend_edits_plan": (_c.c_int, [_c.c_int] * 6 + [_c.c_char_p, _c.c_size_t]),
    "tf_inject_copy_edits": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_void_p]),
    # per-edit injection state (ABI 11)
    "tf_ext_attn_fwd_edits_masked": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float,
                                                _c.c_int, _c.c_int, _c.c_int, _c.c_uint, _c.c_void_p, _c.c_size_t,
                                                _c.c_void_p]),
    "tf_ext_attn_edits_masked_plan": (_c.c_int, [_c.c_int] * 6 + [_c.c_uint, _c.c_int, _c.c_int, _c.c_char_p, _c.c_size_t]),
    # the parts of a multi-edit call (a frame-sharded rank's bank part on its receive buffer, source part on its own tensors)
    "tf_ext_attn_fwd_edits_part": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float,
                                              _c.c_int, _c.c_int, _c.c_int, _c.c_uint, _c.c_int, _c.c_void_p, _c.c_size_t,
                                              _c.c_void_p]),
    "tf_ext_attn_edits_part_plan": (_c.c_int, [_c.c_int] * 6 + [_c.c_uint, _c.c_int, _c.c_int, _c.c_int, _c.c_char_p,
                                               _c.c_size_t]),
    "tf_inject_copy_edits_masked": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int, _c.c_uint, _c.c_int, _c.c_void_p]),
    # attention over a bank that arrives in pieces: run + merge (ABI 9)
    "tf_ext_attn_runs_workspace_bytes": (_c.c_size_t, [_c.c_int] * 7),
    "tf_ext_attn_run": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 10 + [_c.c_int64, _c.c_void_p, _c.c_float, _c.c_int,
                                   _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_runs_merge": (_c.c_int, [_c.c_void_p] + [_c.c_int] * 6 + [_c.c_int64, _c.c_int64, _c.c_int, _c.c_int,
                                          _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_run_plan": (_c.c_int, [_c.c_int] * 9 + [_c.c_char_p, _c.c_size_t]),
    # run + merge for a multi-edit batch (additive to ABI 11)
    "tf_ext_attn_runs_edits_workspace_bytes": (_c.c_size_t, [_c.c_int] * 8),
    "tf_ext_attn_run_edits": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 10 + [_c.c_int64, _c.c_void_p, _c.c_float, _c.c_int,
                                         _c.c_int, _c.c_int, _c.c_uint, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_runs_merge_edits": (_c.c_int, [_c.c_void_p] + [_c.c_int] * 7 + [_c.c_uint, _c.c_int64, _c.c_int64, _c.c_int,
                                                _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_run_edits_plan": (_c.c_int, [_c.c_int] * 8 + [_c.c_uint, _c.c_int, _c.c_int, _c.c_char_p, _c.c_size_t]),
    "tf_head_pack": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p] + [_c.c_int] * 4 + [_c.c_int64, _c.c_int,
                                _c.c_void_p]),
    "tf_head_unpack": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p] + [_c.c_int] * 5 + [_c.c_int64, _c.c_int,
                                  _c.c_void_p]),
    "tf_pivot_inv_norm": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_void_p]),
    "tf_nn_search_workspace_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int, _c.c_int, _c.c_int]),
    "tf_nn_search": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int64] + [_c.c_int] * 6 + [_c.c_void_p, _c.c_size_t,
                                _c.c_void_p]),
    "tf_gather_blend": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int] * 10 + [_c.c_void_p]),
    "tf_nn_gather_blend_workspace_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int, _c.c_int, _c.c_int]),
    "tf_nn_gather_blend": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 11 + [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_nn_gather_blend_chunks_workspace_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int, _c.c_int, _c.c_int]),
    "tf_nn_gather_blend_chunks": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 12 + [_c.c_void_p, _c.c_size_t,
                                             _c.c_void_p]),
    "tf_nn_gather_blend_norm": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 11 + [_c.c_void_p, _c.c_void_p, _c.c_float,
                                           _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_nn_gather_blend_chunks_norm": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 12 + [_c.c_void_p, _c.c_void_p,
                                                  _c.c_float, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p,
                                                  _c.c_size_t, _c.c_void_p]),
    "tf_layer_norm": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int64, _c.c_int, _c.c_float] + [_c.c_int] * 3 + [_c.c_void_p]),
    "tf_add_layer_norm": (_c.c_int, [_c.c_void_p] * 6 + [_c.c_int64, _c.c_int, _c.c_float] + [_c.c_int] * 5 + [_c.c_void_p]),
    "tf_ddim_step": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int64] + [_c.c_float] * 4 + [_c.c_int, _c.c_void_p]),
    "tf_inject_copy": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_int, _c.c_void_p]),
    # multi-GPU exchange steps over RCCL (tokenflow_amd/comm.py; the sharded host path uses torch.distributed instead)
    "tf_comm_available": (_c.c_int, []),
    "tf_comm_unique_id": (_c.c_int, [_c.c_void_p]),
    "tf_comm_init": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p]),
    "tf_comm_destroy": (_c.c_int, [_c.c_void_p]),
    "tf_comm_rank": (_c.c_int, [_c.c_void_p]),
    "tf_comm_world": (_c.c_int, [_c.c_void_p]),
    "tf_allgather_kv": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_void_p]),
    "tf_allgather_rows": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int64, _c.c_int, _c.c_void_p]),
    "tf_all_to_all_rows": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int64, _c.c_int, _c.c_void_p]),
    "tf_sendrecv_pivot": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                     _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "tf_comm_init_hooks": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p]),
    "tf_comm_init_loopback": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p]),
    "tf_comm_loopback_copies": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "tf_comm_loopback_wire": (_c.c_int, [_c.c_void_p, _c.c_double, _c.c_double]),
    # one rank's pivotal pass of a block in one call (csrc/rank_exec.hip; tokenflow_amd/sharded.py NativeShard)
    "tf_rank_create": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "tf_rank_destroy": (_c.c_int, [_c.c_void_p]),
    "tf_rank_local_keyframes": (_c.c_int, [_c.c_void_p]),
    "tf_rank_first_keyframe": (_c.c_int, [_c.c_void_p]),
    "tf_rank_pivotal_workspace_bytes": (_c.c_size_t, [_c.c_void_p] + [_c.c_int] * 4),
    "tf_rank_pivotal": (_c.c_int, [_c.c_void_p] * 8 + [_c.c_int] * 3 + [_c.c_float] + [_c.c_int] * 4 +
                        [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_rank_halo_wait": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p]),
    # the rank executor for a multi-edit batch (additive to ABI 11)
    "tf_rank_pivotal_edits_workspace_bytes": (_c.c_size_t, [_c.c_void_p] + [_c.c_int] * 5),
    "tf_rank_pivotal_edit_runs_workspace_bytes": (_c.c_size_t, [_c.c_void_p] + [_c.c_int] * 5),
    "tf_rank_pivotal_edits": (_c.c_int, [_c.c_void_p] * 8 + [_c.c_int] * 3 + [_c.c_float] + [_c.c_int] * 5 + [_c.c_uint] +
                              [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_rank_pivotal_edits_plan": (_c.c_int, [_c.c_int] * 7 + [_c.c_uint] + [_c.c_int] * 3 + [_c.c_char_p, _c.c_size_t]),
    # keyframe segments: several scenes or clips in one pass (additive to ABI 11)
    "tf_ext_attn_segments_workspace_bytes": (_c.c_size_t, [_c.c_int] * 5),
    "tf_ext_attn_fwd_segments": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int, _c.c_int, _c.c_void_p] + [_c.c_int] * 3 +
                                 [_c.c_int64, _c.c_float, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_segments_plan": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p] + [_c.c_int] * 5 + [_c.c_char_p, _c.c_size_t]),
    "tf_nn_gather_blend_chunks_segments": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 6 + [_c.c_uint64] + [_c.c_int] * 5 +
                                           [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_nn_gather_blend_chunks_norm_segments": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 6 + [_c.c_uint64] +
                                                [_c.c_int] * 5 + [_c.c_void_p, _c.c_void_p, _c.c_float, _c.c_int,
                                                                  _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t,
                                                                  _c.c_void_p]),
    "tf_nn_gather_blend_segments_plan": (_c.c_int, [_c.c_int] * 4 + [_c.c_uint64, _c.c_char_p, _c.c_size_t]),
    # ragged chunk runs: one propagation call for chunks of unequal frame count (additive to ABI 11)
    "tf_nn_gather_blend_ragged_workspace_bytes": (_c.c_size_t, [_c.c_void_p] + [_c.c_int] * 3),
    "tf_nn_gather_blend_chunks_ragged": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int, _c.c_void_p] + [_c.c_int] * 4 +
                                         [_c.c_uint64] + [_c.c_int] * 6 + [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_nn_gather_blend_chunks_norm_ragged": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int, _c.c_void_p] + [_c.c_int] * 4 +
                                              [_c.c_uint64] + [_c.c_int] * 6 +
                                              [_c.c_void_p, _c.c_void_p, _c.c_float, _c.c_int, _c.c_void_p, _c.c_int,
                                               _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_nn_gather_blend_ragged_plan": (_c.c_int, [_c.c_void_p] + [_c.c_int] * 3 + [_c.c_uint64, _c.c_int, _c.c_char_p,
                                                                                  _c.c_size_t]),
    # sliding-window keyframe bank: a keyframe attends to its neighbouring keyframes only (additive to ABI 11)
    "tf_ext_attn_fwd_windows": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float, _c.c_int,
                                           _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_windows_plan": (_c.c_int, [_c.c_int] * 8 + [_c.c_void_p, _c.c_void_p, _c.c_char_p, _c.c_size_t]),
    # ... for a multi-edit batch: several prompts on one long video in one pass (additive to ABI 11)
    "tf_ext_attn_fwd_windows_edits": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float,
                                                 _c.c_int, _c.c_int, _c.c_int, _c.c_uint, _c.c_void_p, _c.c_void_p,
                                                 _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_windows_edits_plan": (_c.c_int, [_c.c_int] * 7 + [_c.c_uint, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                                  _c.c_char_p, _c.c_size_t]),
    # frame-set keyframe bank: a window plus global anchor keyframes, or any other keyframe sparsity (additive to ABI 11)
    "tf_ext_attn_fwd_frame_sets": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float, _c.c_int,
                                              _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_frame_sets_plan": (_c.c_int, [_c.c_int] * 8 + [_c.c_void_p, _c.c_char_p, _c.c_size_t]),
    # ... for a multi-edit batch: several prompts with anchor keyframes in one pass (additive to ABI 11)
    "tf_ext_attn_fwd_frame_sets_edits": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float,
                                                    _c.c_int, _c.c_int, _c.c_int, _c.c_uint, _c.c_void_p, _c.c_void_p,
                                                    _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_frame_sets_edits_plan": (_c.c_int, [_c.c_int] * 7 + [_c.c_uint, _c.c_int, _c.c_int, _c.c_void_p, _c.c_char_p,
                                                     _c.c_size_t]),
    # sliding-window bank on a frame shard: long videos across GPUs (additive to ABI 11)
    "tf_ext_attn_fwd_windows_part": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float,
                                                _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                                _c.c_void_p]),
    "tf_ext_attn_windows_part_plan": (_c.c_int, [_c.c_int] * 8 + [_c.c_void_p, _c.c_void_p, _c.c_char_p, _c.c_size_t]),
    "tf_window_halo_pack": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p] +
                            [_c.c_int] * 3 + [_c.c_int64, _c.c_int, _c.c_void_p]),
    "tf_rank_pivotal_window_workspace_bytes": (_c.c_size_t, [_c.c_void_p] + [_c.c_int] * 5),
    "tf_rank_pivotal_window": (_c.c_int, [_c.c_void_p] * 8 + [_c.c_int] * 3 + [_c.c_float] + [_c.c_int] * 5 +
                               [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_rank_pivotal_window_plan": (_c.c_int, [_c.c_int] * 10 + [_c.c_char_p, _c.c_size_t]),
    # anchor keyframes on a windowed frame shard: frame sets across GPUs (additive to ABI 11)
    "tf_ext_attn_fwd_frame_sets_part": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float,
                                                   _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_frame_sets_part_plan": (_c.c_int, [_c.c_int] * 8 + [_c.c_void_p, _c.c_char_p, _c.c_size_t]),
    "tf_frame_set_halo_pack": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p] +
                               [_c.c_int] * 3 + [_c.c_int64, _c.c_int, _c.c_void_p]),
    "tf_rank_pivotal_frame_sets_workspace_bytes": (_c.c_size_t, [_c.c_void_p] + [_c.c_int] * 5 + [_c.c_void_p, _c.c_int]),
    "tf_rank_pivotal_frame_sets": (_c.c_int, [_c.c_void_p] * 8 + [_c.c_int] * 3 + [_c.c_float] + [_c.c_int] * 5 +
                                   [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_rank_pivotal_frame_sets_plan": (_c.c_int, [_c.c_int] * 7 + [_c.c_void_p] + [_c.c_int] * 4 + [_c.c_char_p, _c.c_size_t]),
    # the bank part of a windowed / frame-set multi-edit pass: all edits under one table (additive to ABI 11)
    "tf_ext_attn_fwd_windows_edits_part": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float,
                                                      _c.c_int, _c.c_int, _c.c_int, _c.c_uint, _c.c_int, _c.c_void_p,
                                                      _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_windows_edits_part_plan": (_c.c_int, [_c.c_int] * 7 + [_c.c_uint, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                                       _c.c_void_p, _c.c_char_p, _c.c_size_t]),
    "tf_ext_attn_fwd_frame_sets_edits_part": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_int64, _c.c_void_p, _c.c_float,
                                                         _c.c_int, _c.c_int, _c.c_int, _c.c_uint, _c.c_int, _c.c_void_p,
                                                         _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_ext_attn_frame_sets_edits_part_plan": (_c.c_int, [_c.c_int] * 7 + [_c.c_uint, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                                          _c.c_char_p, _c.c_size_t]),
    # ... on a frame shard: ONE pack of a multi-edit halo, the rank executor (additive to ABI 11)
    "tf_edit_halo_pack": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                     _c.c_void_p, _c.c_int, _c.c_void_p] + [_c.c_int] * 3 + [_c.c_int64, _c.c_int64, _c.c_int,
                                                                                              _c.c_void_p]),
    "tf_rank_pivotal_frame_sets_edits_workspace_bytes": (_c.c_size_t, [_c.c_void_p] + [_c.c_int] * 5 + [_c.c_void_p, _c.c_int,
                                                                                                         _c.c_int]),
    "tf_rank_pivotal_frame_sets_edits": (_c.c_int, [_c.c_void_p] * 8 + [_c.c_int] * 3 + [_c.c_float] + [_c.c_int] * 5 +
                                         [_c.c_void_p, _c.c_int, _c.c_int, _c.c_uint, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "tf_rank_pivotal_frame_sets_edits_plan": (_c.c_int, [_c.c_int] * 7 + [_c.c_void_p, _c.c_int, _c.c_int, _c.c_uint] +
                                              [_c.c_int] * 3 + [_c.c_char_p, _c.c_size_t]),
}
EXPORTS = tuple(_SIGNATURES)

_lib = None


class TokenflowHipError(RuntimeError):
    pass


def load():
    """Load the library (idempotent).  torch must be imported first so that the
    library's libamdhip64 dependency resolves to the runtime torch already mapped."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (maps libamdhip64 before dlopen)
    if not os.path.isfile(LIB_PATH):
        raise TokenflowHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C tokenflow_amd/csrc`.  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.tf_abi_version() != ABI_VERSION:
        raise TokenflowHipError(f"ABI version {lib.tf_abi_version()} != {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().tf_last_error().decode(errors="replace")
        raise TokenflowHipError(f"{what} failed (rc={rc}): {msg}")
