"""Launch plans of the four-bank run form of the multi-edit attention (TF_ATTN_RUN_MULTI_V: `multi_v=True` on
ops.attn_run_edits_plan / ops.ext_attn_runs_edits[_views]), without a GPU.

  * with the flag, at head dims 40 and 64, the injecting edits are paired ascending and each pair is ONE ',MV4,...,run>' token
    in the place of its first edit's tokens; the odd injecting edit, the other edits, the source token and the merge token are
    the flag-less plan's;
  * the flag is a no-op (the same plan) at other head dims, under TF_ATTN_FOLD_SCALE, beside TF_ATTN_NO_MULTI_V, with fewer
    than two injecting edits and with one edit;
  * the workspace does not know the flag (it is no argument of the size query, and a run call accepts the flag-less size);
  * the one-call hints TF_ATTN_MULTI_V / TF_ATTN_MULTI_V64 stay refused, the merge call accepts the new bit;
  * the native rank executor's TF_RANK_BANK_EDIT_RUNS plan carries the tokens with the bit and is unchanged without it.
"""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import attn_run_edit_forms as ef  # noqa: E402
from tests import attn_run_forms as rf  # noqa: E402

MV4 = {40: "one<40,1,4,MV4,2,fq0,run>", 64: "one<64,1,8,MV4,2,fq1,run>"}
CONFIGS = [(2, 0b11), (3, 0b111), (3, 0b101), (4, 0b0111), (3, 0b010)]
# (S, H): one-tile and interleaved / DUAL launches at both head dims, a ragged frame, the shapes of the GPU tests
SHAPES = [(200, 2), (256, 2), (288, 2), (576, 2), (515, 1)]


def _ops():
    from tokenflow_amd import ops
    return ops


def _lib():
    from tokenflow_amd import _lib
    return _lib


def _inj(mask, E):
    return [e for e in range(E) if (mask >> e) & 1]


def _segments(ops, K, Kq, n, n_runs, S, H, dh, E, mask, bank_only, **kw):
    """The flag-less plan cut into (edit, tokens) segments in issue order, the source token (or None) and the merge token."""
    plan = ops.attn_run_edits_plan(K, Kq, n, n_runs, S, H, dh, E, mask, bank_only=bank_only, **kw)
    assert plan[0] == "vt_pack" and plan[-1] == f"merge[runs={n_runs},edits={E}]", plan
    body = plan[1:-1]
    src = None if bank_only else body.pop()
    segs = []
    for e in _inj(mask, E) + [e for e in range(E) if not (mask >> e) & 1]:
        own = ops.attn_run_plan(K, Kq, n, n_runs, S, H, dh, bool((mask >> e) & 1), bank_only=True, **kw)[1:-1]
        assert body[:len(own)] == own, (plan, e, own)
        segs.append((e, own))
        body = body[len(own):]
    assert not body, plan
    return plan, segs, src


def test_the_constant_is_a_free_bit():
    L = _lib()
    assert L.TF_ATTN_RUN_MULTI_V == 1 << 22
    others = (L.TF_ATTN_INJECT | L.TF_ATTN_EXACT_SCALE | L.TF_ATTN_BANK_ONLY | L.TF_ATTN_SOURCE_ONLY | L.TF_ATTN_NO_SPLIT |
              L.TF_ATTN_OUT_F32 | L.TF_ATTN_FOLD_SCALE | L.TF_ATTN_NO_FUSED | L.TF_ATTN_FUSED | (7 << 8) | (7 << 11) |
              L.TF_ATTN_HINT_QB2 | L.TF_ATTN_PRECISE_P | L.TF_ATTN_NO_PRECISE_P | L.TF_ATTN_HINT_MIX | L.TF_ATTN_MULTI_V |
              L.TF_ATTN_NO_MULTI_V | L.TF_ATTN_MULTI_V64)
    assert not others & L.TF_ATTN_RUN_MULTI_V
    assert L.load().tf_abi_version() == L.ABI_VERSION == 11


@pytest.mark.parametrize("dh", [40, 64])
@pytest.mark.parametrize("S,H", SHAPES, ids=lambda x: str(x))
@pytest.mark.parametrize("E,mask", CONFIGS)
@pytest.mark.parametrize("no_split", [False, True])
def test_pairs_take_one_four_bank_run_token_in_the_place_of_their_first_edit(dh, S, H, E, mask, no_split):
    ops = _ops()
    K, Kq, runs = 6, 2, [(1, 4), (0, 1), (5, 1)]
    inj = _inj(mask, E)
    firsts, seconds = inj[0:2 * (len(inj) // 2):2], inj[1:2 * (len(inj) // 2):2]
    for r, (f0, n) in enumerate(runs):
        bank_only = r != 0
        plain, segs, src = _segments(ops, K, Kq, n, len(runs), S, H, dh, E, mask, bank_only, no_split=no_split)
        got = ops.attn_run_edits_plan(K, Kq, n, len(runs), S, H, dh, E, mask, bank_only=bank_only, no_split=no_split,
                                      multi_v=True)
        want = ["vt_pack"]
        for e, own in segs:
            want += [MV4[dh]] if e in firsts else [] if e in seconds else own
        want += ([] if src is None else [src]) + [plain[-1]]
        assert got == want, (dh, S, H, E, mask, r, got, want)
        assert got.count(MV4[dh]) == len(inj) // 2 == bin(mask).count("1") // 2
        assert sum(1 for t in got if ",MV4," in t) == len(inj) // 2 and got.count("vt_pack") == 1
        assert not any(",MV4," in t for t in plain)
        if len(inj) < 2:
            assert got == plain


@pytest.mark.parametrize("E,mask", CONFIGS + [(2, 0b00), (2, 0b01)])
def test_the_flag_is_a_no_op_where_the_form_does_not_exist(E, mask):
    ops, L = _ops(), _lib()
    K, Kq, n, n_runs = 6, 2, 4, 3

    def both(S, H, dh, **kw):
        return (ops.attn_run_edits_plan(K, Kq, n, n_runs, S, H, dh, E, mask, multi_v=True, **kw),
                ops.attn_run_edits_plan(K, Kq, n, n_runs, S, H, dh, E, mask, **kw))
    for S, H, dh in [(256, 2, 80), (72, 1, 160), (576, 2, 80)]:                     # no four-bank kernel at these head dims
        on, off = both(S, H, dh)
        assert on == off, (dh, on, off)
    for dh in (40, 64):
        on, off = both(256, 2, dh, hints=L.TF_ATTN_NO_MULTI_V)                       # switched off
        assert on == off == ops.attn_run_edits_plan(K, Kq, n, n_runs, 256, 2, dh, E, mask), (dh, on, off)
        if bin(mask).count("1") < 2:                                                # nothing to pair
            on, off = both(256, 2, dh)
            assert on == off, (dh, on, off)
    on, off = both(256, 2, 40, fold_scale=True)                                      # the folded scale (Dh = 40 only)
    assert on == off and not any(",MV4," in t for t in on), (on, off)
    for inject in (0, 1):                                                            # one edit: the single-edit run set
        for dh in (40, 64):
            assert ops.attn_run_edits_plan(K, Kq, n, n_runs, 256, 2, dh, 1, inject, multi_v=True) == \
                ops.attn_run_plan(K, Kq, n, n_runs, 256, 2, dh, bool(inject))


def test_existing_cases_keep_their_plans_without_the_flag_and_pair_with_it():
    ops = _ops()
    for c in ef.CASES:
        inj = bin(c["mask"]).count("1")
        for r, (f0, n) in enumerate(c["runs"]):
            args = (c["K"], c["Kq"], n, len(c["runs"]), c["S"], c["heads"], c["dh"], c["n_edits"], c["mask"])
            off = ops.attn_run_edits_plan(*args, bank_only=r != 0)
            on = ops.attn_run_edits_plan(*args, bank_only=r != 0, multi_v=True)
            assert not any(",MV4," in t for t in off)
            assert sum(1 for t in on if ",MV4," in t) == (inj // 2 if c["dh"] in (40, 64) else 0), (c, on)


def _call_args(Dh=40, E=2):
    L = _lib()
    K, Kq, S, H, n_runs = 5, 2, 256, 2, 3
    D = H * Dh
    fs = S * D
    strides = (ctypes.c_int64 * 9)(Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, D)
    nbytes = L.load().tf_ext_attn_runs_edits_workspace_bytes(K, Kq, S, H, Dh, n_runs, E, L.TF_BF16)
    return K, Kq, S, H, n_runs, D, fs, strides, nbytes


@pytest.mark.parametrize("Dh", [40, 64])
def test_the_old_hints_stay_refused_and_the_merge_ignores_the_new_bit(Dh):
    ops, L = _ops(), _lib()
    lib = L.load()
    E = 2
    K, Kq, S, H, n_runs, D, fs, strides, nbytes = _call_args(Dh, E)
    assert nbytes > 0
    ph = 1 << 12   # placeholder pointers: aligned, never dereferenced by a refused call

    def run(flags, E_=E, mask=0b11):
        return lib.tf_ext_attn_run_edits(ph, ph, ph, ph, K, Kq, 2, 2, 2, 0, n_runs, S, H, Dh, D,
                                         ctypes.cast(strides, ctypes.c_void_p), 1.0, flags, L.TF_BF16, E_, mask, 0, ph, nbytes,
                                         None)

    def merge(flags):
        return lib.tf_ext_attn_runs_merge_edits(ph, K, Kq, S, H, Dh, n_runs, E, 0b11, Kq * fs, fs, flags, L.TF_BF16, ph, nbytes,
                                                None)
    for old in (L.TF_ATTN_MULTI_V, L.TF_ATTN_MULTI_V64, L.TF_ATTN_MULTI_V | L.TF_ATTN_MULTI_V64):
        for extra in (0, L.TF_ATTN_RUN_MULTI_V, L.TF_ATTN_BANK_ONLY):
            for E_, mask in ((E, 0b11), (1, 0b1)):
                assert run(old | extra, E_, mask) == -3
                msg = lib.tf_last_error().decode()
                assert "tf_ext_attn_run_edits" in msg and "TF_ATTN_RUN_MULTI_V" in msg, msg
        assert merge(old) == -3 and "tf_ext_attn_runs_merge_edits" in lib.tf_last_error().decode()
        assert merge(old | L.TF_ATTN_RUN_MULTI_V) == -3 and "tf_ext_attn_runs_merge_edits" in lib.tf_last_error().decode()
        with pytest.raises(L.TokenflowHipError, match="tf_ext_attn_run_edits_plan"):
            ops.attn_run_edits_plan(K, Kq, 2, n_runs, S, H, Dh, E, 0b11, hints=old, multi_v=True)
        with pytest.raises(L.TokenflowHipError, match="tf_ext_attn_run_edits_plan"):
            ops.attn_run_edits_plan(K, Kq, 2, n_runs, S, H, Dh, E, 0b11, hints=old)
    # what a run call refuses of its own stays refused beside the new bit
    for bad in (L.TF_ATTN_INJECT, L.TF_ATTN_SOURCE_ONLY, L.TF_ATTN_FUSED, L.attn_hint(qw=2)):
        assert run(bad | L.TF_ATTN_RUN_MULTI_V) == -3 and "tf_ext_attn_run_edits" in lib.tf_last_error().decode()
    assert run(L.TF_ATTN_RUN_MULTI_V, E, 0b100) == -3
    # the merge call accepts the bit and records the same token (under the plan recorder: nothing is launched)
    on = ops.attn_run_edits_plan(K, Kq, 2, n_runs, S, H, Dh, E, 0b11, multi_v=True)
    assert on[-1] == f"merge[runs={n_runs},edits={E}]"
    # `multi_v=` is a keyword of its own, not a hint
    assert on == ops.attn_run_edits_plan(K, Kq, 2, n_runs, S, H, Dh, E, 0b11, hints=L.TF_ATTN_RUN_MULTI_V)


def test_the_workspace_is_the_flag_less_one():
    """The size query has no flags argument; a run call with the flag accepts exactly the flag-less size and refuses one byte
    less with TF_ERR_WORKSPACE, as without the flag (the four-bank launch writes into the edits' own regions)."""
    L = _lib()
    lib = L.load()
    for Dh in (40, 64):
        for E, mask in CONFIGS:
            K, Kq, S, H, n_runs, D, fs, strides, nbytes = _call_args(Dh, E)
            assert nbytes == lib.tf_ext_attn_runs_edits_workspace_bytes(K, Kq, S, H, Dh, n_runs, E, L.TF_BF16) > 0
            ph = 1 << 12
            for flags in (0, L.TF_ATTN_RUN_MULTI_V):
                rc = lib.tf_ext_attn_run_edits(ph, ph, ph, ph, K, Kq, 2, 2, 2, 0, n_runs, S, H, Dh, D,
                                               ctypes.cast(strides, ctypes.c_void_p), 1.0, flags, L.TF_BF16, E, mask, 0, ph,
                                               nbytes - 1, None)
                assert rc == -5 and "tf_ext_attn_run_edits" in lib.tf_last_error().decode(), (Dh, E, mask, flags, rc)


@pytest.mark.parametrize("dh,S,H", [(40, 256, 2), (64, 320, 5), (40, 192, 2)])
@pytest.mark.parametrize("E,mask", CONFIGS)
@pytest.mark.parametrize("world,rank,K", [(2, 0, 5), (2, 1, 5), (8, 3, 8)])
def test_the_executors_edit_runs_plan_carries_the_tokens(dh, S, H, E, mask, world, rank, K):
    from tokenflow_amd import sharded
    L = _lib()
    off = sharded.rank_edits_plan(world, rank, K, S, H, dh, E, mask, mode="bank_edit_runs")
    on = sharded.rank_edits_plan(world, rank, K, S, H, dh, E, mask, mode="bank_edit_runs", flags=L.TF_ATTN_RUN_MULTI_V)
    assert not any(",MV4," in t for t in off), off
    n_run_calls = off.count("vt_pack")
    assert n_run_calls >= 2
    pairs = bin(mask).count("1") // 2
    assert on.count(MV4[dh]) == pairs * n_run_calls, (on, off)
    if pairs == 0:
        assert on == off
    else:
        # everything that is no bank launch of a paired edit is where it was
        keep = lambda p: [t for t in p if not t.endswith(",run>")]   # noqa: E731
        assert keep(on) == keep(off) and len(on) < len(off)
    # the other modes of the executor never see the bit's tokens
    for mode in ("bank", "heads") if H % world == 0 else ("bank",):
        assert not any(",run>" in t for t in sharded.rank_edits_plan(world, rank, K, S, H, dh, E, mask, mode=mode))


def test_the_shards_take_the_opt_in_from_the_keyword_or_the_environment(monkeypatch):
    from tokenflow_amd import sharded
    monkeypatch.delenv("TOKENFLOW_SHARD_EDIT_RUNS_MULTI_V", raising=False)
    assert sharded.FrameShard(4).edit_runs_multi_v is False
    assert sharded.FrameShard(4, edit_runs=True, edit_runs_multi_v=True).edit_runs_multi_v is True
    monkeypatch.setenv("TOKENFLOW_SHARD_EDIT_RUNS_MULTI_V", "1")
    assert sharded.FrameShard(4).edit_runs_multi_v is True
    assert sharded.FrameShard(4, edit_runs_multi_v=False).edit_runs_multi_v is False
    monkeypatch.setenv("TOKENFLOW_SHARD_EDIT_RUNS_MULTI_V", "0")
    assert sharded.FrameShard(4).edit_runs_multi_v is False
