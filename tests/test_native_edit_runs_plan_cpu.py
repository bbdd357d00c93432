"""The native rank executor's multi-edit run mode (TF_RANK_BANK_EDIT_RUNS of tf_rank_pivotal_edits), host side: the sequence
one call issues, recorded by the call's own body (no device, stream or communicator), and its refusals."""
import ctypes

import pytest

from tokenflow_amd import _lib, ops, sharded

H = 2
SHAPES = [(256, 40), (576, 64), (72, 160)]                        # (S, Dh)
GEOMETRY = [(2, 4), (2, 5), (8, 8)]                               # (world, K): even, uneven 3 + 2, one keyframe per rank
CASES = [(2, 0b00), (2, 0b11), (2, 0b01), (3, 0b101), (3, 0b010)]


def _shard_runs(world, rank, K):
    """(Kl, runs in slot order local, left, right) of `rank`."""
    counts = [K // world + (1 if r < K % world else 0) for r in range(world)]
    kf0, Kl = sum(counts[:rank]), counts[rank]
    runs = [(kf0, Kl)]
    if kf0 > 0:
        runs.append((0, kf0))
    if kf0 + Kl < K:
        runs.append((kf0 + Kl, K - kf0 - Kl))
    return Kl, runs


def test_exports():
    lib = _lib.load()
    assert "tf_rank_pivotal_edit_runs_workspace_bytes" in _lib.EXPORTS
    assert lib.tf_rank_pivotal_edit_runs_workspace_bytes(None, 64, 2, 40, 2, _lib.TF_BF16) == 0
    assert _lib.TF_RANK_BANK_EDIT_RUNS == 3


@pytest.mark.parametrize("E,mask", CASES)
@pytest.mark.parametrize("world,K", GEOMETRY)
@pytest.mark.parametrize("no_split", [True, False])
def test_token_sequence(world, K, E, mask, no_split):
    n_non = E - bin(mask).count("1")
    ns, B = (1 if mask else 0) + 2 * n_non + 2 * E, 1 + 2 * E
    for S, dh in SHAPES:
        for rank in sorted({0, 1, world - 1}):
            Kl, runs = _shard_runs(world, rank, K)
            for inv in (False, True):
                plan = sharded.rank_edits_plan(world, rank, K, S, H, dh, E, mask, "bank_edit_runs", inv_norm=inv,
                                               no_split=no_split)
                want = [("pack+inv" if inv else "pack") + f"[ns={ns}]", f"gather[slabs={ns}]"]
                for r, (f0, n) in enumerate(runs):      # the local run (with the source branch), then each remote run
                    want += ops.attn_run_edits_plan(K, Kl, n, len(runs), S, H, dh, E, mask, bank_only=r != 0,
                                                    no_split=no_split)[:-1]
                want += [f"merge[runs={len(runs)},edits={E}]", f"halo[n={2 + B}]"]
                assert plan == want, (S, dh, rank, plan, want)
                assert sum(t.startswith("pack") for t in plan) == 1 and sum(t.startswith("gather") for t in plan) == 1
                assert not any(t.startswith(("qcompact", "a2a", "unpack", "fused[")) for t in plan), plan   # no q staging copy
            no_halo = sharded.rank_edits_plan(world, 0, K, S, H, dh, E, mask, "bank_edit_runs", no_halo=True)
            assert no_halo == [t for t in sharded.rank_edits_plan(world, 0, K, S, H, dh, E, mask, "bank_edit_runs")
                               if not t.startswith("halo")]


@pytest.mark.parametrize("world,K", GEOMETRY)
def test_one_edit_is_the_bank_runs_sequence(world, K):
    for S, dh in SHAPES:
        for mask in (0, 1):
            for rank in (0, world - 1):
                assert sharded.rank_edits_plan(world, rank, K, S, H, dh, 1, mask, "bank_edit_runs", inv_norm=True) == \
                    sharded.rank_edits_plan(world, rank, K, S, H, dh, 1, mask, "bank_runs", inv_norm=True)


def test_one_rank_behaves_as_today():
    for S, dh in SHAPES:
        assert sharded.rank_edits_plan(1, 0, 4, S, H, dh, 3, 0b101, "bank_edit_runs", inv_norm=True) == \
            sharded.rank_edits_plan(1, 0, 4, S, H, dh, 3, 0b101, "bank", inv_norm=True)


def test_refusals_need_no_device():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    NS, M = _lib.TF_ATTN_NO_SPLIT, _lib.TF_RANK_BANK_EDIT_RUNS

    def plan(world=2, K=4, heads=H, E=2, mask=0, mode=M, flags=NS, dh=40):
        return lib.tf_rank_pivotal_edits_plan(world, 0, K, 256, heads, dh, E, mask, mode, flags, _lib.TF_BF16, buf, len(buf))

    def refused(rc):
        assert rc == -3, rc                                                     # TF_ERR_SHAPE
        assert b"tf_rank_pivotal_edits" in lib.tf_last_error() or b"tf_ext_attn_run_edits" in lib.tf_last_error()
    assert plan() > 0
    assert plan(world=3, K=4, heads=5) > 0                                      # any head count
    refused(plan(mask=0b100))
    assert plan(E=3, mask=0b100) > 0
    refused(plan(flags=NS | _lib.TF_ATTN_INJECT))
    refused(plan(flags=NS | _lib.TF_ATTN_BANK_ONLY))
    refused(plan(flags=NS | _lib.TF_ATTN_SOURCE_ONLY))
    refused(plan(E=0))
    refused(plan(E=_lib.TF_MAX_EDITS + 1))
    refused(plan(dh=48))
    refused(plan(mode=M + 1))
    refused(plan(mode=M | _lib.TF_RANK_NO_HALO | _lib.TF_RANK_INV_NORM))        # the inverse norms need the propagation state
    assert plan(E=_lib.TF_MAX_EDITS, mask=0xA5, K=2) > 0
    assert buf.value.decode().split(";")[-1] == "halo[n=19]"
    refused(plan(mode=_lib.TF_RANK_BANK_RUNS))                                  # mode 2 keeps its refusal for several edits
    strides = (ctypes.c_int64 * 8)()
    rc = lib.tf_rank_pivotal_edits(None, None, None, None, strides, None, None, None, 64, 2, 40, 1.0, 0, _lib.TF_BF16, M, 0, 2,
                                   0, None, 0, None)
    assert rc == -1 and b"tf_rank_pivotal_edits" in lib.tf_last_error()         # TF_ERR_NULL
    with pytest.raises(KeyError):
        sharded.rank_edits_plan(2, 0, 4, 256, H, 40, 2, 0, "edit_runs")         # the mode's name is "bank_edit_runs"
