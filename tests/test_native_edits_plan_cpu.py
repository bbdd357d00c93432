"""The native rank executor for multi-edit batches, host side: tf_rank_pivotal_edits_plan records the sequence ONE
tf_rank_pivotal_edits call issues -- by running that call's own body with the record switch set (no device, stream or
communicator) -- and the argument checks of the call come before anything touches the device."""
import ctypes
import re

import pytest

from tokenflow_amd import _lib, ops, sharded
from tokenflow_amd.workload import CONFIGS

NAMES = ("tf_rank_pivotal_edits_workspace_bytes", "tf_rank_pivotal_edits", "tf_rank_pivotal_edits_plan")
H = 8
LEVELS = [(S, D // heads) for S, D, heads in CONFIGS["cfg2"].levels]          # (S, Dh) of the four UNet levels
WORLDS = [(8, 8), (2, 5)]                                                     # (world, K)
CASES = [(E, m) for E in (2, 3) for m in range(1 << E)]
COLLECTIVE = re.compile(r"(a2a|gather)\[slabs=(\d+)\]")


def _counts(E, mask):
    n_non = E - bin(mask).count("1")
    return (1 if mask else 0), n_non


def _runs(world, K):
    return [K // world + (1 if r < K % world else 0) for r in range(world)]


def _split(plan):
    """(tokens in front of the first collective, attention tokens behind it, the rest from the second collective or the halo)"""
    ic = [i for i, t in enumerate(plan) if COLLECTIVE.fullmatch(t)]
    end = ic[1] if len(ic) > 1 else next((i for i, t in enumerate(plan) if t.startswith("halo[")), len(plan))
    return plan[:ic[0]], plan[ic[0] + 1:end], plan[end:], [plan[i] for i in ic]


def test_exports_and_classes():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert issubclass(sharded.NativeEditShard, sharded.NativeShard)
    assert sharded.NativeEditShard.supports_edits is True
    assert sharded.NativeShard.supports_edits is False


@pytest.mark.parametrize("E,mask", CASES)
@pytest.mark.parametrize("world,K", WORLDS)
@pytest.mark.parametrize("mode", ["heads", "bank"])
def test_slab_counts(world, K, mode, E, mask):
    any_, n_non = _counts(E, mask)
    nq, B = any_ + 2 * n_non, 1 + 2 * E
    mixed = 0 < bin(mask).count("1") < E
    for S, dh in LEVELS:
        for rank in (0, world - 1):
            for inv in (False, True):
                plan = sharded.rank_edits_plan(world, rank, K, S, H, dh, E, mask, mode, inv_norm=inv)
                head, _attn, tail, coll = _split(plan)
                ns = (2 * nq if mode == "heads" else nq) + 2 * E
                assert head[0] == ("pack+inv" if inv else "pack") + f"[ns={ns}]"
                assert sum(t.startswith("pack") for t in plan) == 1
                if mode == "bank" and mixed:
                    assert head[1:] == [f"qcompact[ns={nq}]"]
                else:
                    assert head[1:] == [] and not any(t.startswith("qcompact") for t in plan)
                if mode == "heads":
                    assert coll == [f"a2a[slabs={ns}]", f"a2a[slabs={2 * E}]"]
                    assert tail == [f"a2a[slabs={2 * E}]", f"unpack[nb={2 * E}]", f"halo[n={2 + B}]"]
                else:
                    assert coll == [f"gather[slabs={ns}]"]
                    assert tail == [f"halo[n={2 + B}]"]
            no_halo = sharded.rank_edits_plan(world, 0, K, S, H, dh, E, mask, mode, no_halo=True)
            assert not any(t.startswith("halo") for t in no_halo)
            assert no_halo == [t for t in sharded.rank_edits_plan(world, 0, K, S, H, dh, E, mask, mode)
                               if not t.startswith("halo")]


@pytest.mark.parametrize("E,mask", CASES)
@pytest.mark.parametrize("world,K", WORLDS)
@pytest.mark.parametrize("no_split", [True, False])
def test_attention_tokens_are_the_part_plans(world, K, E, mask, no_split):
    """Between the collectives: the bank part as `ops.attn_edits_part_plan` gives it for the exchanged buffer, then the source
    part of the rank's own frames."""
    runs = _runs(world, K)
    for S, dh in LEVELS:
        for rank in (0, world - 1):
            Kl = runs[rank]
            src = ops.attn_edits_part_plan(Kl, Kl, S, H, dh, E, mask, part="source", no_split=no_split)
            for mode, bank_args in (("heads", (K, K, S, H // world, dh)), ("bank", (K, Kl, S, H, dh))):
                bank = ops.attn_edits_part_plan(*bank_args, E, mask, part="bank", qk_compact=True, no_split=no_split)
                plan = sharded.rank_edits_plan(world, rank, K, S, H, dh, E, mask, mode, no_split=no_split)
                assert _split(plan)[1] == bank + src, (mode, S, dh, rank, plan)


def test_one_rank_is_the_masked_call():
    for S, dh in LEVELS:
        plan = sharded.rank_edits_plan(1, 0, 8, S, H, dh, 3, 0b101, "heads", inv_norm=True)
        assert plan == ["inv_norm"] + ops.attn_edits_plan(8, 8, S, H, dh, False, 3, inject_mask=0b101, no_split=True)


@pytest.mark.parametrize("world,K", WORLDS)
def test_one_edit_is_the_single_edit_executor(world, K):
    """n_edits = 1 delegates to tf_rank_pivotal: ITS slab counts (the bank form gathers the source's k and v too)."""
    for S, dh in LEVELS:
        for mask, n_heads, n_bank in ((0, 6, 6), (1, 4, 4)):
            heads = sharded.rank_edits_plan(world, 1, K, S, H, dh, 1, mask, "heads")
            assert heads[0] == f"pack[ns={n_heads}]" and heads[1] == f"a2a[slabs={n_heads}]"
            assert heads[-3:] == ["a2a[slabs=2]", "unpack[nb=2]", "halo[n=5]"]
            bank = sharded.rank_edits_plan(world, 1, K, S, H, dh, 1, mask, "bank")
            assert bank[0] == f"pack[ns={n_bank}]" and bank[1] == f"gather[slabs={n_bank}]" and bank[-1] == "halo[n=5]"
            Kl = _runs(world, K)[1]
            assert bank[2:-1] == ops.attn_plan(K, Kl, S, H, dh, bool(mask), no_split=True)


def test_refusals_need_no_device():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    NS = _lib.TF_ATTN_NO_SPLIT

    def plan(world=2, K=4, heads=H, E=2, mask=0, mode=_lib.TF_RANK_HEADS, flags=NS):
        return lib.tf_rank_pivotal_edits_plan(world, 0, K, 256, heads, 160, E, mask, mode, flags, _lib.TF_BF16, buf, len(buf))

    def refused(rc):
        assert rc == -3, rc                                                     # TF_ERR_SHAPE
        assert b"tf_rank_pivotal_edits" in lib.tf_last_error()
    assert plan() > 0
    refused(plan(mode=_lib.TF_RANK_BANK_RUNS))                                  # no multi-edit form
    assert plan(E=1, mode=_lib.TF_RANK_BANK_RUNS) > 0                           # one edit: the single-edit executor's
    refused(plan(world=3, heads=8))                                             # heads do not divide
    assert plan(world=3, heads=8, mode=_lib.TF_RANK_BANK) > 0
    refused(plan(mask=0b100))                                                   # a mask bit at or above E
    assert plan(E=3, mask=0b100) > 0
    refused(plan(flags=NS | _lib.TF_ATTN_INJECT))                               # the mask is the injection state
    refused(plan(flags=NS | _lib.TF_ATTN_BANK_ONLY))
    refused(plan(E=0))
    refused(plan(E=_lib.TF_MAX_EDITS + 1))
    assert plan(E=_lib.TF_MAX_EDITS, mask=0xA5, K=2) > 0                        # 19 halo messages
    assert buf.value.decode().split(";")[-1] == "halo[n=19]"
    strides = (ctypes.c_int64 * 8)()
    rc = lib.tf_rank_pivotal_edits(None, None, None, None, strides, None, None, None, 64, 2, 40, 1.0, 0, _lib.TF_BF16,
                                   _lib.TF_RANK_HEADS, 0, 2, 0, None, 0, None)
    assert rc == -1 and b"tf_rank_pivotal_edits" in lib.tf_last_error()         # TF_ERR_NULL
    assert lib.tf_rank_pivotal_edits_workspace_bytes(None, 64, 2, 40, 2, _lib.TF_BF16) == 0
    with pytest.raises(_lib.TokenflowHipError, match="TF_RANK_BANK_RUNS"):
        sharded.rank_edits_plan(2, 0, 4, 256, H, 160, 2, 0, "bank_runs")
