"""The CPU reference of the ragged chunk runs (tests/ragged_forms.py) and the inputs the GPU tests feed it: the reference is
consistent with itself, and every MUTANT -- one thing each that a ragged kernel can get wrong -- gives another result on these
inputs, so a kernel with that fault fails tests/test_ragged_gpu.py.

Run at the two smallest shapes of the GPU table; the frame lists of the large shapes are run at a small S here (what a gather
decodes depends on the frame counts alone), their panel arithmetic at the real S."""
import pytest
import torch

from tests import nn_exact as nx
from tests import ragged_forms as rf

SHAPES = [(45, 72, "bk64"), (45, 320, "rb")]
RAGGED_LISTS = [f for f in rf.SMALL_FRAMES + rf.LARGE_FRAMES if len(set(f)) > 1]
DT = torch.bfloat16


def _tensors(rg, nb=3, seed=1):
    g = torch.Generator().manual_seed(seed)
    F = sum(rg.frames)
    kf = torch.randn(nb * rg.K, rg.S, rg.D, generator=g).to(DT)
    res = torch.randn(nb * F, rg.S, rg.D, generator=g).to(DT)
    return kf, res


@pytest.fixture(scope="module")
def ragged():
    cache = {}

    def get(frames, S, D, family):
        key = (tuple(frames), S, D, family)
        if key not in cache:
            cache[key] = rf.Ragged(frames, S, D, family)
        return cache[key]
    return get


@pytest.mark.parametrize("frames", rf.SMALL_FRAMES + rf.LARGE_FRAMES, ids=str)
def test_frame_by_frame_is_the_per_chunk_reference(ragged, frames):
    S, D, _ = SHAPES[0]
    rg = ragged(frames, S, D, "pool")
    kf, res = _tensors(rg)
    for mask, slot0 in rf.masks(rg.C):
        want = rg.indices(slot0, mask)
        for r in (None, res):
            ref = rf.reference(kf, frames, slot0, mask, want, r, torch.float32, 3)
            by_frame = rf.reference_by_frame(kf, rf.frame_plan(frames, slot0, mask, want, S), r, torch.float32, 3)
            assert torch.equal(nx.bits(ref), nx.bits(by_frame))


def test_weights_are_per_frame_of_the_run():
    w = rf.weights([3, 1, 2])
    assert w.shape == (6,) and w.dtype == torch.float32
    assert torch.equal(w[:3], rf.orc.blend_weights(3, 1)) and torch.equal(w[3:4], rf.orc.blend_weights(1, 1))
    assert torch.equal(w[4:], rf.orc.blend_weights(2, 1))


@pytest.mark.parametrize("mutant", rf.MUTANTS)
@pytest.mark.parametrize("frames", RAGGED_LISTS, ids=str)
@pytest.mark.parametrize("S,D,form", SHAPES)
def test_gather_mutants_are_caught(ragged, S, D, form, frames, mutant):
    rg = ragged(frames, S, D, "dense")
    kf, res = _tensors(rg)
    caught = 0
    for mask, slot0 in rf.masks(rg.C):
        want = rg.indices(slot0, mask)
        ref = rf.reference(kf, frames, slot0, mask, want, res, torch.float32, 3)
        bad = rf.reference_by_frame(kf, rf.frame_plan(frames, slot0, mask, want, S, mutant), res, torch.float32, 3)
        differs = not torch.equal(nx.bits(ref), nx.bits(bad))
        if mutant == "single_rounding_on_wrong_chunk":
            assert differs == (mask != 0), (mask, slot0)      # without a one-keyframe chunk nothing is rounded
        else:
            assert differs, (mask, slot0)
        caught += differs
    assert caught


@pytest.mark.parametrize("family", ["pool", "rollcall"])
@pytest.mark.parametrize("frames", RAGGED_LISTS, ids=str)
@pytest.mark.parametrize("S,D,form", SHAPES)
def test_unsearched_last_panel_is_caught(ragged, S, D, form, frames, family):
    """pool aims every 8th target at the last pivot row, roll-call makes every index the answer of some target: the rows of a
    chunk's partial last panel do not all want index 0."""
    rg = ragged(frames, S, D, family)
    panel = rf.PANEL[form]
    assert any((n * S) % panel for n in frames)
    for mask, slot0 in rf.masks(rg.C):
        want = rg.indices(slot0, mask)
        bad = rf.unsearched_tail(want, frames, S, panel)
        for j, n in enumerate(frames):
            if (n * S) % panel:
                assert all(not torch.equal(a, b) for a, b in zip(want[j], bad[j])), (j, mask)


@pytest.mark.parametrize("S,D,form", rf.LARGE)
def test_large_shapes_end_in_partial_panels(S, D, form):
    for frames in rf.LARGE_FRAMES:
        assert all((n * S) % rf.PANEL[form] for n in frames)


@pytest.mark.parametrize("family", nx.FAMILIES)
@pytest.mark.parametrize("frames", [[3, 1, 2, 5], [2, 3, 2]], ids=str)
def test_next_slot_inv_norm_is_caught_by_the_scaled_variants(ragged, frames, family):
    S, D, _ = SHAPES[1]
    rg = ragged(frames, S, D, family)
    for mask, slot0 in rf.masks(rg.C):
        want = rg.indices(slot0, mask)
        bad = rf.next_slot_inv_norm(rg, slot0, mask)
        for j in range(rg.C):
            assert all(not torch.equal(a, b) for a, b in zip(want[j], bad[j])), (j, mask)
