"""The exact-arithmetic NN inputs have teeth (no GPU): on the inputs tests/test_nn_exact_gpu.py runs -- every NN case of
tests/kernel_forms.CASES, all targets of the small cases and a row sample of the large ones --

  * the preconditions of tests/nn_exact.py hold: one norm per keyframe (dense: D, sparse: 24), every score an integer, pairwise
    distinct roll-call rows, the pool's last row a row of its own; `first_argmax` agrees with a brute-force Python loop;
    the roll-call's closed form agrees with `first_argmax` and covers S of S indices of every searched keyframe;
  * the figures of each (case, family) are printed (the `NNEXACT` lines; profiles/r23_nn_exact.txt): the share of targets with
    an exact tie at the top, the largest number of tied candidates, the number of distinct winning indices;
  * every mutant of the reference -- the ways a subtly wrong kernel goes wrong -- differs from the exact reference on at least
    8 checked targets of every case it applies to, all families of the case taken together (`MIN_CAUGHT`; the `MUTANT` lines).
"""
import pytest
import torch

from tests import kernel_forms as kf
from tests import nn_exact as nx

MIN_CAUGHT = 8
ROWS = 1024       # checked targets per chunk of the large cases: the first 64 (the pool's planted rows among them) + a sample


def _checked_rows(n_tgt, j):
    if n_tgt <= 2 * ROWS:
        return None
    g = torch.Generator().manual_seed(1000 + j)
    return torch.cat([torch.arange(64), torch.randint(64, n_tgt, (ROWS - 64,), generator=g)])


def _checked_chunks(C):
    return sorted({0, 1, C - 1} & set(range(C)))


# ------------------------------------------------------------------------------------------------------------ mutants
class Ctx:
    """One (chunk, slot) of a case: checked targets tgt [R, D] and the slot's pivots piv [S, D] (fp64, unscaled), their scores
    sim [R, S], the kernel's tile size, the scaled variant's exponents of this slot (e) and of slot k + 1 (e_next)."""

    def __init__(self, tgt, piv, tile, e, e_next):
        self.tgt, self.piv, self.tile, self.e, self.e_next = tgt, piv, tile, e, e_next
        self.sim = tgt @ piv.T
        self.S = piv.shape[0]


def _first(sim):
    return nx.first_of_max(sim)[0]


def last_index(x):
    hit = x.sim == x.sim.amax(-1, keepdim=True)
    return torch.where(hit, torch.arange(x.S), -1).amax(-1)


def _tiled_later_wins(sim, T):
    """Exact first index inside every tile of T rows; across tiles the LATER tile wins on equality (`>=` in the running merge)."""
    N, S = sim.shape
    nt = (S + T - 1) // T
    s = torch.nn.functional.pad(sim, (0, nt * T - S), value=float("-inf")).view(N, nt, T)
    inside = _first(s.reshape(N * nt, T)).view(N, nt)
    tmax = s.amax(-1)
    tile = torch.where(tmax == tmax.amax(-1, keepdim=True), torch.arange(nt), -1).amax(-1)
    return tile * T + inside.gather(1, tile.view(N, 1)).squeeze(1)


def tiled(T):
    def f(x):
        return _tiled_later_wins(x.sim, T) if x.S > T else None
    f.__name__ = f"tile{T}_later_wins"
    return f


def interleaved_no_index_compare(x):
    """Two row sets (groups of 4 rows alternating, the MFMA C/D map) reduced exactly, merged on the value alone: set A keeps a
    tie although B's index is smaller."""
    grp = (torch.arange(x.S) // 4) % 2
    ia, ib = _first(x.sim.masked_fill(grp == 1, float("-inf"))), _first(x.sim.masked_fill(grp == 0, float("-inf")))
    va, vb = x.sim.gather(1, ia.view(-1, 1)).squeeze(1), x.sim.gather(1, ib.view(-1, 1)).squeeze(1)
    return torch.where(vb > va, ib, ia)


def splits_descending(x):
    """The pivot range in (up to) 4 splits of whole tiles, merged from the last split down with a strict `>`."""
    n_tiles = (x.S + x.tile - 1) // x.tile
    splits = min(4, n_tiles)
    if splits < 2:
        return None
    return _tiled_later_wins(x.sim, (n_tiles + splits - 1) // splits * x.tile)


def drop_last_row(x):
    return _first(x.sim[:, :x.S - 1])


def drop_last_ragged_tile(x):
    keep = x.S - x.S % x.tile
    return _first(x.sim[:, :keep]) if 0 < keep < x.S else None


def drop_last_16_features(x):
    return _first(x.tgt[:, :-16] @ x.piv[:, :-16].T)


def inv_norm_of_next_row(x):
    """Scaled variant: the score of row j carries 2^e(j) from the pivot and 2^-e(j+1) from the misplaced inverse norm."""
    return _first(x.sim * torch.exp2(x.e - torch.roll(x.e, -1)))


def inv_norm_of_next_slot(x):
    return _first(x.sim * torch.exp2(x.e - x.e_next))


MUTANTS = [last_index, tiled(32), tiled(64), tiled(128), tiled(256), interleaved_no_index_compare, splits_descending,
           drop_last_row, drop_last_ragged_tile, drop_last_16_features, inv_norm_of_next_row, inv_norm_of_next_slot]


# -------------------------------------------------------------------------------------------------------------- tests
def test_first_argmax_against_brute_force():
    for family in nx.FAMILIES:
        inp = nx.Inputs(2, 13, 72, 26, [[1, 0]], family, seed=5)
        tgt = inp.targets(0)
        for slot in (1, 0):
            got, mult = nx.first_argmax(tgt, inp.piv[slot], block=7, want_mult=True)
            assert torch.equal(got, nx.brute_first_argmax(tgt, inp.piv[slot])), family
            assert int(mult.min()) >= 1
    sim = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, -1.0, 0.5, 0.5]], dtype=torch.float64)
    idx, mult = nx.first_of_max(sim)
    assert idx.tolist() == [1, 0, 2] and mult.tolist() == [2, 4, 2]


def test_values_are_exact_in_both_types():
    inp = nx.Inputs(2, 40, 72, 40, [[1, 0]], "sparse", seed=1)
    for dtype in (torch.bfloat16, torch.float16):
        for scaled in (False, True):
            p = inp.pivots("cpu", dtype, scaled)
            want = inp.piv.double() * (torch.exp2(inp.exps.double()).unsqueeze(-1) if scaled else 1.0)
            assert torch.equal(p.double(), want)
        for huge in (False, True):
            assert len(nx.edge_values(dtype, huge)) == (8 if huge else 6)
    assert bool((nx.bits(torch.tensor([0.0])) != nx.bits(torch.tensor([-0.0]))).all())


@pytest.mark.parametrize("form,i", nx.NN_CASES, ids=[f"{f}-{i}" for f, i in nx.NN_CASES])
def test_preconditions_and_mutants(form, i):
    c = kf.CASES[form][i]
    S, D, n_tgt = c["S"], c["D"], c["n_tgt"]
    K, chunks = nx.geometry(c)
    tile = nx.tile_of(form)
    caught = {m.__name__: None for m in MUTANTS}
    for family in nx.FAMILIES:
        inp = nx.Inputs.of_case(c, family)
        piv = inp.piv.double()
        # one norm per keyframe, integer scores
        norm2 = (piv * piv).sum(-1)
        assert bool((norm2 == (nx.SUPPORT if family == "sparse" else D)).all()), f"{family}: row norms differ"
        if family == "rollcall":
            assert all(torch.unique(inp.piv[k], dim=0).shape[0] == S for k in range(K)), "roll-call rows are not distinct"
        if family == "pool":
            assert not bool((inp.piv[:, :S - 1] == inp.piv[:, S - 1:]).all(-1).any()), "the pool's last row is not its own"
        tied = total = 0
        most = 0
        winners = set()
        for j in _checked_chunks(len(chunks)):
            rows = _checked_rows(n_tgt, j)
            tgt = inp.targets(j, rows=rows).double()
            for slot in chunks[j]:
                x = Ctx(tgt, piv[slot], tile, inp.exps[slot].double(), inp.exps[(slot + 1) % K].double())
                assert bool((x.sim == x.sim.round()).all()) and float(x.sim.abs().max()) <= D
                ref, mult = nx.first_of_max(x.sim)
                tied += int((mult > 1).sum())
                most = max(most, int(mult.max()))
                total += len(ref)
                winners |= set(ref.tolist())
                if family == "rollcall":
                    want = inp.rollcall_want(j, slot)
                    assert sorted(set(want.tolist())) == list(range(S)), f"roll-call: chunk {j} slot {slot} misses indices"
                    assert torch.equal(ref, want if rows is None else want[rows]) and int(mult.max()) == 1
                if family == "pool":
                    aimed = inp.aims(j)[0] == slot
                    aimed = aimed if rows is None else aimed[rows]
                    assert bool((x.sim.amax(-1)[aimed] == D).all()), "pool: a target's row is not in its keyframe"
                for m in MUTANTS:
                    got = m(x)
                    if got is not None:
                        caught[m.__name__] = (caught[m.__name__] or 0) + int((got != ref).sum())
        print(f"NNEXACT {form}-{i} {kf.nn_key(c)} {family}: checked {total} (target, keyframe) pairs, tie at the top "
              f"{100.0 * tied / total:.1f} %, most candidates tied {most}, distinct winners {len(winners)}"
              + (f", roll-call coverage {S} of {S}" if family == "rollcall" else ""))
    for name, cnt in caught.items():
        print(f"MUTANT {form}-{i} {name}: " + ("does not apply" if cnt is None else f"differs on {cnt} targets"))
        assert cnt is None or cnt >= MIN_CAUGHT, f"{form}-{i}: mutant {name} differs on {cnt} targets only"
    # the mutants that must apply everywhere
    for name in ("last_index", "interleaved_no_index_compare", "drop_last_row", "drop_last_16_features",
                 "inv_norm_of_next_row", "inv_norm_of_next_slot"):
        assert caught[name] is not None
