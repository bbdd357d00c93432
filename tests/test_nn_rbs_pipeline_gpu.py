"""The pipelined tile loop of nn_search_rbs_kernel (half-tile phases, the fold of pivot rows 16-31 carried over the barrier
into the next tile's first phase) against the fp32 oracle, on inputs aimed at what a reordered fold can get wrong:

  1. update order decides ties: EXACT duplicate pivot rows (a, b), the target equal to the row, the lower index must win --
     the two halves of one tile (a, a + 16, a % 32 < 16), the same lane's rows across a tile boundary (a, a + 16,
     a % 32 >= 16: the carried half against the next tile's first), the last row of a tile and the first of the next, the
     same two across a split boundary, and rows (0, S - 1); for both keyframes of a chunk, bf16 and f16;
  2. the inverse norms of the carried half are those of ITS tile (sInv is double-buffered and overwritten two tiles on):
     pivot rows are scaled by 2 ** e, e a function of row // 16 with period 5 half-tiles -- the halves of a tile, adjacent
     tiles and tiles two apart (the same sInv buffer) all differ; a stale or early inverse norm is off by a power of two
     and moves the argmax far outside a near-tie.  Every checked target must match the oracle tie-aware at NN_TAU, and at
     most 1 % of the checked targets may be oracle near-ties (precondition, exact duplicates apart);
  3. the winning row sits in the second half of the last tile of a split (the fold behind the loop), with the index of
     its own tile.

Every case asserts its launch plan first.  TJ = 4: two splits of 25 and 24 tiles (odd and even loop lengths), a split
multi-chunk launch, an unsplit one.  TJ = 2: one tile per workgroup (the prologue straight into the final fold), four tiles
per split in a multi-chunk launch, three tiles per workgroup (S = 96).
"""
import pytest
import torch

from tests import kernel_forms as kf
from tests import nn_families as nf
from tests.test_kernel_forms_gpu import DTYPES, _check_nn, _rows_chunk, _rows_single, _sampled
from tests.test_kernels_gpu import NN_TAU
from tests.test_nn_norms_gpu import _search, _slots

pytestmark = pytest.mark.gpu

TILE = 32
EXPONENTS = (0, 3, 1, 4, 2)       # per half-tile (row // 16), period 5: >= 0, so the scaling is exact in f16 too

CASES = [
    (kf.N(42, 1568, 320), ["rbs<TJ=4>[splits=2]", "finalize"]),
    (kf.N(16, 2304, 320, C=8), ["rbs<TJ=4>[splits=2,chunks]"]),
    (kf.N(80, 2304, 320), ["rbs<TJ=4>[splits=1]"]),
    (kf.N(1, 64, 320, P=1), ["rbs<TJ=2>[splits=2]", "finalize"]),
    (kf.N(1, 256, 320, C=8), ["rbs<TJ=2>[splits=2,chunks]"]),
    (kf.N(1, 96, 320, C=8), ["rbs<TJ=2>[splits=1,chunks]"]),
]


def _ops():
    from tokenflow_amd import ops
    return ops


def _splits(plan):
    """Splits of the pivot range in the search launch's token."""
    return int(plan[0].split("splits=")[1].split(",")[0].rstrip("]"))


def _plants(S, splits):
    """Pivot rows to duplicate [(first, duplicate)] and rows that win alone [row]: see the module docstring."""
    tps = -(-(S // TILE) // splits)
    pairs = [(TILE + 5, TILE + 21), (20, 36), (TILE - 1, TILE), (0, S - 1)]
    winners = [S - 2]                                          # second half of the last tile of the last split
    if splits > 1:
        b = tps * TILE
        pairs += [(b - 1, b), (b - 12, b + 4)]
        winners.append(b - 3)                                  # second half of the last tile of split 0
    else:
        winners.append(S - 3)
    used, out = set(), []
    for a, b in pairs:
        if a not in used and b not in used:
            out.append((a, b))
            used.update((a, b))
    winners = [w for w in winners if w not in used]
    assert all(b - a == 16 or (a % TILE == TILE - 1 and b == a + 1) or (a, b) == (0, S - 1) for a, b in out)
    assert winners and all(w % TILE >= 16 for w in winners)
    return out, winners


def _inputs(c, dtype, pairs):
    """Cases checked on every target draw from a CPU generator: the same inputs on every machine, so their near-tie count
    was counted without a GPU (at most 9 of a case's 18 432 rows).  The sampled cases draw on the GPU; thousands of their rows are checked."""
    K, _ = _slots(c)
    S, D = c["S"], c["D"]
    g = torch.Generator(device="cuda" if _sampled(c) else "cpu").manual_seed(c["n_tgt"] + S + c["C"])
    piv = nf.unit_pivots(K, S, D, dtype, g)
    e = torch.tensor(EXPONENTS)[(torch.arange(S) // 16) % len(EXPONENTS)].float().to(piv.device)
    scaled = (piv.float() * torch.exp2(e)[None, :, None]).to(dtype)
    assert torch.equal(scaled.float(), piv.float() * torch.exp2(e)[None, :, None]), "precondition: the scaling is exact"
    for a, b in pairs:
        scaled[:, b] = scaled[:, a]
    return scaled.cuda(), nf.unit_targets(c["C"] * c["n_tgt"], D, dtype, g).cuda()


def _plant(tgt, piv, slot, base, pairs, winners):
    """Targets base .. : the first row of every duplicate pair and every lone winner of keyframe `slot`
    -> {offset from base: the index that must come out}."""
    want = [a for a, _b in pairs] + winners
    for j, r in enumerate(want):
        tgt[base + j] = piv[slot, r]
    return dict(enumerate(want))


@pytest.mark.parametrize("case", range(len(CASES)), ids=[t[0] + f"-S{c['S']}" for c, t in CASES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pipelined_fold_order_norms_and_last_half(case, dtype):
    ops = _ops()
    c, want_plan = CASES[case]
    plan = kf.plan(ops, c)
    assert plan == want_plan
    n_tgt, S, C = c["n_tgt"], c["S"], c["C"]
    splits = _splits(plan)
    pairs, winners = _plants(S, splits)
    npl = len(pairs) + len(winners)
    piv, tgt = _inputs(c, dtype, pairs)
    _, slots = _slots(c)
    dups = [b for _a, b in pairs]
    sampled = _sampled(c)
    # planted targets at the end of a chunk: the last npl for its first keyframe, the npl before them for its second
    plants = {}
    for j in range(C):
        end = (j + 1) * n_tgt
        first, second = (slots[0], slots[1] if len(slots) > 1 else None) if C == 1 else (j, j - 1 if j else None)
        plants[j, 0] = _plant(tgt, piv, first, end - npl, pairs, winners)
        if second is not None:
            plants[j, 1] = _plant(tgt, piv, second, end - 2 * npl, pairs, winners)
    res = _search(ops, c, piv, tgt, ops.pivot_inv_norm(piv))
    n_rows = n_ties = 0
    for j in range(C):
        rows = _rows_single(n_tgt, sampled) if C == 1 else _rows_chunk(j, n_tgt, sampled)
        loc = (rows - j * n_tgt).cuda()
        for p in range(2):
            slot = (slots[p] if p < len(slots) else None) if C == 1 else (j - p if j - p >= 0 else None)
            if slot is None:
                continue
            got = res[p][loc] if C == 1 else res[p][j][loc]
            base = len(rows) - (p + 1) * npl
            sim = _check_nn(got, tgt, piv, slot, rows.cuda(), {base + t: r for t, r in plants[j, p].items()})
            sim[:, dups] = -float("inf")
            n_rows += len(rows)
            n_ties += nf.near_tie_rows(sim, NN_TAU)[0]
    print(f"{plan[0]} S={S} {dtype}: {n_rows} rows checked, {n_ties} oracle near-ties, {len(pairs)} duplicate pairs {pairs}, "
          f"lone winners {winners}")
    assert n_ties <= 0.01 * n_rows, f"precondition: {n_ties} oracle near-ties among {n_rows} checked rows"
