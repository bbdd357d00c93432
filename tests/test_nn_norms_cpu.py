"""The spread-norm NN family (tests/nn_families.py) has teeth, and the unit-norm family it replaces under the oracle
comparisons had none: three faulty "kernels", emulated in torch on the oracle's rounded inputs, are run through the
comparison the GPU tests use (orc.nn_mismatch_tie_aware at NN_TAU).

  * `raw.argmax`                       -- ignores inv_norm
  * `(raw * inv.roll(1)).argmax`       -- reads inv_norm one row off
  * `(raw * inv[other keyframe]).argmax`

Bounds (from CPU measurements of the family, none from a kernel): every mutant is flagged on at least a quarter of the
rows; the unit-norm family flags 0 rows of the "ignored" mutant (the gap this documents); fewer than 1 % of the oracle's
rows have a top-2 cosine gap <= NN_TAU (the cap that keeps the tie-aware comparison from hiding a failure).

Measured on the CPU (bf16, seeds below; f16 within one or two rows of these), rows flagged of n * S at (n, S, D):

    shape            ignored     one row off   other keyframe   unit-norm family, ignored   oracle near-ties (min top-2 gap)
    (1,  64,   72)    52 /  64    58 /  64      60 /  64        0 /  64                     0 (2.5e-4)
    (1, 100,  320)    87 / 100    97 / 100      91 / 100        0 / 100                     0 (3.1e-5)
    (2, 256, 1280)   462 / 512   501 / 512     491 / 512        0 / 512                     0 (4.0e-5)
    (1,  64, 1096)    58 /  64    62 /  64      61 /  64        0 /  64                     0 (3.8e-5)

i.e. 81-98 % per mutant, row norms spanning a ratio of 15.0-16.2; and on the sharded workers' video-like targets (permuted
pivot rows + 0.1 * noise) at K = 4, n = 2, S = 320, D = 80 the left neighbour's inv_norm is flagged on 2094 of 2560 rows,
0 near-ties.  The tests print these figures (run with -s).
"""
import pytest
import torch

from oracle import tokenflow_oracle as orc
from tests import nn_families as nf
from tests.test_kernels_gpu import NN_TAU

SHAPES = [(1, 64, 72), (1, 100, 320), (2, 256, 1280), (1, 64, 1096)]      # (n, S, D): bk64, rb, deep[split], deep
K, SLOT, OTHER = 2, 1, 0


def _rounded(t):
    return t.float()


def _mutants(tgt, piv, slot, other):
    """(oracle sim, {mutant: indices}) for targets [R, D] against keyframe `slot` of piv [K, S, D] (fp32 copies of the
    rounded 16-bit values: what a kernel reads)."""
    sim = orc.batch_cosine_sim(tgt, piv[slot])
    raw = tgt @ piv[slot].T
    inv = 1.0 / piv.norm(dim=-1)
    return sim, {
        "ignored": raw.argmax(-1),
        "one row off": (raw * inv[slot].roll(1)).argmax(-1),
        "other keyframe": (raw * inv[other]).argmax(-1),
    }


def _flagged(sim, got):
    return orc.nn_mismatch_tie_aware(sim, sim.argmax(-1), got, NN_TAU)[1]


@pytest.mark.parametrize("n,S,D", SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_spread_family_flags_every_inv_norm_mutant(n, S, D, dtype):
    g = torch.Generator().manual_seed(n + S + D)
    piv, gamma, beta = nf.spread_pivots(K, S, D, dtype, g)
    tgt = nf.spread_targets(n * S, D, dtype, g, gamma, beta)
    piv, tgt = _rounded(piv), _rounded(tgt)
    norms = piv.norm(dim=-1)
    assert float(norms.max() / norms.min()) > 8.0           # about 15 at spread = 2
    assert float(piv.abs().max()) < 1024.0                  # far below the f16 maximum
    sim, mut = _mutants(tgt, piv, SLOT, OTHER)
    ties, min_gap = nf.near_tie_rows(sim, NN_TAU)
    rows = n * S
    counts = {name: _flagged(sim, got) for name, got in mut.items()}
    print(f"spread n{n} S{S} D{D} {dtype}: norm ratio {float(norms.max() / norms.min()):.1f}, flagged of {rows} rows: {counts}; "
          f"oracle near-ties {ties} (min top-2 gap {min_gap:.1e})")
    assert ties < 0.01 * rows
    for name, c in counts.items():
        assert c >= rows / 4, f"{name}: only {c} of {rows} rows flagged"
    # the oracle agrees with itself, and the honest kernel (raw * inv) is not flagged
    honest = ((tgt @ piv[SLOT].T) * (1.0 / piv[SLOT].norm(dim=-1))).argmax(-1)
    assert _flagged(sim, honest) == 0


@pytest.mark.parametrize("n,S,D", SHAPES)
def test_unit_norm_family_cannot_see_inv_norm(n, S, D):
    """The gap: on affine-free LayerNorm pivots a kernel that ignores inv_norm returns the oracle's index (tie-aware) on
    every row.  If this ever fails the old family has changed and the comment in tests/nn_families.py is out of date."""
    g = torch.Generator().manual_seed(n + S + D)
    piv = _rounded(nf.unit_pivots(K, S, D, torch.bfloat16, g))
    tgt = _rounded(nf.unit_targets(n * S, D, torch.bfloat16, g))
    sim, mut = _mutants(tgt, piv, SLOT, OTHER)
    c = _flagged(sim, mut["ignored"])
    print(f"unit-norm n{n} S{S} D{D}: 'ignored' mutant flagged on {c} of {n * S} rows")
    assert c == 0


def test_videolike_targets_flag_another_keyframes_inv_norm():
    """The sharded workers' targets (tests/test_sharded_gpu.py: permuted pivot rows plus 0.1 * noise, n copies) on spread
    pivots: every chunk against its own keyframe with the left neighbour's inv_norm."""
    Kv, n, S, D = 4, 2, 320, 80
    g = torch.Generator().manual_seed(0)
    piv = _rounded(nf.spread_pivots(Kv, S, D, torch.bfloat16, g)[0])
    flagged = ties = 0
    for c in range(Kv):
        tgt = orc.bf16_round(piv[c][torch.randperm(S, generator=g)].repeat(n, 1) + 0.1 * torch.randn(n * S, D, generator=g))
        sim, mut = _mutants(tgt, piv, c, (c - 1) % Kv)
        flagged += _flagged(sim, mut["other keyframe"])
        ties += nf.near_tie_rows(sim, NN_TAU)[0]
    rows = Kv * n * S
    print(f"video-like K{Kv} n{n} S{S} D{D}: other keyframe's inv_norm flagged on {flagged} of {rows} rows; near-ties {ties}")
    assert ties < 0.01 * rows
    assert flagged >= rows / 4
