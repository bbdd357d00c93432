"""NN-search input families whose pivot rows have DIFFERENT norms (a plain helper module: no fixtures, no pytest hooks).

The search computes `argmax_j <tgt, piv_j> * inv_norm[j]`.  Pivots that come out of an affine-free LayerNorm all have norm
sqrt(D) up to one rounding, so `inv_norm` is a constant of the argmax and a kernel that reads it from the wrong row, slab,
halo slot or segment -- or not at all -- returns the oracle's index for every row (tests/test_nn_norms_cpu.py measures this).
The family here is what a trained `norm1` emits (per-channel gain and shift) times a per-row scale `2 ** u`,
u ~ U(-spread, spread): not something a LayerNorm can produce, but the C ABI promises cosine similarity for any pivots, and
it is the sharpest probe of the `inv_norm` path.  Row norms span a max / min ratio of about 15 at spread = 2; at f16 the
values stay far below 65504.

Every draw comes from `generator`, on the generator's device, in a fixed order (rows, gamma, beta, row scales)."""
import torch


def _affine_rows(shape, D, generator, gamma, beta):
    x = torch.randn(*shape, D, generator=generator, device=generator.device)
    return torch.nn.functional.layer_norm(x, (D,)) * gamma + beta


def spread_pivots(K, S, D, dtype, generator, spread=2.0):
    """([K, S, D] pivots of `dtype`, gamma [D], beta [D]): layer_norm(randn) * gamma + beta with gamma = 1 + 0.5 * randn,
    beta = 0.3 * randn, every (keyframe, row) scaled by 2 ** U(-spread, spread), rounded once to `dtype`."""
    dev = generator.device
    x = torch.nn.functional.layer_norm(torch.randn(K, S, D, generator=generator, device=dev), (D,))
    gamma = 1.0 + 0.5 * torch.randn(D, generator=generator, device=dev)
    beta = 0.3 * torch.randn(D, generator=generator, device=dev)
    u = (torch.rand(K, S, 1, generator=generator, device=dev) * 2.0 - 1.0) * spread
    return ((x * gamma + beta) * torch.exp2(u)).to(dtype), gamma, beta


def spread_targets(n_rows, D, dtype, generator, gamma, beta):
    """[n_rows, D] iid targets of the same `norm1` (the pivots' gamma / beta), without the row scale: the cosine does not
    care about the target's scale."""
    return _affine_rows((n_rows,), D, generator, gamma, beta).to(dtype)


def unit_pivots(K, S, D, dtype, generator):
    """The family the suite used everywhere before: affine-free LayerNorm rows (norm sqrt(D) up to one rounding) for pivots
    and targets alike.  Kept so that tests/test_nn_norms_cpu.py can document that it cannot see `inv_norm`."""
    dev = generator.device
    return torch.nn.functional.layer_norm(torch.randn(K, S, D, generator=generator, device=dev), (D,)).to(dtype)


def unit_targets(n_rows, D, dtype, generator):
    dev = generator.device
    return torch.nn.functional.layer_norm(torch.randn(n_rows, D, generator=generator, device=dev), (D,)).to(dtype)


def near_tie_rows(sim, tau):
    """Number of rows of the similarity matrix whose top-2 gap is <= tau, and the smallest gap: the rows on which a
    tie-aware comparison would accept either index."""
    top = sim.topk(2, dim=-1).values
    gap = top[:, 0] - top[:, 1]
    return int((gap <= tau).sum()), float(gap.min())
