"""Inputs that make the NN search's scores exact, the plain first-index reference they are held to, and the CPU reference of
the propagation family (gather + blend + residual) on the indices that follow.

Every score the search kernels compare is  dot(target, pivot) * inv_norm[pivot].  The families built here make the dot
products small integers -- exact in fp32 under any summation order, 16- or 32-wide MFMA steps alike -- and give every pivot
row of a keyframe the same norm, so all rows share ONE fp32 inv_norm and distinct integers times that common positive factor
stay strictly ordered.  The kernel's argmax is then the integer argmax with the first index on ties, exactly: no tolerance,
no tie-awareness, every target.

  * dense: pivots and targets iid +-1 over all D features (norm^2 = D, |dot| <= D <= 1536);
  * sparse: +-1 on a fixed support of 24 features spread evenly over D (one at least in every 64-wide chunk), 0 elsewhere
    (norm^2 = 24): dots in -24 .. 24, so ties of two, three and more candidates at random distances;
  * pool: the rows of a keyframe are drawn with replacement from ceil(S / 4) distinct dense rows and the targets are rows of
    the searched keyframes: the maximum D is attained at every copy and the FIRST copy must win; copies sit at random
    positions, so every merge distance of the kernels (lane, 16-lane group, wave half, tile, ring phase, split) is hit many
    times.  The last row of every keyframe is a row of its own that occurs nowhere else, and every 8th target of a slot
    is aimed at it: a kernel that drops the last row or the last ragged tile loses exactly there;
  * roll-call: S pairwise distinct dense rows; every keyframe holds all of them in a permutation of its own, and target t of
    a chunk is row perm[t mod S] of the chunk's first keyframe -- so in EVERY searched keyframe each index 0 .. S-1 is the
    unique answer of some target, also where a chunk has S targets for two keyframes (n = 1);
  * scaled variant of each: pivot row j of slot k times 2^e(k, j), e in -3 .. 3.  inv_norm scales by exactly 2^-e
    (1.0f / sqrtf(x) under a scaling of x by 4^e), products and partial sums stay exact multiples of 2^e, so every score is
    bit-identical to the unscaled one and the expected indices do not change -- but an inv_norm taken from a neighbouring
    row, slot, halo or chunk is off by a power of two and loses exactly.

All values are exactly representable in bf16 and f16.  Everything is drawn from CPU generators with fixed seeds (`Inputs`),
so tests/test_nn_exact_cpu.py checks the very inputs tests/test_nn_exact_gpu.py runs.
"""
import re
import zlib

import torch

from tests import kernel_forms as kf

FAMILIES = ("dense", "sparse", "pool", "rollcall")
SUPPORT = 24
E_MAX = 3
# pivot rows per tile of the search kernels (nn_search.hip: nn_plan's shape(tn, tm) calls)
TILE = {"rb": 32, "rbs": 32, "glds": 256, "wide": 128, "bk64": 128, "bk128": 128, "deep": 64, "finalize": 32}

NN_CASES = [(f, i) for f, cs in kf.CASES.items() for i, c in enumerate(cs) if "n_tgt" in c]


def kernel_of(form):
    return re.match(r"[a-z0-9]+", form).group(0)


def tile_of(form):
    return TILE[kernel_of(form)]


def geometry(c):
    """(K, slots per chunk) of a kernel_forms NN case: C = 1 searches slot 1 (and 0, P = 2) of two keyframes; C > 1 is
    propagate_chunks with first_single over K = C keyframes: chunk 0 slot 0 alone, chunk j slots j and j - 1."""
    if c["C"] == 1:
        return 2, [[1, 0] if c["P"] == 2 else [1]]
    return c["C"], [[j, j - 1] if j else [0] for j in range(c["C"])]


def case_seed(c, family, salt=0):
    return zlib.crc32(f"{kf.nn_key(c)}/{family}/{salt}".encode())


def support(D):
    """The sparse family's 24 features: floor(i D / 24), a spacing of D / 24 <= 64."""
    pos = (torch.arange(SUPPORT) * D) // SUPPORT
    assert len(set(pos.tolist())) == SUPPORT and D / SUPPORT <= 64
    return pos


def _pm1(shape, g):
    return torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1


class Inputs:
    """One family's pivots and targets for a call that searches `chunks[j]` (one or two keyframe slots) for chunk j's n_tgt
    targets.  piv: int8 [K, S, D] (the unscaled values -1 / 0 / 1), exps: int8 [K, S] (the scaled variant's exponents)."""

    def __init__(self, K, S, D, n_tgt, chunks, family, seed):
        assert family in FAMILIES
        self.K, self.S, self.D, self.n_tgt, self.chunks, self.family, self.seed = K, S, D, n_tgt, chunks, family, seed
        g = torch.Generator().manual_seed(seed)
        if family == "dense":
            self.piv = _pm1((K, S, D), g)
        elif family == "sparse":
            self.piv = torch.zeros(K, S, D, dtype=torch.int8)
            self.piv[..., support(D)] = _pm1((K, S, SUPPORT), g)
        elif family == "pool":
            npool = (S + 3) // 4
            base = _pm1((K, npool, D), g)
            draw = torch.randint(0, npool, (K, S), generator=g)
            self.piv = torch.stack([base[k, draw[k]] for k in range(K)])
            self.piv[:, S - 1] = _pm1((K, D), g)          # a row of its own at the very end
        else:
            base = _pm1((S, D), g)
            self.sigma = torch.stack([torch.randperm(S, generator=g) for _ in range(K)])
            self.piv = base[self.sigma]
        self.exps = torch.randint(-E_MAX, E_MAX + 1, (K, S), generator=g, dtype=torch.int8)
        self._dev = {}

    @classmethod
    def of_case(cls, c, family, salt=0):
        K, chunks = geometry(c)
        return cls(K, c["S"], c["D"], c["n_tgt"], chunks, family, case_seed(c, family, salt))

    # ---- pivots
    def pivots(self, device, dtype, scaled):
        p = self.piv.to(device).float()
        if scaled:
            p = p * torch.exp2(self.exps.to(device).float()).unsqueeze(-1)
        return p.to(dtype)

    def scale(self, device):
        """2^-e [K, S] fp32: what inv_norm of the scaled rows is multiplied by."""
        return torch.exp2(-self.exps.to(device).float())

    # ---- targets
    def _gen(self, j):
        return torch.Generator().manual_seed(self.seed * 64 + j + 1)

    def aims(self, j):
        """pool / roll-call: (slot, row) [n_tgt] of the pivot row every target of chunk j is a copy of."""
        ss, S, t = self.chunks[j], self.S, torch.arange(self.n_tgt)
        g = self._gen(j)
        if self.family == "pool":
            slot = torch.as_tensor(ss)[t % len(ss)]
            row = torch.randint(0, S, (self.n_tgt,), generator=g)
            row[(t // len(ss)) % 8 == 0] = S - 1
            return slot, row
        perm = torch.randperm(S, generator=g)
        return torch.full_like(t, ss[0]), perm[t % S]

    def rollcall_want(self, j, slot):
        """Closed form of the roll-call: the one index of `slot` that holds target t's row, [n_tgt]."""
        s0, row = self.aims(j)
        inv = torch.empty(self.S, dtype=torch.long)
        inv[self.sigma[slot]] = torch.arange(self.S)
        return inv[self.sigma[s0[0]][row]]

    def targets(self, j, device="cpu", rows=None):
        """int8 [n_tgt, D] (or the selected `rows` of them): chunk j's targets, the same values on either device."""
        if self.family in ("pool", "rollcall"):
            slot, row = self.aims(j)
            if rows is not None:
                slot, row = slot[rows], row[rows]
            if device not in self._dev:
                self._dev = {device: self.piv.to(device)}
            return self._dev[device][slot.to(device), row.to(device)]
        g = self._gen(j)
        if self.family == "dense":
            t = _pm1((self.n_tgt, self.D), g)
            return (t if rows is None else t[rows]).to(device)
        v = _pm1((self.n_tgt, SUPPORT), g)
        v = (v if rows is None else v[rows]).to(device)
        t = torch.zeros(v.shape[0], self.D, dtype=torch.int8, device=device)
        t[:, support(self.D).to(device)] = v
        return t


# ------------------------------------------------------------------------------------------------------ the reference
def first_of_max(sim):
    """sim [N, S] -> the smallest index that attains the row maximum (never argmax's own tie rule), and how many attain it."""
    S = sim.shape[1]
    hit = sim == sim.amax(-1, keepdim=True)
    ar = torch.arange(S, device=sim.device)
    return torch.where(hit, ar, S).amin(-1), hit.sum(-1)


def first_argmax(tgt, piv, block=4096, want_mult=False):
    """tgt [N, D], piv [S, D] (any dtype holding the exact values) -> int64 [N]: fp64 dot products in row blocks on the tensors'
    device, the row maximum, the first index that attains it.  want_mult: also the number of candidates tied at the top."""
    p = piv.double().T.contiguous()
    idx, mult = [], []
    for r0 in range(0, tgt.shape[0], block):
        i, m = first_of_max(tgt[r0:r0 + block].double() @ p)
        idx.append(i)
        mult.append(m)
    return (torch.cat(idx), torch.cat(mult)) if want_mult else torch.cat(idx)


def brute_first_argmax(tgt, piv):
    """The same in plain Python integers (tiny sizes)."""
    out = []
    for t in tgt.tolist():
        best, arg = None, -1
        for j, p in enumerate(piv.tolist()):
            d = sum(int(a) * int(b) for a, b in zip(t, p))
            if best is None or d > best:
                best, arg = d, j
        out.append(arg)
    return torch.tensor(out)


def locate(form, token, S, idx):
    """Where pivot row idx sits in the kernel's merge tree: tile, split (from the plan token's splits=), 16-lane group and
    wave half inside its tile."""
    tile = tile_of(form)
    m = re.search(r"splits=(\d+)", token)
    splits = int(m.group(1)) if m else 1
    n_tiles = (S + tile - 1) // tile
    tps = (n_tiles + splits - 1) // splits
    t = idx // tile
    return f"row {idx}: tile {t} of {n_tiles} ({tile} rows), split {t // tps} of {splits}, row {idx % tile} of its tile (16-row group " \
           f"{(idx % tile) // 16}, 32-row half {(idx % tile) // 32})"


# ------------------------------------------------------------------------------------- propagation: the CPU reference
def bits(t):
    """The bit patterns of a float tensor (so that -0 and +0 differ and NaNs compare)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def edge_values(dtype, huge=True):
    """+-0, the smallest normal, a subnormal and (huge) half the largest finite value of `dtype`."""
    fi = torch.finfo(dtype)
    vals = [0.0, -0.0, fi.tiny, -fi.tiny, fi.tiny / 4, -fi.tiny / 4] + ([fi.max / 2, -fi.max / 2] if huge else [])
    v = torch.tensor(vals, dtype=torch.float64).to(dtype)
    assert bool((v.double() == torch.tensor(vals, dtype=torch.float64)).all())
    return v


def edge_frame(S, D, dtype, shift, huge=True):
    """[S, D]: the edge values, cycling along the features with a different phase in every row."""
    v = edge_values(dtype, huge)
    return v[(torch.arange(S).view(S, 1) * 3 + torch.arange(D).view(1, D) + shift) % len(v)]


def propagation_reference(kf_out, slots, want, w, residual, out_dtype, nb, n):
    """The reference's own op order on the CPU (oracle.tokenflow_oracle.gather_blend, tokenflow_utils.py:362-397), chunk by
    chunk on the exact indices `want[j]` (one int64 [n*S] per searched slot of `slots[j]`):
      two keyframes: w1 * a1 + (1 - w1) * a2 (+ residual) in fp32, separate torch ops, rounded once to `out_dtype`;
      one keyframe:  a1 (+ residual) in torch's promoted dtype, rounded once, then widened / rounded to `out_dtype`.
    kf_out [nb*K, S, D], residual [nb*C*n, S, D] or None, w fp32 [n] -> [nb*C*n, S, D] of out_dtype."""
    _, S, D = kf_out.shape
    C = len(slots)
    kf4 = kf_out.view(nb, -1, S, D)
    res5 = None if residual is None else residual.view(nb, C, n, S, D)
    outs = []
    for j, (ss, idx) in enumerate(zip(slots, want)):
        a1 = kf4[:, ss[0]][:, idx[0]].view(nb, n, S, D)
        if len(ss) == 2:
            a2 = kf4[:, ss[1]][:, idx[1]].view(nb, n, S, D)
            w1 = w.view(1, n, 1, 1)
            o = w1 * a1 + (1 - w1) * a2
            assert o.dtype == torch.float32
        else:
            o = a1
        if res5 is not None:
            o = o + res5[:, j]
        outs.append(o.to(out_dtype))
    return torch.stack(outs, dim=1).reshape(nb * C * n, S, D)
