"""Cases and the CPU reference of the ragged chunk runs (`ops.propagate_chunks_ragged`: chunk j of a run has its own frame
count n_j).

The reference is the one-chunk reference, chunk by chunk: `nn_exact.propagation_reference` on chunk j's tensors alone with
n = n_j and the blend weights of n_j, concatenated along the frames.  The search inputs are the exact families of
tests/nn_exact.py: ONE `Inputs` per distinct n_j, all with the same seed, so they share their pivots (the pivots are drawn
before anything that depends on the target count) and chunk j takes its targets from the `Inputs` of its own n_j.

`frame_plan` / `reference_by_frame` spell the same computation frame by frame (a chunk of one frame per call: the gather
arithmetic is elementwise, so this is the per-chunk reference bit for bit) -- the form in which the MUTANTS of
tests/test_ragged_cpu.py are written: each of them breaks one thing a ragged kernel can get wrong, and the inputs of the GPU
tests must tell every one of them from the reference.
"""
import torch

from oracle import tokenflow_oracle as orc
from tests import nn_exact as nx

# (S, D, kernel form of every search involved, frame lists): tests/test_ragged_gpu.py asserts the form through the plan entry
# points.  Frame counts of the last three shapes stay in {2, 3}: a one-frame chunk alone leaves the form there.
SMALL = [(45, 320, "rb"), (96, 320, "rbs<TJ=2>"), (45, 72, "bk64"), (45, 640, "bk128"), (45, 1280, "deep")]
LARGE = [(11808, 320, "rbs<TJ=4>"), (2180, 640, "glds"), (4040, 72, "wide")]
SMALL_FRAMES = [[3, 1, 2, 5], [1, 1, 1], [2, 5, 1, 3, 2]]
LARGE_FRAMES = [[2, 3, 2], [3, 2, 3, 2]]
# targets per panel of a form (nn_search.hip: `tn` of the form descriptions)
PANEL = {"rb": 128, "rbs<TJ=2>": 128, "rbs<TJ=4>": 256, "glds": 256, "wide": 128, "bk64": 64, "bk128": 64, "deep": 64}


def masks(C):
    """(single_mask, slot0): a one-keyframe chunk at the front, one in the middle (and the front), none at all (slot0 = 1)."""
    out = [(1, 0), (0, 1)]
    if C > 2:
        out.insert(1, (1 | (1 << (C // 2)), 0))
    return out


def slots_of(C, slot0, mask):
    return [[slot0 + j] if (mask >> j) & 1 else [slot0 + j, slot0 + j - 1] for j in range(C)]


def weights(frames):
    """The `w` of a ragged call: the blend weights of every chunk's own size, concatenated -- one float per frame of the run."""
    return torch.cat([orc.blend_weights(n, 1) for n in frames])


def starts(frames):
    out = [0]
    for n in frames:
        out.append(out[-1] + n)
    return out


class Ragged:
    """The search inputs of one (frames, S, D, family): K = C + 1 keyframe slots, chunk j may search slots slot0 + j and
    slot0 + j - 1 for slot0 in {0, 1}.  want[(j, s)]: the exact first-index answer of chunk j's targets in slot s."""

    def __init__(self, frames, S, D, family, seed=None, device="cpu"):
        self.frames, self.S, self.D, self.family = list(frames), S, D, family
        C = self.C = len(frames)
        self.K = C + 1
        seed = S * 7 + D if seed is None else seed
        # chunk j of every Inputs aims at slot j first (pool: at both of j, j + 1; roll-call: at slot j)
        layout = [[j, j + 1] for j in range(C)]
        self.inputs = {n: nx.Inputs(self.K, S, D, n * S, layout, family, seed) for n in sorted(set(frames))}
        first = self.inputs[self.frames[0]]
        assert all(torch.equal(i.piv, first.piv) and torch.equal(i.exps, first.exps) for i in self.inputs.values()), \
            "the Inputs of different frame counts do not share their pivots"
        self.piv8, self.exps = first.piv, first.exps
        self.tgt8 = [self.inputs[n].targets(j, device) for j, n in enumerate(frames)]
        pv = self.piv8.to(device)
        self.want = {(j, s): nx.first_argmax(self.tgt8[j], pv[s]).cpu() for j in range(C) for s in (j - 1, j, j + 1)
                     if 0 <= s < self.K}

    def pivots(self, device, dtype, scaled):
        return self.inputs[self.frames[0]].pivots(device, dtype, scaled)

    def targets(self, device, dtype):
        return torch.cat([t.to(device) for t in self.tgt8]).to(dtype)

    def indices(self, slot0, mask):
        return [[self.want[(j, s)] for s in ss] for j, ss in enumerate(slots_of(self.C, slot0, mask))]


def reference(kf_out, frames, slot0, mask, want, residual, out_dtype, nb):
    """Per-chunk `nn_exact.propagation_reference`, concatenated: kf_out [nb*K, S, D], residual [nb*F, S, D] or None,
    want[j] = the index tensors of chunk j's slots -> [nb*F, S, D]."""
    _, S, D = kf_out.shape
    F, st = sum(frames), starts(frames)
    res4 = None if residual is None else residual.view(nb, F, S, D)
    outs = []
    for j, (n, ss) in enumerate(zip(frames, slots_of(len(frames), slot0, mask))):
        res = None if res4 is None else res4[:, st[j]:st[j + 1]].reshape(nb * n, S, D)
        o = nx.propagation_reference(kf_out, [ss], [want[j]], orc.blend_weights(n, 1), res, out_dtype, nb, n)
        outs.append(o.view(nb, n, S, D))
    return torch.cat(outs, dim=1).reshape(nb * F, S, D)


# ------------------------------------------------------------------------------------------------ frame by frame, mutants
MUTANTS = ("w_of_n_max", "w_index_mod_uniform", "chunk_by_mean_division", "prefix_off_by_one_frame", "neighbour_slot",
           "single_rounding_on_wrong_chunk")


def frame_plan(frames, slot0, mask, want, S, mutant=None):
    """One entry per frame of the run: dict(slots, idx, w, single_round).  `idx` are the frame's rows of the indices the
    SEARCH found for its true chunk; everything else is what the GATHER decodes, which is where the mutants lie."""
    assert mutant is None or mutant in MUTANTS
    C, F, st = len(frames), sum(frames), starts(frames)
    w_all = weights(frames)
    n_max = max(frames)
    mean = -(-F // C)
    plan = []
    for f in range(F):
        j = max(c for c in range(C) if st[c] <= f)
        i = f - st[j]
        jg = j                                            # the chunk the gather takes the frame for
        if mutant == "chunk_by_mean_division":
            jg = min(f // mean, C - 1)
        elif mutant == "prefix_off_by_one_frame":
            jg = max(c for c in range(C) if st[c] + (1 if c else 0) <= f)
        single = bool((mask >> jg) & 1)
        ss = [slot0 + jg] if single else [slot0 + jg, slot0 + jg - 1]
        if mutant == "neighbour_slot" and not single:
            ss = [slot0 + jg, slot0 + jg + 1] if jg + 1 < C else [slot0 + jg - 1, slot0 + jg]
        idx = [t[i * S:(i + 1) * S] for t in want[j]]
        idx = (idx + idx)[:len(ss)]                       # a gather that takes the frame for another kind of chunk
        w = w_all[f]
        if mutant == "w_of_n_max":
            w = orc.blend_weights(n_max, 1)[i]
        elif mutant == "w_index_mod_uniform":
            w = orc.blend_weights(n_max, 1)[f % n_max]
        rounds = single
        if mutant == "single_rounding_on_wrong_chunk":
            rounds = bool((mask >> ((jg + C - 1) % C)) & 1)
        plan.append(dict(slots=ss, idx=idx, w=w.reshape(1), single=single, rounds=rounds))
    return plan


def reference_by_frame(kf_out, plan, residual, out_dtype, nb):
    """`reference` spelled frame by frame over a `frame_plan`."""
    _, S, D = kf_out.shape
    F = len(plan)
    res4 = None if residual is None else residual.view(nb, F, S, D)
    outs = []
    for f, p in enumerate(plan):
        res = None if res4 is None else res4[:, f].reshape(nb, S, D)
        if p["single"] == p["rounds"]:
            o = nx.propagation_reference(kf_out, [p["slots"]], [p["idx"]], p["w"], res, out_dtype, nb, 1)
        elif p["single"]:      # a one-keyframe frame that is NOT rounded to the dtype its own pass produces
            o = nx.propagation_reference(kf_out.float(), [p["slots"]], [p["idx"]], p["w"],
                                         None if res is None else res.float(), torch.float32, nb, 1).to(out_dtype)
        else:                  # a two-keyframe frame that IS
            sd = kf_out.dtype if res is None else torch.promote_types(kf_out.dtype, res.dtype)
            o = nx.propagation_reference(kf_out, [p["slots"]], [p["idx"]], p["w"], res, torch.float32, nb, 1).to(sd).to(out_dtype)
        outs.append(o.view(nb, 1, S, D))
    return torch.cat(outs, dim=1).reshape(nb * F, S, D)


# -------------------------------------------------------------------------------------------------- mutants of the search
def unsearched_tail(want, frames, S, panel):
    """The indices a search leaves when the partial last panel of every chunk is never computed: zeros in the last
    n_j * S mod panel rows of chunk j (nothing changes where the chunk fills its panels)."""
    out = []
    for j, n in enumerate(frames):
        tail = (n * S) % panel
        ws = [t.clone() for t in want[j]]
        for t in ws:
            if tail:
                t[-tail:] = 0
        out.append(ws)
    return out


def next_slot_inv_norm(rg, slot0, mask):
    """The indices a search finds that scales the scores of slot s with the inverse norms of slot s + 1 (cyclically): with the
    SCALED pivots score = dot * 2^(e[s, r] - e[s + 1, r]); with the unscaled ones nothing changes."""
    out = []
    e = rg.exps.double()
    for j, ss in enumerate(slots_of(rg.C, slot0, mask)):
        ws = []
        for s in ss:
            sim = rg.tgt8[j].double() @ rg.piv8[s].double().T * torch.exp2(e[s] - e[(s + 1) % rg.K])
            ws.append(nx.first_of_max(sim)[0])
        out.append(ws)
    return out
