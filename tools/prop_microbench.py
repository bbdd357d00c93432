#!/usr/bin/env python
"""Propagation of ALL chunks of one block: K calls of tf_nn_gather_blend (the reference's one chunk per UNet pass)
against ONE call of tf_nn_gather_blend_chunks, on BASELINE shapes.  TF_NN_MIN_WGS=<n> sets the grid target of the
multi-chunk search's pivot-range split.   python tools/prop_microbench.py [K,n,S,D ...]
--edits E: a multi-edit batch of E edits -- E single-edit `propagate_chunks` calls (one per prompt) against ONE
`propagate_chunks_edits` call, alternating, median / min over --rounds rounds.  A fourth arm times ONE single-edit call;
from it and the _edits call (search + 3 gathers, search + B gathers) the search's and a branch gather's time follow."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tokenflow_amd import ops  # noqa: E402
from attn_microbench import ab, flag, time_it  # noqa: E402


def edits_ab(shapes, E, rounds):
    g = torch.Generator(device="cuda").manual_seed(0)
    B = 1 + 2 * E
    ln = torch.nn.functional.layer_norm
    for K, n, S, D in shapes:
        piv = ln(torch.randn(K, S, D, generator=g, device="cuda"), (D,)).bfloat16()
        inv = ops.pivot_inv_norm(piv)
        kf = torch.randn(B * K, S, D, generator=g, device="cuda").bfloat16()
        tgt = ln(torch.randn(K * n * S, D, generator=g, device="cuda"), (D,)).bfloat16()
        res = torch.randn(B * K * n, S, D, generator=g, device="cuda").bfloat16()
        s = torch.arange(0, n)
        w = torch.sigmoid(torch.abs(s + n - n // 2) / (torch.abs(s - n // 2) + torch.abs(s + n - n // 2))).cuda()
        sl = lambda t, e: t.view(B, -1, S, D)[[0, 1 + 2 * e, 2 + 2 * e]].reshape(-1, S, D).contiguous()
        singles = [(sl(kf, e), sl(res, e)) for e in range(E)]

        def a_single():      # one pass per prompt: E searches, E three-branch gathers
            for kf1, res1 in singles:
                ops.propagate_chunks(tgt, piv, inv, kf1, w, n, K, 0, True, res1, torch.float32)

        def one_single():    # one prompt alone: 1 search + 1 three-branch gather
            ops.propagate_chunks(tgt, piv, inv, singles[0][0], w, n, K, 0, True, singles[0][1], torch.float32)
        arms = {"(a) E single-edit calls": a_single,
                "(b) one _edits call": lambda: ops.propagate_chunks_edits(tgt, piv, inv, kf, w, n, K, 0, True, res,
                                                                          torch.float32, E),
                "(b') the same again": lambda: ops.propagate_chunks_edits(tgt, piv, inv, kf, w, n, K, 0, True, res,
                                                                          torch.float32, E),
                "(s) ONE single-edit call": one_single}
        print(f"propagate_chunks_edits K={K} n={n} S={S} D={D} E={E}  ({rounds} alternating rounds)")
        print(f"  plan: {ops.propagate_edits_plan(n, K, S, D, True, E)}")
        r = ab(arms, rounds)
        for name, (med, mn, mx) in r.items():
            print(f"  {name:26s} median {med * 1e3:.1f} us  min {mn * 1e3:.1f} us  max {mx * 1e3:.1f} us", flush=True)
        # gather cost per branch g and search cost s from (s) = s + 3g and (b) = s + B g
        g_ = (r["(b) one _edits call"][0] - r["(s) ONE single-edit call"][0]) / (B - 3)
        print(f"  => per-branch gather ~{g_ * 1e3:.1f} us, search ~{(r['(s) ONE single-edit call'][0] - 3 * g_) * 1e3:.1f} us "
              f"(paid once in (b), {E} times in (a))", flush=True)


def main():
    shapes = [(8, 5, 4096, 320), (8, 5, 1024, 640), (8, 5, 256, 1280), (8, 5, 64, 1280), (4, 2, 1024, 320), (4, 2, 16, 1280)]
    E, rounds = flag("--edits", 0), flag("--rounds", 15)
    if len(sys.argv) > 1:
        shapes = [tuple(int(x) for x in a.split(",")) for a in sys.argv[1:]]
    if E:
        return edits_ab(shapes, E, rounds)
    g = torch.Generator(device="cuda").manual_seed(0)
    for K, n, S, D in shapes:
        ln = torch.nn.functional.layer_norm
        piv = ln(torch.randn(K, S, D, generator=g, device="cuda"), (D,)).bfloat16()
        inv = ops.pivot_inv_norm(piv)
        kf = torch.randn(3 * K, S, D, generator=g, device="cuda").bfloat16()
        tgt = ln(torch.randn(K * n * S, D, generator=g, device="cuda"), (D,)).bfloat16()
        res = torch.randn(3, K, n, S, D, generator=g, device="cuda").bfloat16()
        resc = [res[:, j].reshape(3 * n, S, D).contiguous() for j in range(K)]
        s = torch.arange(0, n)
        w = torch.sigmoid(torch.abs(s + n - n // 2) / (torch.abs(s - n // 2) + torch.abs(s + n - n // 2))).cuda()
        nS = n * S

        def per_chunk():
            for c in range(K):
                ids = [c] if c == 0 else [c, c - 1]
                ops.propagate(tgt[c * nS:(c + 1) * nS], piv, inv, ids, kf, w if c else None, n, resc[c],
                              torch.float32 if c else torch.bfloat16)

        def batched():
            ops.propagate_chunks(tgt, piv, inv, kf, w, n, K, 0, True, res.view(3 * K * n, S, D), torch.float32)
        fl = 2.0 * n * S * S * D * (2 * K - 1)
        for name, fn in (("per-chunk", per_chunk), ("one call ", batched)):
            avg, mn = time_it(fn, reps=20, warm=3)
            print(f"propagate K={K} n={n} S={S} D={D} {name}: avg {avg * 1e3:.1f} us  min {mn * 1e3:.1f} us  "
                  f"(NN part {fl / avg / 1e9:.0f} TF/s if it were all of it)", flush=True)


if __name__ == "__main__":
    main()
