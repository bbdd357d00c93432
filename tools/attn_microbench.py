#!/usr/bin/env python
"""Time tf_ext_attn_fwd (and optionally tf_nn_search) on BASELINE shapes, one process per library
build so that kernel variants can be A/B-ed:  TOKENFLOW_HIP_LIB=<.so> python tools/attn_microbench.py
Prints avg/min ms over `reps` launches (HIP events on the launch stream) and TFLOP/s (algorithmic).
--edits E: a multi-edit batch of E edits under q/k injection, alternating A/B of three arms per shape -- (a) E full
single-edit `ext_attn` calls (one per prompt), (b) `ext_attn_edits`, the composition, (c) `ext_attn_edits` with the
four-bank form on (head dim 40: multi_v=True; head dim 64: multi_v64=True) -- median / min over --rounds rounds, plus the
spread of arm (b) against itself; the largest absolute difference between the results of (c) and (b) is printed first.
--edits E --inject-mask M: the edits differ in their injection state (bit e of M = edit e injects) -- (a) E single-edit
`ext_attn` calls, each with its own flag, (b) ONE masked call `ext_attn_edits(..., inject_mask=M)` with the library's
default rule, (b') the same again (the spread), (c) the masked call as a pure composition (multi_v=False).
--single-lib PATH takes arm (a) from another build of the library (tf_ext_attn_fwd of that .so, e.g. the parent commit's).
--edits E --inject-mask M --runs W,R [--no-split]: ONE run set of a multi-edit batch as rank R of W frame-sharded ranks issues
it (`ext_attn_runs_edits`: the rank's own keyframes hold the queries, then the frames left and right of them; remote runs read
a compact k) -- (a) the DUAL composition, (a') the same again (the spread), (b) multi_v=True, the four-bank run launches for
pairs of injecting edits.  --no-split: one-pass runs, the shards' default."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tokenflow_amd import ops, workload  # noqa: E402


def time_it(fn, reps=8, warm=2):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) for a, b in ev]
    return sum(t) / len(t), min(t)


def ab(arms, rounds=15, warm=3):
    """Alternating A/B: every round times each arm once, in turn (device events).  {name: (median, min, max)} in ms."""
    for _ in range(warm):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t[name].append(a.elapsed_time(b))
    return {name: (sorted(x)[len(x) // 2], min(x), max(x)) for name, x in t.items()}


def flag(name, default):
    """--name VALUE out of sys.argv (removed from it)."""
    if name in sys.argv:
        i = sys.argv.index(name)
        val = int(sys.argv[i + 1], 0)      # 5, 0b101, 0x5
        del sys.argv[i:i + 2]
        return val
    return default


def foreign_single_edit(path):
    """`ext_attn` (dense tensors, fresh output) through tf_ext_attn_fwd of ANOTHER build of the library."""
    from tokenflow_amd import _lib
    lib = ctypes.CDLL(path)
    for name in ("tf_ext_attn_fwd", "tf_ext_attn_workspace_bytes"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib._SIGNATURES[name]
    ws = {}

    def ext_attn(q, k, v, h, scale, inject, out):
        K, S, D = k.shape[0] // 3, k.shape[1], k.shape[2]
        dtc = _lib.TF_BF16 if q.dtype == torch.bfloat16 else _lib.TF_F16
        key = (K, S, h, D // h, dtc)
        if key not in ws:
            ws[key] = torch.empty(lib.tf_ext_attn_workspace_bytes(*key), dtype=torch.uint8, device=q.device)
        rc = lib.tf_ext_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), K, K, 0, S, h, D // h, D,
                                 float(scale), 1 if inject else 0, dtc, ws[key].data_ptr(), ws[key].numel(),
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return out
    return lib.tf_abi_version(), ext_attn


def edits_masked_ab(shapes, E, mask, dt, rounds, single_lib):
    g = torch.Generator(device="cuda").manual_seed(0)
    B = 1 + 2 * E
    single, where = (lambda q1, k1, v1, h, sc, inj, out: ops.ext_attn(q1, k1, v1, h, sc, inj, out=out)), "this build"
    if single_lib:
        abi, single = foreign_single_edit(single_lib)
        where = f"{single_lib} (ABI {abi})"
    for K, S, h, d in shapes:
        D = h * d
        q, k, v = (torch.randn(B * K, S, D, generator=g, device="cuda").to(dt) for _ in range(3))
        out = torch.empty_like(q)
        singles = []
        for e in range(E):      # what a user with differing schedules does without the mask: one full pass per edit
            sel = [0, 1 + 2 * e, 2 + 2 * e]
            singles.append(tuple(t.view(B, K, S, D)[sel].reshape(3 * K, S, D).contiguous() for t in (q, k, v)))
        out1 = torch.empty_like(singles[0][0])

        def a_single():
            for e, (q1, k1, v1) in enumerate(singles):
                single(q1, k1, v1, h, d ** -0.5, bool((mask >> e) & 1), out1)
        # the foreign build against this one on the same inputs, before anything is timed
        for e, (q1, k1, v1) in enumerate(singles):
            inj = bool((mask >> e) & 1)
            assert torch.equal(single(q1, k1, v1, h, d ** -0.5, inj, torch.empty_like(q1)), ops.ext_attn(q1, k1, v1, h, d ** -0.5, inj))

        def masked(mv):
            return lambda: ops.ext_attn_edits(q, k, v, h, d ** -0.5, False, E, out=out, multi_v=mv, inject_mask=mask)
        arms = {"(a) E single-edit calls": a_single, "(b) one masked call": masked(None), "(b') masked call again": masked(None),
                "(c) masked, composition": masked(False)}
        print(f"ext_attn_edits {str(dt)[6:]} K={K} S={S} h={h} d={d} E={E} inject_mask={mask:#b}  ({rounds} alternating rounds; "
              f"arm (a): {where})")
        print(f"  plan (b): {ops.attn_edits_plan(K, K, S, h, d, False, E, dtype=dt, inject_mask=mask)}")
        print(f"  plan (c): {ops.attn_edits_plan(K, K, S, h, d, False, E, dtype=dt, multi_v=False, inject_mask=mask)}")
        for name, (med, mn, mx) in ab(arms, rounds).items():
            print(f"  {name:26s} median {med:.3f} ms  min {mn:.3f} ms  max {mx:.3f} ms", flush=True)


def runs_ab(shapes, E, mask, W, R, dt, rounds, no_split):
    g = torch.Generator(device="cuda").manual_seed(0)
    B = 1 + 2 * E
    for K, S, h, d in shapes:
        D = h * d
        counts = [K // W + (1 if r < K % W else 0) for r in range(W)]
        f0, Kl = sum(counts[:R]), counts[R]
        runs = [(f0, Kl)] + ([(0, f0)] if f0 else []) + ([(f0 + Kl, K - f0 - Kl)] if f0 + Kl < K else [])
        q, k, v = (torch.randn(B * K, S, D, generator=g, device="cuda").to(dt) for _ in range(3))
        ql = q.view(B, K, S, D)[:, f0:f0 + Kl].reshape(B * Kl, S, D).contiguous()
        out = torch.empty_like(ql)

        def run_set(mv):
            return lambda: ops.ext_attn_runs_edits(ql, k, v, h, d ** -0.5, E, mask, runs, q_frame0=f0, out=out, no_split=no_split,
                                                   k_compact=True, multi_v=mv)
        print(f"ext_attn_runs_edits {str(dt)[6:]} K={K} S={S} h={h} d={d} E={E} inject_mask={mask:#b} rank {R} of {W}: runs {runs} "
              f"no_split={int(no_split)}  ({rounds} alternating rounds)")
        for mv in (False, True):
            for r, (_, n) in enumerate(runs):
                plan = ops.attn_run_edits_plan(K, Kl, n, len(runs), S, h, d, E, mask, dtype=dt, bank_only=r != 0, no_split=no_split,
                                               multi_v=mv)
                print(f"  plan multi_v={int(mv)} run {r} ({n} frames): {plan}")
        res_a, res_b = run_set(False)().float(), run_set(True)().float()
        print(f"  max |(b) - (a)| = {float((res_b - res_a).abs().max()):.3e}  (max |(a)| = {float(res_a.abs().max()):.3e})")
        del res_a, res_b
        arms = {"(a) DUAL composition": run_set(False), "(a') composition again": run_set(False),
                "(b) four-bank run launches": run_set(True)}
        for name, (med, mn, mx) in ab(arms, rounds).items():
            print(f"  {name:26s} median {med:.3f} ms  min {mn:.3f} ms  max {mx:.3f} ms", flush=True)


def edits_ab(shapes, E, dt, rounds, single_lib=None):
    g = torch.Generator(device="cuda").manual_seed(0)
    B = 1 + 2 * E
    single, where = (lambda q1, k1, v1, h, sc, inj, out: ops.ext_attn(q1, k1, v1, h, sc, inj, out=out)), "this build"
    if single_lib:
        abi, single = foreign_single_edit(single_lib)
        where = f"{single_lib} (ABI {abi})"
    for K, S, h, d in shapes:
        D = h * d
        q, k, v = (torch.randn(B * K, S, D, generator=g, device="cuda").to(dt) for _ in range(3))
        out = torch.empty_like(q)
        singles = []
        for e in range(E):      # what a user does today: one full pass per prompt over [source | uncond_e | cond_e]
            sel = [0, 1 + 2 * e, 2 + 2 * e]
            singles.append(tuple(t.view(B, K, S, D)[sel].reshape(3 * K, S, D).contiguous() for t in (q, k, v)))
        out1 = torch.empty_like(singles[0][0])

        def a_single():
            for q1, k1, v1 in singles:
                single(q1, k1, v1, h, d ** -0.5, True, out1)
        on = dict(multi_v64=True) if d == 64 else dict(multi_v=True)   # the hint of the four-bank form at this head dim
        arms = {"(a) E single-edit calls": a_single,
                "(b) composition": lambda: ops.ext_attn_edits(q, k, v, h, d ** -0.5, True, E, out=out, multi_v=False),
                "(b') composition again": lambda: ops.ext_attn_edits(q, k, v, h, d ** -0.5, True, E, out=out, multi_v=False)}
        plan_c = ops.attn_edits_plan(K, K, S, h, d, True, E, dtype=dt, **on)
        if any("MV4" in t for t in plan_c):
            arms["(c) four-bank form"] = lambda: ops.ext_attn_edits(q, k, v, h, d ** -0.5, True, E, out=out, **on)
        print(f"ext_attn_edits {str(dt)[6:]} K={K} S={S} h={h} d={d} inject=1 E={E}  ({rounds} alternating rounds; "
              f"arm (a): {where})")
        print(f"  plan (b): {ops.attn_edits_plan(K, K, S, h, d, True, E, dtype=dt, multi_v=False)}")
        print(f"  plan (c): {plan_c}")
        if "(c) four-bank form" in arms:   # the two forms on the same inputs, before anything is timed
            res_b = ops.ext_attn_edits(q, k, v, h, d ** -0.5, True, E, multi_v=False).float()
            res_c = ops.ext_attn_edits(q, k, v, h, d ** -0.5, True, E, **on).float()
            print(f"  max |(c) - (b)| = {float((res_c - res_b).abs().max()):.3e}  (max |(b)| = {float(res_b.abs().max()):.3e})")
            del res_b, res_c
        for name, (med, mn, mx) in ab(arms, rounds).items():
            print(f"  {name:26s} median {med:.3f} ms  min {mn:.3f} ms  max {mx:.3f} ms", flush=True)


def main():
    shapes = [(8, 4096, 8, 40), (8, 1024, 8, 80), (8, 256, 8, 160), (10, 9216, 5, 64)]
    E, rounds, mask = flag("--edits", 0), flag("--rounds", 15), flag("--inject-mask", None)
    single_lib = None
    if "--single-lib" in sys.argv:
        i = sys.argv.index("--single-lib")
        single_lib = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    runs_of = None
    if "--runs" in sys.argv:
        i = sys.argv.index("--runs")
        runs_of = tuple(int(x) for x in sys.argv[i + 1].split(","))
        del sys.argv[i:i + 2]
    no_split = "--no-split" in sys.argv
    if no_split:
        sys.argv.remove("--no-split")
    args = [a for a in sys.argv[1:] if a not in ("f16", "bf16")]
    dt = torch.float16 if "f16" in sys.argv[1:] else torch.bfloat16
    if args:
        shapes = [tuple(int(x) for x in a.split(",")) for a in args]
    if E and runs_of:
        return runs_ab(shapes, E, (1 << E) - 1 if mask is None else mask, runs_of[0], runs_of[1], dt, rounds, no_split)
    if E and mask is not None:
        return edits_masked_ab(shapes, E, mask, dt, rounds, single_lib)
    if E:
        return edits_ab(shapes, E, dt, rounds, single_lib)
    g = torch.Generator(device="cuda").manual_seed(0)
    for K, S, h, d in shapes:
        D = h * d
        q, k, v = (torch.randn(3 * K, S, D, generator=g, device="cuda").to(dt) for _ in range(3))
        fl = workload.attn_flops(K, S, D)
        for inj in (False, True):
            avg, mn = time_it(lambda: ops.ext_attn(q, k, v, h, d ** -0.5, inj), reps=6 if S > 4096 else 10)
            print(f"ext_attn {str(dt)[6:]} K={K} S={S} h={h} d={d} inject={int(inj)}: avg {avg:.3f} ms  min {mn:.3f} ms  "
                  f"{fl / avg / 1e9:.0f} TF/s", flush=True)


if __name__ == "__main__":
    main()
