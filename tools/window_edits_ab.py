#!/usr/bin/env python
"""A/B of the sliding-window keyframe bank for a multi-edit batch (`ops.ext_attn_windows_edits`) on one box, arms alternating
inside every round, one process per shape:
  (a)  E windowed single-edit calls (tf_ext_attn_fwd_windows on [source | uncond_e | cond_e], one per edit) -- what E prompts on
       a windowed clip cost without this call (--parent-lib PATH takes this arm from another build of the library, e.g. the
       parent commit's);
  (b)  ONE `ops.ext_attn_windows_edits` call, the DUAL composition (multi_v=False);
  (c)  the same call with the four-bank form forced (multi_v / multi_v64=True); only with injection on.
Shapes (every keyframe's queries, radius 2): the level-0 attention shapes of BASELINE configs 5, 4 and 2; E = 2 and 3, injection
on and off.  Per cell: median / min / max ms over the rounds and the run-to-run spread of each arm (interquartile range of its
rounds), b/a, c/b and whether (c) is ahead of (b) by more than the two arms' spreads.
    python tools/window_edits_ab.py [--rounds N] [--parent-lib PATH] [--shape cfg5|cfg4|cfg2] >> profiles/<name>.txt"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tokenflow_amd import _lib, ops  # noqa: E402
from tools.attn_microbench import flag  # noqa: E402

SHAPES = {"cfg5": (25, 4096, 5, 64), "cfg4": (10, 9216, 5, 64), "cfg2": (8, 4096, 8, 40)}      # level 0: K, S, H, Dh
RADIUS = 2


def foreign_windows(path):
    """`ext_attn_windows` (dense tensors) through tf_ext_attn_fwd_windows of ANOTHER build of the library."""
    lib = ctypes.CDLL(path)
    for name in ("tf_ext_attn_fwd_windows", "tf_ext_attn_workspace_bytes"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib._SIGNATURES[name]
    ws = {}

    def call(q, k, v, h, scale, inject, windows, out):
        K, S, D = k.shape[0] // 3, k.shape[1], k.shape[2]
        key = (K, S, h, D // h, _lib.TF_BF16)
        if key not in ws:
            ws[key] = torch.empty(lib.tf_ext_attn_workspace_bytes(*key), dtype=torch.uint8, device=q.device)
        lo, n = (ctypes.c_int * K)(*[w[0] for w in windows]), (ctypes.c_int * K)(*[w[1] for w in windows])
        fs = S * D
        strides = (ctypes.c_int64 * 9)(K * fs, fs, K * fs, fs, K * fs, fs, K * fs, fs, D)
        rc = lib.tf_ext_attn_fwd_windows(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), K, K, 0, S, h, D // h, D,
                                         ctypes.cast(strides, ctypes.c_void_p), float(scale), 1 if inject else 0, _lib.TF_BF16,
                                         ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p), ws[key].data_ptr(),
                                         ws[key].numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return out
    return lib.tf_abi_version(), call


def rounds_of(arms, rounds, warm=3):
    """Alternating rounds: every round times each arm once, in turn (device events).  {name: sorted ms}."""
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
    return {name: sorted(x) for name, x in t.items()}


def stats(x):
    n = len(x)
    return x[n // 2], x[0], x[-1], x[(3 * n) // 4] - x[n // 4]      # median, min, max, interquartile range


def main():
    rounds = flag("--rounds", 12)
    parent, only = None, None
    for name in ("--parent-lib", "--shape"):
        if name in sys.argv:
            i = sys.argv.index(name)
            parent, only = (sys.argv[i + 1], only) if name == "--parent-lib" else (parent, sys.argv[i + 1])
            del sys.argv[i:i + 2]
    dt = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    single, where = (lambda q1, k1, v1, h, sc, inj, w, out: ops.ext_attn_windows(q1, k1, v1, h, sc, inj, w, out=out)), "this build"
    if parent:
        abi, single = foreign_windows(parent)
        where = f"another build of the library (--parent-lib, ABI {abi})"
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, bf16, radius {RADIUS}, {rounds} alternating rounds per cell; "
          "median / min / max ms, spread = interquartile range of the arm's rounds")
    print(f"# (a) E windowed single-edit calls, tf_ext_attn_fwd_windows of {where}; (b) ONE ops.ext_attn_windows_edits, DUAL "
          "composition (multi_v=False); (c) the same call, four-bank form forced")
    print("# 'c ahead of b' = (b - c) of the medians exceeds the sum of the two arms' spreads")
    for cfg_name, (K, S, H, Dh) in SHAPES.items():
        if only and cfg_name != only:
            continue
        D, scale, windows = H * Dh, Dh ** -0.5, ops.bank_windows(K, RADIUS)
        hint = {"multi_v": True} if Dh == 40 else {"multi_v64": True}
        bank = sum(n for _, n in windows)
        print(f"\n{cfg_name} level 0: K={K} S={S} H={H} Dh={Dh}, windows hold {bank} of {K * K} frame-banks ({bank / (K * K):.2f})")
        for E in (2, 3):
            B = 1 + 2 * E
            q, k, v = (torch.randn(B * K, S, D, generator=g, device="cuda").to(dt) for _ in range(3))
            out = torch.empty_like(q)
            singles = [tuple(t.view(B, K, S, D)[[0, 1 + 2 * e, 2 + 2 * e]].reshape(3 * K, S, D).contiguous() for t in (q, k, v))
                       for e in range(E)]
            out1 = torch.empty_like(singles[0][0])
            for inject in (True, False):
                mask = (1 << E) - 1 if inject else 0

                def a_calls():
                    for q1, k1, v1 in singles:
                        single(q1, k1, v1, H, scale, inject, windows, out1)
                arms = {"a": a_calls,
                        "b": lambda: ops.ext_attn_windows_edits(q, k, v, H, scale, inject, E, windows, multi_v=False, out=out)}
                if inject:
                    arms["c"] = lambda: ops.ext_attn_windows_edits(q, k, v, H, scale, inject, E, windows, out=out, **hint)
                # every arm against arm (a) on the same inputs before anything is timed (different launches: close, not equal)
                ref = torch.empty_like(q).view(B, K, S, D)
                for e, (q1, k1, v1) in enumerate(singles):
                    o = single(q1, k1, v1, H, scale, inject, windows, torch.empty_like(q1)).view(3, K, S, D)
                    ref[0], ref[1 + 2 * e], ref[2 + 2 * e] = o[0], o[1], o[2]
                for name in list(arms)[1:]:
                    got = arms[name]().view(B, K, S, D)
                    assert torch.allclose(got.float(), ref.float(), atol=3e-2, rtol=3e-2), (cfg_name, E, inject, name)
                st = {name: stats(x) for name, x in rounds_of(arms, rounds).items()}
                plans = {"b": ops.attn_windows_edits_plan(K, windows, S, H, Dh, E, mask, multi_v=False)}
                if inject:
                    plans["c"] = ops.attn_windows_edits_plan(K, windows, S, H, Dh, E, mask, **hint)
                print(f"  E={E} inject={inject}")
                for name, label in (("a", f"{E} single-edit windowed calls"), ("b", "one call, DUAL composition"), ("c", "one call, four-bank form")):
                    if name not in st:
                        continue
                    med, lo, hi, iqr = st[name]
                    line = f"    ({name}) {label:30s} {med:8.3f} / {lo:8.3f} / {hi:8.3f} ms  spread {iqr:6.3f} ms ({100 * iqr / med:4.1f} %)"
                    if name == "b":
                        line += f"  b/a {med / st['a'][0]:.3f}"
                        line += "  b ahead of a" if st["a"][0] - med > iqr + st["a"][3] else "  b NOT ahead of a beyond the spread"
                    if name == "c":
                        line += f"  c/a {med / st['a'][0]:.3f}  c/b {med / st['b'][0]:.3f}"
                        line += "  c ahead of b" if st["b"][0] - med > iqr + st["b"][3] else "  c NOT ahead of b beyond the spread"
                    print(line + (f"  plan {plans[name]}" if name in plans else ""))
                sys.stdout.flush()
            del q, k, v, out, singles, out1
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
