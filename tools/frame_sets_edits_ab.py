#!/usr/bin/env python
"""A/B of the frame-set keyframe bank for a multi-edit batch (`ops.ext_attn_frame_sets_edits`) on one box, arms alternating
inside every round, one process per shape:
  (a)  E single-edit frame-set calls (tf_ext_attn_fwd_frame_sets on [source | uncond_e | cond_e], one per edit) -- what E prompts
       with anchor keyframes cost without this call (--parent-lib PATH takes this arm from another build of the library, e.g.
       the parent commit's);
  (b)  ONE `ops.ext_attn_frame_sets_edits` call, the DUAL composition (multi_v=False);
  (c)  the same call with the four-bank form forced (multi_v / multi_v64=True); only with injection on.
Shapes (every keyframe's queries, radius 2 with anchor keyframe 0): the level-0 attention shapes of BASELINE configs 5, 4 and 2;
E = 2 and 3, injection on and off.  Per cell: median / min / max ms over the rounds and the run-to-run spread of each arm
(interquartile range of its rounds), b/a, c/b and whether (c) is ahead of (b) by more than the two arms' spreads.
    python tools/frame_sets_edits_ab.py [--rounds N] [--parent-lib PATH] [--shape cfg5|cfg4|cfg2] >> profiles/<name>.txt"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tokenflow_amd import _lib, ops  # noqa: E402
from tools.attn_microbench import flag  # noqa: E402
from tools.window_edits_ab import SHAPES, rounds_of, stats  # noqa: E402

RADIUS, ANCHORS = 2, (0,)


def foreign_frame_sets(path):
    """`ext_attn_frame_sets` (dense tensors) through tf_ext_attn_fwd_frame_sets of ANOTHER build of the library."""
    lib = ctypes.CDLL(path)
    for name in ("tf_ext_attn_fwd_frame_sets", "tf_ext_attn_workspace_bytes"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib._SIGNATURES[name]
    ws = {}

    def call(q, k, v, h, scale, inject, sets, out):
        K, S, D = k.shape[0] // 3, k.shape[1], k.shape[2]
        key = (K, S, h, D // h, _lib.TF_BF16)
        if key not in ws:
            ws[key] = torch.empty(lib.tf_ext_attn_workspace_bytes(*key), dtype=torch.uint8, device=q.device)
        tab = (ctypes.c_uint64 * K)(*sets)
        fs = S * D
        strides = (ctypes.c_int64 * 9)(K * fs, fs, K * fs, fs, K * fs, fs, K * fs, fs, D)
        rc = lib.tf_ext_attn_fwd_frame_sets(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), K, K, 0, S, h, D // h, D,
                                            ctypes.cast(strides, ctypes.c_void_p), float(scale), 1 if inject else 0, _lib.TF_BF16,
                                            ctypes.cast(tab, ctypes.c_void_p), ws[key].data_ptr(), ws[key].numel(),
                                            torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return out
    return lib.tf_abi_version(), call


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
    single, where = (lambda q1, k1, v1, h, sc, inj, s, out: ops.ext_attn_frame_sets(q1, k1, v1, h, sc, inj, s, out=out)), "this build"
    if parent:
        abi, single = foreign_frame_sets(parent)
        where = f"another build of the library (--parent-lib, ABI {abi})"
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, bf16, radius {RADIUS} with anchors {list(ANCHORS)}, {rounds} "
          "alternating rounds per cell; median / min / max ms, spread = interquartile range of the arm's rounds")
    print(f"# (a) E single-edit frame-set calls, tf_ext_attn_fwd_frame_sets of {where}; (b) ONE ops.ext_attn_frame_sets_edits, DUAL "
          "composition (multi_v=False); (c) the same call, four-bank form forced")
    print("# 'c ahead of b' = (b - c) of the medians exceeds the sum of the two arms' spreads")
    for cfg_name, (K, S, H, Dh) in SHAPES.items():
        if only and cfg_name != only:
            continue
        D, scale, sets = H * Dh, Dh ** -0.5, ops.bank_frame_sets(K, RADIUS, ANCHORS)
        hint = {"multi_v": True} if Dh == 40 else {"multi_v64": True}
        bank = sum(bin(m).count("1") for m in sets)
        print(f"\n{cfg_name} level 0: K={K} S={S} H={H} Dh={Dh}, sets hold {bank} of {K * K} frame-banks ({bank / (K * K):.2f}), "
              f"largest set {max(bin(m).count('1') for m in sets)}")
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
                        single(q1, k1, v1, H, scale, inject, sets, out1)
                arms = {"a": a_calls,
                        "b": lambda: ops.ext_attn_frame_sets_edits(q, k, v, H, scale, inject, E, sets, multi_v=False, out=out)}
                if inject:
                    arms["c"] = lambda: ops.ext_attn_frame_sets_edits(q, k, v, H, scale, inject, E, sets, out=out, **hint)
                # every arm against arm (a) on the same inputs before anything is timed (different launches: close, not equal)
                ref = torch.empty_like(q).view(B, K, S, D)
                for e, (q1, k1, v1) in enumerate(singles):
                    o = single(q1, k1, v1, H, scale, inject, sets, torch.empty_like(q1)).view(3, K, S, D)
                    ref[0], ref[1 + 2 * e], ref[2 + 2 * e] = o[0], o[1], o[2]
                for name in list(arms)[1:]:
                    got = arms[name]().view(B, K, S, D)
                    assert torch.allclose(got.float(), ref.float(), atol=3e-2, rtol=3e-2), (cfg_name, E, inject, name)
                st = {name: stats(x) for name, x in rounds_of(arms, rounds).items()}
                plans = {"b": ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, E, mask, multi_v=False)}
                if inject:
                    plans["c"] = ops.attn_frame_sets_edits_plan(K, sets, S, H, Dh, E, mask, **hint)
                print(f"  E={E} inject={inject}")
                for name, label in (("a", f"{E} single-edit frame-set calls"), ("b", "one call, DUAL composition"), ("c", "one call, four-bank form")):
                    if name not in st:
                        continue
                    med, lo, hi, iqr = st[name]
                    line = f"    ({name}) {label:31s} {med:8.3f} / {lo:8.3f} / {hi:8.3f} ms  spread {iqr:6.3f} ms ({100 * iqr / med:4.1f} %)"
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
