#!/usr/bin/env python
"""A/B of the frame-set keyframe bank (`ops.ext_attn_frame_sets`: a sliding window plus global anchor keyframes) on one box,
arms alternating:
  (a)   the full-bank call -- what every pivotal pass costs without a window (--full-lib PATH takes this arm, and (b'), from
        another build of the library, e.g. the parent commit's);
  (b)   `ops.ext_attn_windows` at radius R from this build;
  (b')  the same windowed call through tf_ext_attn_fwd_windows of the --full-lib build: the windowed path is meant to be
        untouched, so (b) against (b') must lie within the spread;
  (c0)  `ops.ext_attn_frame_sets` at radius R with the anchor {0};
  (c8)  ... with every 8th keyframe as an anchor;
  (d0)  `ops.ext_attn_windows` on CONTIGUOUS windows of (c0)'s lengths, frame by frame: the same work in the same workgroup
        order without the set walk -- what separates the walk's cost from the effect of the longer, differently distributed
        key sequences;
  (a')  arm (a) again: the run-to-run spread.
Shapes: the level-0 and level-1 attention shapes of BASELINE configs 2, 4 and 5, each with the config's own injection state,
R = 1 and 2.  Per arm: median / min ms and TF/s on the work actually done (K + 2 * sum popcount frame-banks).  The judgement:
(c)'s TF/s against (b)'s at the same radius -- the set walk adds only scalar work per frame boundary, so a gap beyond the
spread of (a) against (a') is a finding.
    python tools/frame_sets_ab.py [--rounds N] [--full-lib PATH] > profiles/<name>.txt"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tokenflow_amd import _lib, ops, workload  # noqa: E402
from tools.attn_microbench import ab, flag, foreign_single_edit  # noqa: E402
from tools.window_ab import flops  # noqa: E402

RADII = (1, 2)


def foreign_windows(path):
    """`ext_attn_windows` (dense tensors, given output) through tf_ext_attn_fwd_windows of ANOTHER build of the library."""
    lib = ctypes.CDLL(path)
    for name in ("tf_ext_attn_fwd_windows", "tf_ext_attn_workspace_bytes"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib._SIGNATURES[name]
    ws = {}

    def ext_attn_windows(q, k, v, h, scale, inject, windows, out):
        K, S, D = k.shape[0] // 3, k.shape[1], k.shape[2]
        dtc = _lib.TF_BF16 if q.dtype == torch.bfloat16 else _lib.TF_F16
        key = (K, S, h, D // h, dtc)
        if key not in ws:
            ws[key] = torch.empty(lib.tf_ext_attn_workspace_bytes(*key), dtype=torch.uint8, device=q.device)
        lo, n = (ctypes.c_int * K)(*[w[0] for w in windows]), (ctypes.c_int * K)(*[w[1] for w in windows])
        fs = S * D
        strides = (ctypes.c_int64 * 9)(K * fs, fs, K * fs, fs, K * fs, fs, K * fs, fs, D)
        rc = lib.tf_ext_attn_fwd_windows(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), K, K, 0, S, h, D // h, D,
                                         ctypes.cast(strides, ctypes.c_void_p), float(scale), 1 if inject else 0, dtc,
                                         ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p), ws[key].data_ptr(),
                                         ws[key].numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return out
    return ext_attn_windows


def same_length_windows(K, sets):
    """Contiguous windows with the popcounts of `sets`, each holding its own frame."""
    return [(max(0, min(i - n // 2, K - n)), n) for i, n in enumerate(bin(m).count("1") for m in sets)]


def main():
    rounds = flag("--rounds", 15)
    full_lib = None
    if "--full-lib" in sys.argv:
        i = sys.argv.index("--full-lib")
        full_lib = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    dt = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    other = "another build of the library (--full-lib)" if full_lib else "this build"
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, bf16, {rounds} alternating rounds per shape (median / min ms)")
    print(f"# (a), (a') the full bank and (b') the windowed call: {other}; (b) ops.ext_attn_windows and (c0), (c8) "
          "ops.ext_attn_frame_sets (anchors {0} / every 8th keyframe): this build")
    print("# all arms alternate inside every round, one box, one process.  TF/s: source branch + bank work actually done "
          "(K + 2 * sum popcount frame-banks)")
    for cfg_name in ("cfg2", "cfg4", "cfg5"):
        cfg = workload.CONFIGS[cfg_name]
        K = cfg.K
        for lvl in (0, 1):
            S, D, H = cfg.levels[lvl]
            inject = cfg.pnp
            q, k, v = (torch.randn(3 * K, S, D, generator=g, device="cuda").to(dt) for _ in range(3))
            out = torch.empty_like(q)
            scale = (D // H) ** -0.5
            full = (lambda: ops.ext_attn(q, k, v, H, scale, inject, out=out))
            win_other = (lambda w: ops.ext_attn_windows(q, k, v, H, scale, inject, w, out=out))
            if full_lib:
                _abi, foreign = foreign_single_edit(full_lib)
                full = (lambda: foreign(q, k, v, H, scale, inject, out))
                fwin = foreign_windows(full_lib)
                win_other = (lambda w: fwin(q, k, v, H, scale, inject, w, out))
            arms = {"a": full}
            tables = {}
            for R in RADII:
                if R >= K - 1:
                    continue
                win = ops.bank_windows(K, R)
                sets = {"c0": ops.bank_frame_sets(K, R, [0]), "c8": ops.bank_frame_sets(K, R, range(0, K, 8))}
                tables[R] = (win, sets)
                # the windowed call of the two builds on the same inputs, before anything is timed
                assert torch.equal(win_other(win).clone(), ops.ext_attn_windows(q, k, v, H, scale, inject, win))
                arms[f"b{R}"] = (lambda w=win: ops.ext_attn_windows(q, k, v, H, scale, inject, w, out=out))
                arms[f"b'{R}"] = (lambda w=win: win_other(w))
                for name, s in sets.items():
                    arms[f"{name}_{R}"] = (lambda s=s: ops.ext_attn_frame_sets(q, k, v, H, scale, inject, s, out=out))
                arms[f"d0_{R}"] = (lambda w=same_length_windows(K, sets["c0"]): ops.ext_attn_windows(q, k, v, H, scale, inject, w, out=out))
            arms["a'"] = full
            t = ab(arms, rounds=rounds)
            a_med = t["a"][0]
            a_tf = flops(S, D, K, K * K) / a_med * 1e-9
            spread = abs(t["a'"][0] - a_med) / a_med
            print(f"\n{cfg_name} level {lvl}: K={K} S={S} H={H} Dh={D // H} inject={inject}")
            print(f"  (a)  full bank             {a_med:8.3f} / {t['a'][1]:8.3f} ms  {a_tf:7.1f} TF/s   plan {ops.attn_plan(K, K, S, H, D // H, inject)}")
            print(f"  (a') full bank again       {t[chr(97) + chr(39)][0]:8.3f} / {t[chr(97) + chr(39)][1]:8.3f} ms  spread of the medians {100 * spread:.2f} %")
            for R, (win, sets) in tables.items():
                bank = sum(n for _, n in win)
                b_med, bp_med = t[f"b{R}"][0], t[f"b'{R}"][0]
                b_tf = flops(S, D, K, bank) / b_med * 1e-9
                print(f"  (b)  windows R={R}           {b_med:8.3f} / {t[f'b{R}'][1]:8.3f} ms  {b_tf:7.1f} TF/s   {bank} frame-banks, b/a {b_med / a_med:.3f}"
                      f"   plan {ops.attn_windows_plan(K, win, S, H, D // H, inject)}")
                print(f"  (b') windows R={R}, other    {bp_med:8.3f} / {t[chr(98) + chr(39) + str(R)][1]:8.3f} ms  b/b' {b_med / bp_med:.4f}")
                for name, s in sets.items():
                    n_banks = sum(bin(m).count("1") for m in s)
                    c_med = t[f"{name}_{R}"][0]
                    c_tf = flops(S, D, K, n_banks) / c_med * 1e-9
                    anchors = "{0}" if name == "c0" else "{0,8,..}"
                    print(f"  ({name}) sets R={R} + {anchors:9s} {c_med:8.3f} / {t[f'{name}_{R}'][1]:8.3f} ms  {c_tf:7.1f} TF/s   {n_banks} frame-banks, "
                          f"c/a {c_med / a_med:.3f}, {c_tf / b_tf:.3f} of (b)'s TF/s   plan {ops.attn_frame_sets_plan(K, s, S, H, D // H, inject)}")
                d_med = t[f"d0_{R}"][0]
                print(f"  (d0) windows of (c0)'s lengths {d_med:6.3f} / {t[f'd0_{R}'][1]:8.3f} ms  c0/d0 {t[f'c0_{R}'][0] / d_med:.4f}")


if __name__ == "__main__":
    main()
