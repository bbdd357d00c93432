#!/usr/bin/env python
"""A/B of the sliding-window keyframe bank (`ops.ext_attn_windows`) on one box, arms alternating:
  (a)  the full-bank `ops.ext_attn` -- what every pivotal pass costs today
       (--full-lib PATH takes this arm from another build of the library, e.g. the parent commit's);
  (b)  the windowed call at radius 1, 2 and 4: ONE launch for all keyframes;
  (c)  the K own calls it replaces (`ops.ext_attn` per keyframe on its window's tensors, Kq = 1), at each radius;
  (a') arm (a) again: the run-to-run spread.
Shapes: the level-0 and level-1 attention shapes of BASELINE configs 2, 4 and 5, each with the config's own injection state.
Per shape and radius: median / min ms, the flop ratio sum_i win_n[i] / K^2 of the bank work, (b)'s time against (a)'s, and the
fraction of (a)'s TF/s the windowed launch achieves on its (smaller) work.
    python tools/window_ab.py [--rounds N] [--full-lib PATH] > profiles/<name>.txt"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tokenflow_amd import ops, workload  # noqa: E402
from tools.attn_microbench import ab, flag, foreign_single_edit  # noqa: E402

RADII = (1, 2, 4)


def flops(S, D, K, bank_frames):
    """QK^T and P.V at 2 flop/MAC: the source branch of K frames on their own S keys, uncond and cond on `bank_frames` frame-banks
    in all (K * K for the full bank, sum_i win_n[i] for windows)."""
    return 4.0 * S * D * S * (K + 2.0 * bank_frames)


def main():
    rounds = flag("--rounds", 15)
    full_lib = None
    if "--full-lib" in sys.argv:
        i = sys.argv.index("--full-lib")
        full_lib = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    dt = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, bf16, {rounds} alternating rounds per shape (median / min ms)")
    print(f"# arm (a): {'tf_ext_attn_fwd of another build of the library (--full-lib)' if full_lib else 'ops.ext_attn of this build'}; "
          "(b) ops.ext_attn_windows, ONE launch; (c) the K own calls (Kq = 1) it replaces; (a') arm (a) again = the run-to-run spread")
    print("# all arms alternate inside every round, one box, one process.  TF/s: source branch + bank work actually done "
          "(K + 2 * sum win_n frame-banks); 'bank flop ratio' = sum win_n / K^2")
    print("# workgroups keep frame order: no reordering arm (long windows first) is built or measured")
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
            if full_lib:
                _abi, foreign = foreign_single_edit(full_lib)
                full = (lambda: foreign(q, k, v, H, scale, inject, out))
            arms = {"a": full}
            tables = {}
            for R in RADII:
                if R >= K - 1:
                    continue
                win = tables[R] = ops.bank_windows(K, R)
                arms[f"b{R}"] = (lambda w=win: ops.ext_attn_windows(q, k, v, H, scale, inject, w, out=out))
                own = []
                for i, (lo, n) in enumerate(win):
                    sl = lambda t, a, b: t.view(3, K, S, D)[:, a:b].reshape(3 * (b - a), S, D).contiguous()      # noqa: E731
                    own.append((sl(q, i, i + 1), sl(k, lo, lo + n), sl(v, lo, lo + n), i - lo, torch.empty(3, S, D, dtype=dt, device="cuda")))

                def own_calls(own=own):
                    for q1, k1, v1, f0, o1 in own:
                        ops.ext_attn(q1, k1, v1, H, scale, inject, out=o1, q_frame0=f0)
                arms[f"c{R}"] = own_calls
            arms["a'"] = full
            t = ab(arms, rounds=rounds)
            a_med = t["a"][0]
            a_tf = flops(S, D, K, K * K) / a_med * 1e-9
            spread = abs(t["a'"][0] - a_med) / a_med
            print(f"\n{cfg_name} level {lvl}: K={K} S={S} H={H} Dh={D // H} inject={inject}")
            print(f"  (a)  full bank           {a_med:8.3f} / {t['a'][1]:8.3f} ms  {a_tf:7.1f} TF/s   plan {ops.attn_plan(K, K, S, H, D // H, inject)}")
            print(f"  (a') full bank again     {t[chr(97) + chr(39)][0]:8.3f} / {t[chr(97) + chr(39)][1]:8.3f} ms  spread of the medians {100 * spread:.2f} %")
            for R, win in tables.items():
                bank = sum(n for _, n in win)
                b_med, c_med = t[f"b{R}"][0], t[f"c{R}"][0]
                b_tf = flops(S, D, K, bank) / b_med * 1e-9
                print(f"  (b)  windows R={R}         {b_med:8.3f} / {t[f'b{R}'][1]:8.3f} ms  {b_tf:7.1f} TF/s   bank flop ratio {bank}/{K * K} = "
                      f"{bank / (K * K):.3f}, time ratio b/a {b_med / a_med:.3f}, {b_tf / a_tf:.2f} of (a)'s TF/s   plan "
                      f"{ops.attn_windows_plan(K, win, S, H, D // H, inject)}")
                print(f"  (c)  {K} own calls R={R}     {c_med:8.3f} / {t[f'c{R}'][1]:8.3f} ms  c/b {c_med / b_med:.3f}")


if __name__ == "__main__":
    main()
