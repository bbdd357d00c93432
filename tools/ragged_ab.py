#!/usr/bin/env python
"""A/B of the ragged chunk runs at BASELINE block shapes, alternating on one box:
  (a) one `tf_nn_gather_blend` per chunk -- what a user with chunks of unequal length has without the ragged call -- through
      --parent-lib PATH (another build of the library, e.g. the parent commit's; default: this build);
  (b) ONE `ops.propagate_chunks_ragged` of this build over all chunks.
Also the UNIFORM call (`tf_nn_gather_blend_chunks_segments`, 5 chunks of 8 frames) through the parent library against this
build's: the same code, so the difference is the run-to-run spread of the box.
Per shape: median [min .. max] ms per call over --rounds alternating rounds of 20 calls each (HIP events around the arm's whole
call sequence, so the host's launch issue is inside), and the launches of each arm (the plan functions).

    python tools/ragged_ab.py [--parent-lib PATH] [--rounds N] [--config cfg2]
Cases: a video of 43 frames (chunks 5 x 8 + 3), and two scenes of 23 + 17 frames at 5 frames per chunk."""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokenflow_amd import _lib, ops, workload  # noqa: E402

CASES = [
    ("43 frames, chunks 5 x 8 + 3", [8, 8, 8, 8, 8, 3], 0b1),
    ("scenes of 23 + 17 frames, chunks of 5", [5, 5, 5, 5, 3, 5, 5, 5, 2], 0b100001),
]
UNIFORM = (8, 5, 0b1)       # n, C, mask


INNER = 20      # calls of an arm inside one timed window (a single call at the coarse levels is tens of microseconds)


def ab(arms, rounds, warm=3):
    """Alternating A/B: every round times each arm in turn, INNER calls per window.  {name: (median, min, max)} in ms per call."""
    for _ in range(warm):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(INNER):
                fn()
            b.record()
            torch.cuda.synchronize()
            t[name].append(a.elapsed_time(b) / INNER)
    return {name: (sorted(x)[len(x) // 2], min(x), max(x)) for name, x in t.items()}


def parent_ops(path):
    """(`propagate` of one chunk, the uniform segments call) on dense bf16 tensors through the library at `path`."""
    lib = ctypes.CDLL(path)
    for name in ("tf_nn_gather_blend", "tf_nn_gather_blend_workspace_bytes", "tf_nn_gather_blend_chunks_segments",
                 "tf_nn_gather_blend_chunks_workspace_bytes", "tf_abi_version"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib._SIGNATURES[name]
    ws = {}
    bf, f32 = _lib.TF_BF16, _lib.TF_F32

    def scratch(key, nbytes, dev):
        if key not in ws:
            ws[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        return ws[key]

    def propagate(tgt, piv, inv, kf, w_, n, slot, single, res, out):
        K, S, D = piv.shape
        P = 1 if single else 2
        w = scratch(("1", n, S, D, P), lib.tf_nn_gather_blend_workspace_bytes(n * S, S, D, P), tgt.device)
        rc = lib.tf_nn_gather_blend(tgt.data_ptr(), piv.data_ptr(), inv.data_ptr(), kf.data_ptr(), 0 if single else w_.data_ptr(),
                                    res.data_ptr(), out.data_ptr(), K, n, S, D, P, slot, 0 if single else slot - 1, bf, bf, bf,
                                    bf if single else f32, w.data_ptr(), w.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def chunks(tgt, piv, inv, kf, w_, n, C, mask, res, out):
        K, S, D = piv.shape
        w = scratch(("c", n, S, D, C), lib.tf_nn_gather_blend_chunks_workspace_bytes(n * S, S, D, C), tgt.device)
        rc = lib.tf_nn_gather_blend_chunks_segments(tgt.data_ptr(), piv.data_ptr(), inv.data_ptr(), kf.data_ptr(), w_.data_ptr(),
                                                    res.data_ptr(), out.data_ptr(), K, n, C, S, D, 0, mask, bf, bf, bf, f32, bf,
                                                    w.data_ptr(), w.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return lib.tf_abi_version(), propagate, chunks


def fmt(x):
    return f"{x[0]:7.3f} [{x[1]:7.3f} .. {x[2]:7.3f}]"


def main():
    rounds, path, cfg_name = 15, _lib.LIB_PATH, "cfg2"
    if "--rounds" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1])
    if "--parent-lib" in sys.argv:
        path = sys.argv[sys.argv.index("--parent-lib") + 1]
    if "--config" in sys.argv:
        cfg_name = sys.argv[sys.argv.index("--config") + 1]
    abi, prop1, chunks1 = parent_ops(path)
    print(f"(a) one tf_nn_gather_blend per chunk through {os.path.basename(path)} (ABI {abi}) | (b) one ragged call of this build; "
          f"median [min .. max] ms over {rounds} alternating rounds, bf16, residual and fp32 result as the hooks issue them")
    cfg = workload.CONFIGS[cfg_name]
    g = torch.Generator(device="cuda").manual_seed(0)
    ln = torch.nn.functional.layer_norm
    mk = lambda *shape: torch.randn(*shape, generator=g, device="cuda").bfloat16()     # noqa: E731
    for lvl, (S, D, _h) in enumerate(cfg.levels):
        print(f"{cfg_name} level {lvl} (S={S:5d} D={D:4d}):")
        for title, frames, mask in CASES:
            C, F = len(frames), sum(frames)
            piv = ln(torch.randn(C, S, D, generator=g, device="cuda"), (D,)).bfloat16()
            tgt = ln(torch.randn(F * S, D, generator=g, device="cuda"), (D,)).bfloat16()
            kf, res = mk(3 * C, S, D), mk(3 * F, S, D)
            inv = ops.pivot_inv_norm(piv)
            wn = {n: torch.sigmoid(torch.rand(n, generator=g, device="cuda")) for n in set(frames)}
            w = torch.cat([wn[n] for n in frames]).contiguous()
            per, f0 = [], 0
            for j, n in enumerate(frames):        # every chunk's own dense tensors, made before the clock starts
                single = bool((mask >> j) & 1)
                per.append(dict(tgt=tgt[f0 * S:(f0 + n) * S], n=n, slot=j, single=single, w=wn[n],
                                res=res.view(3, F, S, D)[:, f0:f0 + n].reshape(3 * n, S, D).contiguous(),
                                out=torch.empty(3 * n, S, D, dtype=torch.bfloat16 if single else torch.float32, device="cuda")))
                f0 += n
            out = torch.empty(3 * F, S, D, dtype=torch.float32, device="cuda")
            t = ab({"a": lambda: [prop1(c["tgt"], piv, inv, kf, c["w"], c["n"], c["slot"], c["single"], c["res"], c["out"]) for c in per],
                    "b": lambda: ops.propagate_chunks_ragged(tgt, piv, inv, kf, w, frames, 0, mask, res, torch.float32, out=out)}, rounds)
            la = sum(len([x for x in ops.nn_plan(c["n"] * S, S, D, 1 if c["single"] else 2) if x != "finalize"]) + 1 for c in per)
            plan = ops.propagate_ragged_plan(frames, S, D, mask)
            print(f"    {title}: (a) {fmt(t['a'])} {la:2d} launches | (b) {fmt(t['b'])} {len(plan):2d} launches {plan[0]} | "
                  f"b/a {t['b'][0] / t['a'][0]:.2f}")
        n, C, mask = UNIFORM
        piv = ln(torch.randn(C, S, D, generator=g, device="cuda"), (D,)).bfloat16()
        tgt = ln(torch.randn(C * n * S, D, generator=g, device="cuda"), (D,)).bfloat16()
        kf, res = mk(3 * C, S, D), mk(3 * C * n, S, D)
        inv, w = ops.pivot_inv_norm(piv), torch.sigmoid(torch.rand(n, generator=g, device="cuda"))
        out = torch.empty(3 * C * n, S, D, dtype=torch.float32, device="cuda")
        t = ab({"a": lambda: chunks1(tgt, piv, inv, kf, w, n, C, mask, res, out),
                "b": lambda: ops.propagate_chunks_segments(tgt, piv, inv, kf, w, n, C, 0, mask, res, torch.float32, out=out),
                "b2": lambda: ops.propagate_chunks_segments(tgt, piv, inv, kf, w, n, C, 0, mask, res, torch.float32, out=out)}, rounds)
        print(f"    uniform {C} x {n} frames (the same code in both builds): (a) {fmt(t['a'])} | (b) {fmt(t['b'])} | b/a "
              f"{t['b'][0] / t['a'][0]:.3f} | this build against itself {t['b2'][0] / t['b'][0]:.3f}")


if __name__ == "__main__":
    main()
