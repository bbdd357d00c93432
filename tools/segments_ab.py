#!/usr/bin/env python
"""A/B of the keyframe-segment ops at BASELINE block shapes, alternating on one box:
  (a) V single-clip passes -- per clip one `ext_attn` and one all-chunks `propagate_chunks` -- through --single-lib PATH
      (another build of the library, e.g. the parent commit's; default: this build);
  (b) ONE segmented pass of this build: `ops.ext_attn_segments` and `ops.propagate_chunks_segments` over all V clips.
Per block shape: attention and propagation as median [min .. max] ms over --rounds alternating rounds (HIP events around the
arm's whole call sequence, so the host's launch issue is inside), and the launches of each arm (the plan functions).

    python tools/segments_ab.py [--single-lib PATH] [--rounds N]
Shapes: config 1's four levels with V = 2 and V = 4 clips of its 4 keyframes; levels 2-3 of config 2 as segments [4, 4]."""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokenflow_amd import _lib, ops, workload  # noqa: E402


def ab(arms, rounds, warm=3):
    """Alternating A/B: every round times each arm once, in turn.  {name: (median, min, max)} in ms."""
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


def single_clip_ops(path):
    """(`ext_attn`, `propagate_chunks` with first_single) on dense bf16 tensors through the library at `path`."""
    lib = ctypes.CDLL(path)
    for name in ("tf_ext_attn_fwd", "tf_ext_attn_workspace_bytes", "tf_nn_gather_blend_chunks",
                 "tf_nn_gather_blend_chunks_workspace_bytes", "tf_abi_version"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib._SIGNATURES[name]
    ws = {}

    def scratch(key, nbytes, dev):
        if key not in ws:
            ws[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        return ws[key]

    def ext_attn(q, k, v, h, scale, inject, out):
        K, S, D = k.shape[0] // 3, k.shape[1], k.shape[2]
        key = (K, S, h, D // h, _lib.TF_BF16)
        w = scratch(("a",) + key, lib.tf_ext_attn_workspace_bytes(*key), q.device)
        rc = lib.tf_ext_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), K, K, 0, S, h, D // h, D,
                                 float(scale), 1 if inject else 0, _lib.TF_BF16, w.data_ptr(), w.numel(),
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def propagate_chunks(tgt, piv, inv, kf, w_, n, C, res, out):
        K, S, D = piv.shape
        w = scratch(("p", n, S, D, C), lib.tf_nn_gather_blend_chunks_workspace_bytes(n * S, S, D, C), tgt.device)
        rc = lib.tf_nn_gather_blend_chunks(tgt.data_ptr(), piv.data_ptr(), inv.data_ptr(), kf.data_ptr(), w_.data_ptr(),
                                           res.data_ptr(), out.data_ptr(), K, n, C, S, D, 0, 1, _lib.TF_BF16, _lib.TF_BF16,
                                           _lib.TF_BF16, _lib.TF_F32, _lib.TF_BF16, w.data_ptr(), w.numel(),
                                           torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return lib.tf_abi_version(), ext_attn, propagate_chunks


def fmt(x):
    return f"{x[0]:7.3f} [{x[1]:7.3f} .. {x[2]:7.3f}]"


def main():
    rounds, path = 15, _lib.LIB_PATH
    if "--rounds" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1])
    if "--single-lib" in sys.argv:
        path = sys.argv[sys.argv.index("--single-lib") + 1]
    abi, attn1, prop1 = single_clip_ops(path)
    print(f"(a) V single-clip passes through {os.path.basename(path)} (ABI {abi}) | (b) one segmented pass of this build; "
          f"median [min .. max] ms over {rounds} alternating rounds, bf16, q/k injection on")
    cases = [("cfg1", lvl, [4] * V) for V in (2, 4) for lvl in range(4)] + [("cfg2", lvl, [4, 4]) for lvl in (2, 3)]
    g = torch.Generator(device="cuda").manual_seed(0)
    ln = torch.nn.functional.layer_norm
    for name, lvl, segs in cases:
        cfg = workload.CONFIGS[name]
        S, D, h = cfg.levels[lvl]
        n, K, V, dh = cfg.chunk, sum(segs), len(segs), D // h
        mk = lambda *shape: torch.randn(*shape, generator=g, device="cuda").bfloat16()     # noqa: E731
        q, k, v = mk(3 * K, S, D), mk(3 * K, S, D), mk(3 * K, S, D)
        piv = ln(torch.randn(K, S, D, generator=g, device="cuda"), (D,)).bfloat16()
        tgt = ln(torch.randn(K * n * S, D, generator=g, device="cuda"), (D,)).bfloat16()
        kf, res = mk(3 * K, S, D), mk(3 * K * n, S, D)
        inv, w = ops.pivot_inv_norm(piv), torch.sigmoid(torch.rand(n, generator=g, device="cuda"))
        win = lambda t, F, f0, f1: t.view(3, F, *t.shape[1:])[:, f0:f1].reshape(3 * (f1 - f0), *t.shape[1:]).contiguous()   # noqa: E731
        clips, f0 = [], 0
        for kv in segs:       # every clip's own dense tensors, made before the clock starts
            clips.append(dict(q=win(q, K, f0, f0 + kv), k=win(k, K, f0, f0 + kv), v=win(v, K, f0, f0 + kv),
                              out=torch.empty(3 * kv, S, D, dtype=torch.bfloat16, device="cuda"),
                              piv=piv[f0:f0 + kv].contiguous(), inv=inv[f0:f0 + kv].contiguous(), kf=win(kf, K, f0, f0 + kv),
                              tgt=tgt[f0 * n * S:(f0 + kv) * n * S].contiguous(), res=win(res.view(3 * K, n * S, D), K, f0, f0 + kv),
                              pout=torch.empty(3 * kv * n, S, D, dtype=torch.float32, device="cuda"), kv=kv))
            f0 += kv
        out = torch.empty(3 * K, S, D, dtype=torch.bfloat16, device="cuda")
        mask = sum(1 << sum(segs[:i]) for i in range(V))
        t_attn = ab({"a": lambda: [attn1(c["q"], c["k"], c["v"], h, dh ** -0.5, True, c["out"]) for c in clips],
                     "b": lambda: ops.ext_attn_segments(q, k, v, h, dh ** -0.5, True, segs, out=out)}, rounds)
        t_prop = ab({"a": lambda: [prop1(c["tgt"], c["piv"], c["inv"], c["kf"], w, n, c["kv"], c["res"], c["pout"]) for c in clips],
                     "b": lambda: ops.propagate_chunks_segments(tgt, piv, inv, kf, w, n, K, 0, mask, res, torch.float32)}, rounds)
        la = sum(len(ops.attn_plan(kv, kv, S, h, dh, True)) for kv in segs)
        lb = len(ops.attn_segments_plan(K, segs, S, h, dh, True))
        pa = sum(len([t for t in ops.nn_plan(n * S, S, D, 2, kv) if t != "finalize"]) + 1 for kv in segs)
        pb = len(ops.propagate_segments_plan(n, K, S, D, mask))
        print(f"{name} level {lvl} (S={S:5d} D={D:4d} h={h}) segments {segs}:")
        print(f"    attention    (a) {fmt(t_attn['a'])} {la:2d} launches | (b) {fmt(t_attn['b'])} {lb:2d} launches | b/a {t_attn['b'][0] / t_attn['a'][0]:.2f}")
        print(f"    propagation  (a) {fmt(t_prop['a'])} {pa:2d} launches | (b) {fmt(t_prop['b'])} {pb:2d} launches | b/a {t_prop['b'][0] / t_prop['a'][0]:.2f}")
        print(f"    block        (a) {t_attn['a'][0] + t_prop['a'][0]:7.3f} {la + pa:2d} launches | (b) {t_attn['b'][0] + t_prop['b'][0]:7.3f} {lb + pb:2d} launches | "
              f"b/a {(t_attn['b'][0] + t_prop['b'][0]) / (t_attn['a'][0] + t_prop['a'][0]):.2f}")


if __name__ == "__main__":
    main()
