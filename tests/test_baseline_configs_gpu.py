"""Parity on BASELINE.json's own configurations, through the public API (needs an MI355X).

* config 1 (8 frames, 256x256 SD1.5, K = 4 keyframes, n = 2, "20 DDIM steps"): the hooks are installed with the
  PUBLIC installers (`register_extended_attention_pnp`, `register_conv_injection`, `set_tokenflow`) on the
  16-block stand-in UNet at the real widths (320/640/1280, 8 heads, S = 1024/256/64/16) and driven by
  `register_time` / `register_pivotal` / `register_batch_idx` exactly as run_tokenflow_pnp.py:198-231 drives
  them, for 20 steps with the driver's schedules (q/k injection on the first int(20*0.5) = 10 timesteps, feature
  injection on the first int(20*0.8) = 16, run_tokenflow_pnp.py:254-255).
* config 4 (SD2.1 @768: K = 10, S = 9216 / 2304, d = 64 -- the ping-pong kernel at 1 440 tiles per bank problem)
  and config 5 (SDEdit, K = 25 > 12: the reference's per-frame loop, tokenflow_utils.py:165) at full size on
  sampled query rows, bf16 and f16.
* the fp32-output mode, the decision data for the folded softmax scale, strongly negative first tiles, the
  multi-chunk propagation call, the fused QKV projection and HIP-graph replay of a pass.

Tolerances are stated where they are asserted.
"""
import copy
import zlib

import pytest
import torch

import tokenflow_utils as tfu
from oracle import tokenflow_oracle as orc
from tests import fake_diffusers as fd
from tests.fake_ops import FakeOps
from tests.test_kernels_gpu import ATTN_ATOL, assert_attn_close, attn_bound, attn_ref
from tokenflow_amd import hooks

pytestmark = pytest.mark.gpu


def _ops():
    from tokenflow_amd import ops
    return ops


# ------------------------------------------------------------------------------------------- config 1, end to end
CFG1 = dict(K=4, n=2, S=(1024, 256, 64, 16), D=(320, 640, 1280, 1280), heads=8, cross=32, steps=20)


def _cfg1_timesteps():
    """20 DDIM timesteps of a 1000-step schedule (descending), the first 10 / 16 of which inject."""
    ts = [951 - 50 * i for i in range(CFG1["steps"])]
    return ts, ts[:int(len(ts) * 0.5)], ts[:int(len(ts) * 0.8)]


def _cfg1_inputs(step):
    """Per block (UNet execution order): pivotal input [3K,S,D] and the 4 chunk inputs [3n,S,D], generator seeded
    1234 + 16*step + block.  Video-like: every frame of the source branch is a permutation
    of one base token set plus noise, so the nearest-neighbour fields are far from ties (as between real frames)."""
    K, n = CFG1["K"], CFG1["n"]
    levels = [0, 0, 1, 1, 2, 2, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0]
    out = []
    for b, lvl in enumerate(levels):
        g = torch.Generator().manual_seed(1234 + 16 * step + b)
        S, D = CFG1["S"][lvl], CFG1["D"][lvl]
        base = torch.randn(S, D, generator=g)

        def frames(m):
            perm = torch.stack([torch.randperm(S, generator=g) for _ in range(m)])
            return base[perm.reshape(-1)].view(m, S, D) + 0.1 * torch.randn(m, S, D, generator=g)
        piv = torch.cat([frames(K), torch.randn(2 * K, S, D, generator=g)])
        chunks = [torch.cat([frames(n), torch.randn(2 * n, S, D, generator=g)]) for _ in range(K)]
        out.append((piv, chunks))
    g = torch.Generator().manual_seed(99 + step)
    return dict(blocks=out, enc=torch.randn(3 * K, 7, CFG1["cross"], generator=g),
                enc_n=torch.randn(3 * n, 7, CFG1["cross"], generator=g),
                res_x=torch.randn(3 * n, 1280, 8, 8, generator=g), res_temb=torch.randn(3 * n, 16, generator=g))


class _SpyOps:
    """Records every call of the HIP ops the hooks make (inputs and outputs, on the host) and forwards it."""

    def __init__(self, real):
        self._real, self.calls, self.record = real, [], False

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in ("ext_attn", "propagate", "inject_copy_") or not callable(fn):
            return fn

        def wrapped(*a, **kw):
            cpu = lambda t: t.detach().cpu().clone() if isinstance(t, torch.Tensor) else t
            args = [cpu(x) for x in a] if self.record else None
            out = fn(*a, **kw)
            meta = bool(a[5]) if name == "ext_attn" else None        # the inject flag
            self.calls.append((name, args, cpu(out) if self.record else None, meta))
            return out
        return wrapped


def _drive(pipe, inp, t, dev):
    """One denoising step's hook traffic, as the reference driver issues it (run_tokenflow_pnp.py:198-231)."""
    blocks = [b for _, b in pipe.unet.transformer_blocks_in_order()]
    outs = dict(pivotal=[], chunks=[])
    tfu.register_time(pipe, t)
    with torch.no_grad():
        tfu.register_pivotal(pipe, True)
        for blk, (x, _) in zip(blocks, inp["blocks"]):
            outs["pivotal"].append(blk(x.to(dev), encoder_hidden_states=inp["enc"].to(dev)).float().cpu())
        tfu.register_pivotal(pipe, False)
        for c in range(CFG1["K"]):
            tfu.register_batch_idx(pipe, c)
            outs["chunks"].append([blk(ch[c].to(dev), encoder_hidden_states=inp["enc_n"].to(dev)).float().cpu()
                                   for blk, (_, ch) in zip(blocks, inp["blocks"])])
        outs["resnet"] = pipe.unet.up_blocks[1].resnets[1](inp["res_x"].to(dev), inp["res_temb"].to(dev)).float().cpu()
    return outs


def test_cfg1_end_to_end_public_installers(monkeypatch):
    """BASELINE config 1 through the public hook API, 20 steps.

    Every step: the injection schedule fires on exactly the 8 decoder blocks / the one resnet for exactly the
    scheduled timesteps, and all outputs are finite.  On one step per injection state (q/k + feature injection,
    feature injection only, none):
      (1) every HIP op call of the step is checked against the oracle ON THE INPUTS IT RECEIVED, at the kernel
          tolerances of tests/test_kernels_gpu.py (attention: 2e-4 + 2^-8 |ref| + 2^-8 softmax.|V|; propagation:
          bit-exact, tie-aware on the indices; feature injection: bit-exact);
      (2) every block output is compared with the SAME hooks run on the CPU over the oracle-backed ops with the
          kernels' rounding points (inputs rounded to bf16, fp32 arithmetic, attention output rounded to bf16).
          Both sides have identical op boundaries and fp32 layers, so they differ by the attention kernel's own
          error carried through the block's remaining layers (to_out, cross-attention, feed-forward: random-init
          stand-ins of gain <= 1): asserted at 1.5x the largest attention bound of that block's call;
      (3) every block output is compared with `oracle.block_forward` in pure fp32 (no rounding anywhere): the
          difference is the bf16 rounding of the kernel inputs (2^-9 relative per element of q, k, v, pivots) plus
          the kernel error of (1): asserted at 1e-3 of the output range (the CPU emulation of the same rounding
          contract measures 3e-5 .. 2e-4 of the range).
    """
    run_cfg1(_ops(), torch.device("cuda"), monkeypatch, steps=range(CFG1["steps"]), full_steps={0, 10, 16})


def run_cfg1(ops, dev, monkeypatch, steps, full_steps):
    """The harness of test_cfg1_end_to_end_public_installers; `ops` is what the hooks under test call (the HIP
    ops on the GPU; tests/test_hooks_cpu.py dry-runs the same harness on the CPU with the oracle-backed ops)."""
    torch.manual_seed(0)
    pipe_cpu = fd.FakePipeline(dims=CFG1["D"][:3], heads=CFG1["heads"], cross_dim=CFG1["cross"]).eval()
    pipe_gpu = copy.deepcopy(pipe_cpu).to(dev)
    ts, qk_sched, conv_sched = _cfg1_timesteps()
    for pipe in (pipe_cpu, pipe_gpu):   # the driver passes schedules as tensors (run_tokenflow_pnp.py:254-257)
        tfu.register_extended_attention_pnp(pipe, torch.tensor(qk_sched))
        tfu.register_conv_injection(pipe, torch.tensor(conv_sched))
        tfu.set_tokenflow(pipe.unet)
    spy = _SpyOps(ops)
    blocks_cpu = [b for _, b in pipe_cpu.unet.transformer_blocks_in_order()]
    injected = {id(pipe_cpu.unet.up_blocks[r].attentions[b].transformer_blocks[0])
                for r, bs in ((1, (1, 2)), (2, (0, 1, 2)), (3, (0, 1, 2))) for b in bs}
    worst = dict(attn=0.0, block=0.0, fp32=0.0)
    for step in steps:
        t = ts[step]
        inp = _cfg1_inputs(step)
        spy.calls.clear()
        spy.record = step in full_steps
        monkeypatch.setattr(hooks, "ops", spy)
        gpu = _drive(pipe_gpu, inp, t, dev)
        calls = list(spy.calls)
        # ---- schedule: 16 attention calls, 8 of them injecting on the first 10 steps; 64 propagations; 1 feature copy
        attn_calls = [c for c in calls if c[0] == "ext_attn"]
        assert len(attn_calls) == 16 and len([c for c in calls if c[0] == "propagate"]) == 64
        assert sum(1 for c in attn_calls if c[3]) == (8 if t in qk_sched else 0), step
        assert len([c for c in calls if c[0] == "inject_copy_"]) == (1 if t in conv_sched else 0)
        for o in gpu["pivotal"] + sum(gpu["chunks"], []) + [gpu["resnet"]]:
            assert bool(torch.isfinite(o).all())
        if step not in full_steps:
            continue
        # ---- (1) every op call against the oracle on its own inputs
        attn_bounds = []
        for name, a, out, kw in calls:
            if name == "ext_attn":
                q, k, v, heads, scale, inject = a[:6]
                d = q.shape[-1] // heads
                refs = attn_ref(q.float(), k.float(), v.float(), heads, scale, inject, need_sigma=False)
                worst["attn"] = max(worst["attn"], assert_attn_close(out, refs, f"step{step} ext_attn"))
                attn_bounds.append(float(attn_bound(refs[0], refs[1], torch.bfloat16).max()))
            elif name == "propagate":
                tgt, piv, inv, ids, kf, w, n, res, out_dtype = a
                S, D = piv.shape[1:]
                sim = orc.batch_cosine_sim(tgt.float(), piv[list(ids)].float().reshape(-1, D))
                idx = [c.argmax(-1) for c in sim.chunk(len(ids), dim=1)]
                ref = orc.gather_blend(kf, idx, ids[0], n, residual=res)       # ids = [c] or [c, c-1]
                assert ref.dtype == out.dtype == out_dtype
                if not torch.equal(out, ref):       # only a near-tie may differ: find the rows, check the gap
                    got = ops.nn_search(tgt.to(dev), piv.to(dev), inv.to(dev), list(ids)).cpu()
                    for p_, (r, s_) in enumerate(zip(idx, sim.chunk(len(ids), dim=1))):
                        assert orc.nn_mismatch_tie_aware(s_, r, got[p_], 1e-5)[1] == 0
            else:
                x_before = a[0]
                assert torch.equal(out, orc.conv_inject_(x_before.clone()))
        # ---- (2) same hooks on the CPU over oracle-backed ops with the kernels' rounding points
        monkeypatch.setattr(hooks, "ops", FakeOps(round16=True))
        cpu = _drive(pipe_cpu, inp, t, "cpu")
        for i in range(16):
            tol = 1.5 * attn_bounds[i]
            for what, a_, b_ in [("pivotal", gpu["pivotal"][i], cpu["pivotal"][i])] + \
                                [(f"chunk{c}", gpu["chunks"][c][i], cpu["chunks"][c][i]) for c in range(CFG1["K"])]:
                err = float((a_ - b_).abs().max())
                worst["block"] = max(worst["block"], err)
                assert err <= tol, f"step {step} block {i} {what}: {err:.3e} > {tol:.3e}"
        assert float((gpu["resnet"] - cpu["resnet"]).abs().max()) <= 1e-3 * float(cpu["resnet"].abs().max())
        # ---- (3) pure fp32 oracle.block_forward
        states = [orc.BlockState() for _ in range(16)]
        with torch.no_grad():
            for i, (blk, (x, chunks)) in enumerate(zip(blocks_cpu, inp["blocks"])):
                inj = orc.should_inject(t, qk_sched if id(blk) in injected else [])
                ref = orc.block_forward(blk, states[i], x, pivotal=True, inject=inj, encoder_hidden_states=inp["enc"])
                pairs = [(gpu["pivotal"][i], ref)]
                for c in range(CFG1["K"]):
                    pairs.append((gpu["chunks"][c][i], orc.block_forward(
                        blk, states[i], chunks[c], pivotal=False, batch_idx=c, encoder_hidden_states=inp["enc_n"])))
                for got, ref in pairs:
                    rel = float((got - ref).abs().max() / ref.abs().max())
                    worst["fp32"] = max(worst["fp32"], rel)
                    assert rel <= 1e-3, f"step {step} block {i}: {rel:.3e} of the output range"
    print(f"cfg1 e2e: worst attention err {worst['attn']:.3e}, worst block err vs rounding-matched CPU hooks "
          f"{worst['block']:.3e}, vs pure fp32 oracle {worst['fp32']:.3e} of range")


# ------------------------------------------------------------------------------------------- configs 4 and 5
def _oracle_rows(q, k, v, K, S, h, d, b, f, head, rows, inject):
    """fp32 oracle for a few query rows of one (branch, frame, head): tokenflow_utils.py:173-179."""
    qv, kv, vv = (t.view(3, K, S, h, d) for t in (q, k, v))
    bq = 0 if (inject and b > 0) else b
    qr = qv[bq, f, rows, head].float()
    if b == 0:
        kk, vals = kv[0, f, :, head].float(), vv[0, f, :, head].float()
    else:
        kk, vals = kv[bq, :, :, head].reshape(K * S, d).float(), vv[b, :, :, head].reshape(K * S, d).float()
    p = torch.softmax(qr @ kk.T * d ** -0.5, dim=-1)
    return p @ vals, p @ vals.abs()


CFG45 = {  # name: (K, S, heads, d, variants (inject flags))
    "cfg4_L0": (10, 9216, 5, 64, (False, True)),
    "cfg4_L1": (10, 2304, 10, 64, (False, True)),
    "cfg5_L0": (25, 4096, 5, 64, (False,)),       # SDEdit: register_extended_attention never injects
    "cfg5_L1": (25, 1024, 10, 64, (False,)),
}


@pytest.mark.parametrize("name", list(CFG45))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ext_attn_cfg4_cfg5_sampled_rows(name, dtype):
    """Full-size attention of configs 4 and 5 (the reference cannot materialise these score matrices: 31.6 and
    39 GiB per head and branch) on sampled query rows of sampled (branch, frame, head) problems against the
    fp32 oracle.  Tolerance: per-token deviation < 1e-3 (north star) as the plain number on the fp32 output
    (TF_ATTN_OUT_F32); the 16-bit output within 1e-3 + half an ulp of the reference value (what any tensor of that
    type is off by), and for f16 also within its parity bound 2e-4 + 2^-11 (|ref| + softmax.|V|).
    (Rounds 1-3 asserted the plain 1e-3 on the bf16 OUTPUT tensor, which held only because |out| < 0.25 at these bank
    sizes; round 4 moved the absolute check to the fp32 output -- the quantity the kernel controls -- and bounds the
    16-bit tensor by its own format: half an ulp of a bf16 value in [0.5, 1) is already 1.95e-3.)"""
    ops = _ops()
    K, S, h, d, variants = CFG45[name]
    D = h * d
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(name.encode()) % 1000)
    q, k, v = (torch.randn(3 * K, S, D, generator=g, device="cuda").to(dtype) for _ in range(3))
    qc, kc, vc = q.cpu(), k.cpu(), v.cpu()
    rows = torch.tensor([0, 1, 31, 32, 63, 64, 255, 256, S // 2 + 5, S - 257, S - 2, S - 1])
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    for inject in variants:
        out = ops.ext_attn(q, k, v, h, d ** -0.5, inject)
        out32 = ops.ext_attn(q, k, v, h, d ** -0.5, inject, out_dtype=torch.float32)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
        oc, oc32 = out.float().cpu().view(3, K, S, h, d), out32.cpu().view(3, K, S, h, d)
        worst32 = 0.0
        ulp_exp = 8 if dtype == torch.bfloat16 else 11
        for b, f, head in [(0, 0, 0), (0, K - 1, h - 1), (1, 0, h // 2), (1, K - 1, 0), (2, K // 2, h - 1), (2, K - 2, 1)]:
            ref, ref_abs = _oracle_rows(qc, kc, vc, K, S, h, d, b, f, head, rows, inject)
            err = (oc[b, f, rows, head] - ref).abs()
            half_ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - ulp_exp)
            assert float((err - (1e-3 + half_ulp)).max()) <= 0, f"{name} inject {inject} ({b},{f},{head}): {float(err.max()):.3e}"
            if dtype == torch.float16:
                assert float((err - (ATTN_ATOL + eps * (ref.abs() + ref_abs))).max()) <= 0
            worst32 = max(worst32, float((oc32[b, f, rows, head] - ref).abs().max()))
        assert worst32 < 1e-3, f"{name} inject {inject}: max per-token deviation (fp32 output) {worst32:.3e}"


# ------------------------------------------------------------------------------------------- fp32 output mode
@pytest.mark.parametrize("K,S,h,d", [(8, 256, 8, 160), (8, 64, 8, 160), (4, 1024, 8, 40), (3, 520, 2, 64), (2, 264, 1, 80)])
@pytest.mark.parametrize("inject", [False, True])
def test_ext_attn_fp32_output(K, S, h, d, inject):
    """TF_ATTN_OUT_F32: the normalised fp32 accumulator is stored unrounded.  (a) rounding it to bf16 on the host
    reproduces the default call bit for bit (same accumulator, one rounding) when the call runs one pass;
    (b) against the oracle the output-rounding term of the bound disappears:  2e-4 + 2^-8 softmax.|V| -- on the short source problems of the coarse levels, where |out| > 0.256
    makes a bf16 output miss 1e-3 by construction, the fp32 output is inside it."""
    # (the bound has no folded-scale term: fp32 score scaling is the default at every head dim)
    ops = _ops()
    g = torch.Generator().manual_seed(K + S + d)
    D = h * d
    q, k, v = (orc.bf16_round(torch.randn(3 * K, S, D, generator=g)) for _ in range(3))
    dq, dk, dv = (t.bfloat16().cuda() for t in (q, k, v))
    import tokenflow_amd.ops as real_ops
    old = real_ops.NO_SPLIT
    real_ops.NO_SPLIT = True
    try:
        o16 = ops.ext_attn(dq, dk, dv, h, d ** -0.5, inject)
        o32 = ops.ext_attn(dq, dk, dv, h, d ** -0.5, inject, out_dtype=torch.float32)
    finally:
        real_ops.NO_SPLIT = old
    assert o32.dtype == torch.float32 and o32.shape == o16.shape
    assert torch.equal(o32.to(torch.bfloat16), o16)
    ref, ref_abs, _ = attn_ref(q, k, v, h, d ** -0.5, inject, need_sigma=False)
    bound = ATTN_ATOL + 2.0 ** -8 * ref_abs + 2.0 ** -24 * ref.abs()
    err = (o32.cpu() - ref).abs()
    assert float((err - bound).max()) <= 0, f"fp32 out: {float(err.max()):.3e}"
    o32s = ops.ext_attn(dq, dk, dv, h, d ** -0.5, inject, out_dtype=torch.float32)     # split form where it applies
    assert float(((o32s.cpu() - ref).abs() - bound).max()) <= 0


def test_ext_attn_fp32_output_meets_1e3_where_bf16_cannot():
    """cfg2 level 2 (S = 256, d = 160), source branch: outputs reach |o| ~ 0.3-0.5, so a bf16 output carries up
    to 2^-9 |o| > 1e-3 of rounding alone; the fp32 output is within the north star's 1e-3 per token."""
    ops = _ops()
    K, S, h, d = 8, 256, 8, 160
    g = torch.Generator(device="cuda").manual_seed(102)
    q, k, v = (torch.randn(3 * K, S, h * d, generator=g, device="cuda").bfloat16() for _ in range(3))
    out = ops.ext_attn(q, k, v, h, d ** -0.5, False, out_dtype=torch.float32).cpu().view(3, K, S, h, d)
    qc, kc, vc = q.cpu(), k.cpu(), v.cpu()
    rows = torch.arange(0, S, 5)
    worst = 0.0
    for b, f, head in [(0, 0, 0), (0, K - 1, h - 1), (0, 3, 4), (1, 2, 3), (2, 5, 7)]:
        ref, _ = _oracle_rows(qc, kc, vc, K, S, h, d, b, f, head, rows, False)
        worst = max(worst, float((out[b, f, rows, head] - ref).abs().max()))
    assert worst < 1e-3, worst


# ------------------------------------------------------------------------------------------- first-tile underflow
@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ext_attn_strongly_negative_first_tile(d, dtype):
    """Every score of the first 64-key tile far below zero (q.k*scale ~ -110 < -88: exp2 of the shift difference
    overflows fp32): the folded-shift kernels (Dh = 40) used to compute 0 * inf = NaN on the first tile."""
    ops = _ops()
    K, S, h = 2, 256, 2
    g = torch.Generator().manual_seed(d)
    D = h * d
    q, k, v = (torch.randn(3 * K, S, D, generator=g) for _ in range(3))
    u = torch.nn.functional.normalize(torch.randn(h, d, generator=g), dim=-1)
    amp = (110.0 * d ** 0.5) ** 0.5                              # |q.k| * d^-0.5 = 110
    q = (amp * u.view(1, 1, h, d) + 0.05 * q.view(3 * K, S, h, d)).reshape(3 * K, S, D)
    kv = k.view(3 * K, S, h, d)
    kv[:, :64] = -amp * u.view(1, 1, h, d) + 0.05 * kv[:, :64]     # first tile of every frame: anti-aligned keys
    k = kv.reshape(3 * K, S, D)
    rnd = orc.bf16_round if dtype == torch.bfloat16 else (lambda x: x.half().float())
    q, k, v = rnd(q), rnd(k), rnd(v)
    for inject in (False, True):
        out = ops.ext_attn(q.to(dtype).cuda(), k.to(dtype).cuda(), v.to(dtype).cuda(), h, d ** -0.5, inject)
        assert bool(torch.isfinite(out.float()).all()), f"d={d} {dtype} inject={inject}: non-finite output"
        refs = attn_ref(q, k, v, h, d ** -0.5, inject)
        assert_attn_close(out, refs, f"negative first tile d={d} {dtype} inject={inject}", dtype=dtype)
        if d == 40:
            out = ops.ext_attn(q.to(dtype).cuda(), k.to(dtype).cuda(), v.to(dtype).cuda(), h, d ** -0.5, inject,
                               fold_scale=True)
            assert bool(torch.isfinite(out.float()).all()), f"fold d={d} {dtype} inject={inject}: non-finite output"
            assert_attn_close(out, refs, f"negative first tile fold {dtype} inject={inject}", dtype=dtype, folded=True)


# ------------------------------------------------------------------------------------------- multi-chunk propagation
@pytest.mark.parametrize("K,n,S,D", [(8, 5, 4096, 320), (8, 5, 1024, 640), (4, 2, 64, 1280), (4, 2, 16, 1280),
                                     (5, 3, 200, 72), (3, 8, 576, 1280), (3, 3, 200, 320), (4, 1, 45, 320),
                                     # multi-chunk launches of the LDS-DMA search whose pivot tile is the whole frame
                                     # (cfg5 level 2) / half empty (128 pivots in a 256-row tile), and cfg1 level 0
                                     (12, 8, 256, 1280), (24, 8, 128, 1280), (4, 2, 1024, 320)])
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("res_dtype", [torch.bfloat16, torch.float32])
def test_propagate_chunks_equals_per_chunk_calls(K, n, S, D, first, res_dtype):
    """tf_nn_gather_blend_chunks over chunks first..K-1 in one call == K - first calls of tf_nn_gather_blend, bit
    for bit (the one-keyframe chunk 0 rounded to the dtype its own pass would produce, then widened)."""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(41 + S)
    ln = torch.nn.functional.layer_norm
    piv = ln(torch.randn(K, S, D, generator=g, device="cuda"), (D,)).bfloat16()
    inv = ops.pivot_inv_norm(piv)
    kf_out = torch.randn(3 * K, S, D, generator=g, device="cuda").bfloat16()
    C = K - first
    tgt = ln(torch.randn(C * n * S, D, generator=g, device="cuda"), (D,)).bfloat16()
    res = torch.randn(3, C, n, S, D, generator=g, device="cuda").to(res_dtype)
    w = orc.blend_weights(n, 1).cuda()
    want = []
    for j in range(C):
        c = first + j
        ids = [c] if c == 0 else [c, c - 1]
        r = res[:, j].reshape(3 * n, S, D)
        dt = torch.promote_types(torch.float32 if len(ids) == 2 else kf_out.dtype, res_dtype)
        want.append(ops.propagate(tgt[j * n * S:(j + 1) * n * S], piv, inv, ids, kf_out, w if len(ids) == 2 else None,
                                  n, r, dt).float().view(3, n, S, D))
    want = torch.stack(want, dim=1).reshape(3 * C * n, S, D)
    got = ops.propagate_chunks(tgt, piv, inv, kf_out, w, n, C, first, first == 0, res.reshape(3 * C * n, S, D),
                               torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, want)


@pytest.mark.parametrize("K,n,S,D", [(3, 2, 1024, 320), (3, 3, 200, 640), (3, 2, 64, 1280), (3, 2, 45, 72)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("affine", [True, False])
def test_propagate_with_fused_norm_equals_propagate_then_layer_norm(K, n, S, D, dtype, affine):
    """tf_nn_gather_blend_norm / tf_nn_gather_blend_chunks_norm (the block's next LayerNorm in the gather's epilogue):
    the result tensor is bit-identical to the unfused call's and the norm bit-identical to tf_layer_norm of that
    result -- one keyframe (model-dtype result), two keyframes (fp32 result) and the multi-chunk call with and
    without the one-keyframe chunk."""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(77 + S)
    ln = torch.nn.functional.layer_norm
    piv = ln(torch.randn(K, S, D, generator=g, device="cuda"), (D,)).to(dtype)
    inv = ops.pivot_inv_norm(piv)
    kf_out = torch.randn(3 * K, S, D, generator=g, device="cuda").to(dtype)
    w = orc.blend_weights(n, 1).cuda()
    gamma = (1 + 0.1 * torch.randn(D, generator=g, device="cuda")).to(dtype) if affine else None
    beta = (0.1 * torch.randn(D, generator=g, device="cuda")).to(dtype) if affine else None
    for ids in ([0], [2, 1]):
        P = len(ids)
        tgt = ln(torch.randn(n * S, D, generator=g, device="cuda"), (D,)).to(dtype)
        res = (2 * torch.randn(3 * n, S, D, generator=g, device="cuda")).to(dtype)
        odt = torch.float32 if P == 2 else dtype
        assert ops.norm_fusable(kf_out, res, odt, P, dtype)
        want = ops.propagate(tgt, piv, inv, ids, kf_out, w if P == 2 else None, n, res, odt)
        want_n, _ = ops.layer_norm(want, gamma, beta, 1e-5, dtype)
        got, got_n = ops.propagate(tgt, piv, inv, ids, kf_out, w if P == 2 else None, n, res, odt,
                                   norm=(gamma, beta, 1e-5, dtype))
        assert got.dtype == odt and got_n.dtype == dtype
        assert torch.equal(got, want) and torch.equal(got_n, want_n), (ids, float((got_n.float() - want_n.float()).abs().max()))
    for first in (0, 1):
        C = K - first
        tgt = ln(torch.randn(C * n * S, D, generator=g, device="cuda"), (D,)).to(dtype)
        res = torch.randn(3 * C * n, S, D, generator=g, device="cuda").to(dtype)
        want = ops.propagate_chunks(tgt, piv, inv, kf_out, w, n, C, first, first == 0, res, torch.float32)
        want_n, _ = ops.layer_norm(want, gamma, beta, 1e-5, dtype)
        got, got_n = ops.propagate_chunks(tgt, piv, inv, kf_out, w, n, C, first, first == 0, res, torch.float32,
                                          norm=(gamma, beta, 1e-5, dtype))
        assert torch.equal(got, want) and torch.equal(got_n, want_n), first
    # what the fused form does not cover is refused, not silently computed some other way
    assert not ops.norm_fusable(kf_out, res.float(), torch.float32, 2, dtype)
    with pytest.raises(TypeError):
        ops.propagate_chunks(tgt, piv, inv, kf_out, w, n, C, first, first == 0, res.float(), torch.float32,
                             norm=(gamma, beta, 1e-5, dtype))


def test_hooks_chunk_pass_fused_gather_norm_equals_unfused(monkeypatch):
    """A propagation pass of a 16-bit block under autocast with the gather+norm fusion (the default) against the same
    pass with TOKENFLOW_FUSED_GATHER_NORM off: identical block outputs, and the fused call really is the one taken."""
    ops = _ops()
    dev = torch.device("cuda")
    holder, blk = _one_block_pipe(320, 8, dev, torch.bfloat16)
    K, n, S = 3, 2, 256
    g = torch.Generator().manual_seed(5)
    calls = []
    real = ops.propagate
    monkeypatch.setattr(hooks.ops, "propagate", lambda *a, **kw: (calls.append(kw.get("norm") is not None), real(*a, **kw))[1])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        tfu.register_pivotal(holder, True)
        blk(torch.randn(3 * K, S, 320, generator=g).bfloat16().to(dev), encoder_hidden_states=torch.randn(3 * K, 7, 32, generator=g).bfloat16().to(dev))
        tfu.register_pivotal(holder, False)
        x = torch.randn(3 * n, S, 320, generator=g).bfloat16().to(dev)
        enc = torch.randn(3 * n, 7, 32, generator=g).bfloat16().to(dev)
        outs = {}
        for fused in (True, False):
            monkeypatch.setattr(hooks, "FUSE_GATHER_NORM", fused)
            for c in (0, 2):
                tfu.register_batch_idx(holder, c)
                outs[(fused, c)] = blk(x, encoder_hidden_states=enc)
    assert calls == [True, True, False, False]
    for c in (0, 2):
        assert torch.equal(outs[(True, c)], outs[(False, c)])


# ------------------------------------------------------------------------------------------- hook-level pieces
def _one_block_pipe(D, heads, dev, dtype):
    torch.manual_seed(0)
    blk = fd.BasicTransformerBlock(D, heads, cross_dim=32).eval()
    holder = torch.nn.Module()
    holder.unet = torch.nn.Module()
    holder.unet.blk = blk
    holder.to(dev).to(dtype)
    blk.attn1.forward = hooks._make_sa_forward(blk.attn1, pnp=True)
    hooks._set_schedule(blk.attn1, [5])
    blk.attn1.t = 5
    tfu.set_tokenflow(holder)
    return holder, blk


def test_fused_qkv_projection_matches_separate_projections(monkeypatch):
    """One [3K,S,3D] GEMM read in place by the attention kernel (row stride 3D) against the three Linear calls:
    q, k, v agree to the last bit or one 16-bit ulp (the BLAS library may tile N = 3D differently from N = D),
    and the block output within the 16-bit rounding of the stream."""
    holder, blk = _one_block_pipe(640, 8, "cuda", torch.bfloat16)
    K, S = 4, 256
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3 * K, S, 640, generator=g).cuda().bfloat16()
    enc = torch.randn(3 * K, 7, 32, generator=g).cuda().bfloat16()
    # while autograd is recording and the weights require grad the fused form steps aside (the cached concatenation is
    # built without autograd): the three Linear calls stay
    assert hooks._fused_qkv(blk.attn1, x) is None
    with torch.no_grad():
        qkv = hooks._fused_qkv(blk.attn1, x)
        assert qkv is not None and qkv.shape == (3 * K, S, 1920) and qkv.dtype == torch.bfloat16
        for i, lin in enumerate((blk.attn1.to_q, blk.attn1.to_k, blk.attn1.to_v)):
            a, b = qkv[..., 640 * i:640 * (i + 1)].float(), lin(x).float()
            assert float(((a - b).abs() - 2.0 ** -7 * b.abs()).max()) <= 1e-6
    outs = []
    for fuse in (True, False):
        monkeypatch.setattr(hooks, "FUSE_QKV", fuse)
        with torch.no_grad():
            tfu.register_pivotal(holder, True)
            outs.append(blk(x, encoder_hidden_states=enc).float())
    assert float((outs[0] - outs[1]).abs().max()) <= 2.0 ** -6 * float(outs[1].abs().max())
    # the cache follows the weights
    with torch.no_grad():
        blk.attn1.to_k.weight.mul_(2.0)
        assert torch.allclose(hooks._fused_qkv(blk.attn1, x)[..., 640:1280].float(), blk.attn1.to_k(x).float(),
                              rtol=2.0 ** -6, atol=1e-3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_hipgraph_replay_of_hook_passes(dtype):
    """A pivotal pass and a propagation pass captured into HIP graphs (tokenflow_amd.graphs.GraphCache) replay to
    the same bits as the eager passes, for new input contents (bf16, and f16 -- the reference's own autocast dtype)."""
    from tokenflow_amd.graphs import GraphCache
    holder, blk = _one_block_pipe(320, 8, "cuda", dtype)
    K, n, S = 4, 2, 1024
    g = torch.Generator().manual_seed(3)
    enc, enc_n = (torch.randn(3 * m, 7, 32, generator=g).cuda().to(dtype) for m in (K, n))

    def mk(m):
        return torch.randn(3 * m, S, 320, generator=g).cuda().to(dtype)

    def pivotal(x):
        tfu.register_pivotal(holder, True)
        return blk(x, encoder_hidden_states=enc)

    def chunk(x):
        tfu.register_pivotal(holder, False)
        tfu.register_batch_idx(holder, 2)
        return blk(x, encoder_hidden_states=enc_n)

    cache = GraphCache()
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        for rep in range(3):
            xp, xc = mk(K), mk(n)
            want_p = pivotal(xp).clone()
            want_c = chunk(xc).clone()
            got_p = cache.run(("pivotal", True), pivotal, xp).clone()
            got_c = cache.run(("chunk", 2, True), chunk, xc).clone()
            torch.cuda.synchronize()
            assert torch.equal(got_p, want_p) and torch.equal(got_c, want_c), rep
    assert len(cache) == 2


@pytest.mark.parametrize("native", [False, True])
def test_hipgraph_replay_of_a_sharded_rank(native):
    """The hook passes of ONE rank of a frame-sharded run (register_frame_shard on the library's loopback transport:
    rank 3 of 8, every exchange a stream-ordered local copy) captured into HIP graphs: the pivotal pass ends with
    hooks.join_frame_shard (a capture joins the halo stream before it ends), the chunk pass then waits for nothing.
    Replays equal the eager passes bit for bit, for new input contents."""
    from tokenflow_amd import sharded
    from tokenflow_amd.comm import HipComm
    from tokenflow_amd.graphs import GraphCache
    dtype = torch.bfloat16
    holder, blk = _one_block_pipe(640, 8, "cuda", dtype)
    K, n, S = 8, 2, 256
    comm, hcomm = HipComm.loopback(3, 8), HipComm.loopback(3, 8)
    shard = (sharded.NativeShard(K, comm, hcomm) if native else sharded.FrameShard(K, comm=comm, halo_comm=hcomm))
    hooks.register_frame_shard(holder, shard)
    g = torch.Generator().manual_seed(4)
    enc, enc_n = (torch.randn(3 * m, 7, 32, generator=g).cuda().to(dtype) for m in (shard.Kl, n))

    def mk(m):
        return torch.randn(3 * m, S, 640, generator=g).cuda().to(dtype)

    def pivotal(x, join):
        tfu.register_pivotal(holder, True)
        y = blk(x, encoder_hidden_states=enc)
        if join:
            hooks.join_frame_shard(holder)
        return y

    def chunk(x):
        tfu.register_pivotal(holder, False)
        tfu.register_batch_idx(holder, shard.kf0)
        return blk(x, encoder_hidden_states=enc_n)

    cache = GraphCache()
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
            for rep in range(3):
                xp, xc = mk(shard.Kl), mk(n)
                want_p = pivotal(xp, False).clone()
                want_c = chunk(xc).clone()                 # eager: the chunk pass waits for the halo itself
                got_p = cache.run(("pivotal", True), lambda x: pivotal(x, True), xp).clone()
                got_c = cache.run(("chunk", shard.kf0, True), chunk, xc).clone()
                torch.cuda.synchronize()
                assert torch.equal(got_p, want_p) and torch.equal(got_c, want_c), rep
        assert len(cache) == 2
    finally:
        hooks.register_frame_shard(holder, None)
        if native:
            shard.close()
        comm.close()
        hcomm.close()


# ------------------------------------------------------------------------------------------- collective-shaped layouts
@pytest.mark.parametrize("K,S,h,d", [(4, 320, 2, 40), (3, 136, 2, 64), (2, 264, 1, 80), (2, 72, 1, 160), (5, 1024, 1, 40),
                                     (4, 4096, 8, 40)])       # the last one: the interleaved Dh = 40 kernel
@pytest.mark.parametrize("inject", [False, True])
def test_ext_attn_strided_views_equal_dense(K, S, h, d, inject, monkeypatch):
    """tf_ext_attn_fwd_strided on the buffers of the head re-sharding -- q / k / v read from a [frame][slab][S][D]
    all-to-all receive buffer, the output written into a [frame][branch][S][D] send buffer -- must equal the dense
    call bit for bit (one-pass form: the arithmetic of a (query, head) does not depend on the layout)."""
    ops = _ops()
    monkeypatch.setattr(ops, "NO_SPLIT", True)
    D = h * d
    g = torch.Generator(device="cuda").manual_seed(S + d)
    q, k, v = (torch.randn(3 * K, S, D, generator=g, device="cuda").bfloat16() for _ in range(3))
    dense = ops.ext_attn(q, k, v, h, d ** -0.5, inject, part="bank", out=torch.zeros_like(q)).view(3, K, S, D)
    q3, k3, v3 = (t.view(3, K, S, D) for t in (q, k, v))
    slabs = [q3[0], k3[0], v3[1], v3[2]] if inject else [q3[1], q3[2], k3[1], k3[2], v3[1], v3[2]]
    recv = torch.stack(slabs, dim=1).contiguous()                 # [K, ns, S, D]: what the first all-to-all delivers
    rp = recv.permute(1, 0, 2, 3)
    send2 = torch.full((K, 2, S, D), 7.0, dtype=q.dtype, device="cuda")
    o4 = send2.permute(1, 0, 2, 3)
    if inject:
        ops.ext_attn_views(rp[0:1], rp[1:2], rp[2:4], o4, h, d ** -0.5, True, "bank", branch0=(0, 0, 1, 1))
    else:
        ops.ext_attn_views(rp[0:2], rp[2:4], rp[4:6], o4, h, d ** -0.5, False, "bank", branch0=(1, 1, 1, 1))
    assert torch.equal(o4, dense[1:3])
    # full call on dense 4-D views == the 3-D call
    full = ops.ext_attn(q, k, v, h, d ** -0.5, inject).view(3, K, S, D)
    out = torch.empty_like(full)
    ops.ext_attn_views(q3, k3, v3, out, h, d ** -0.5, inject)
    assert torch.equal(out, full)


@pytest.mark.parametrize("W,Kl,S,D,dtype", [(8, 1, 4096, 320, torch.bfloat16), (2, 3, 200, 160, torch.float16),
                                             (4, 2, 64, 1280, torch.bfloat16), (2, 2, 45, 80, torch.float32)])
def test_head_pack_unpack(W, Kl, S, D, dtype):
    """tf_head_pack / tf_head_unpack against the torch formulation of the same re-layout (bit-exact: pure copies),
    with strided source slabs (column slabs of a fused projection output)."""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(W + S)
    fused = torch.randn(3 * Kl, S, 3 * D, generator=g, device="cuda").to(dtype)
    q3, k3, v3 = (fused[..., i * D:(i + 1) * D].unflatten(0, (3, Kl)) for i in range(3))
    slabs = [q3[1], q3[2], k3[1], k3[2], v3[1], v3[2]]
    hd = D // W
    send = ops.head_pack(slabs, W)
    want = torch.stack([t.reshape(Kl, S, W, hd) for t in slabs], dim=1).permute(3, 0, 1, 2, 4)
    assert send.shape == (W, Kl, 6, S, hd) and torch.equal(send, want)
    recv2 = torch.randn(W, Kl, 2, S, hd, generator=g, device="cuda").to(dtype)
    out = torch.zeros(3, Kl, S, D, dtype=dtype, device="cuda")
    ops.head_unpack(recv2, [out[1], out[2]])
    assert torch.equal(out[1:3].view(2, Kl, S, W, hd), recv2.permute(2, 1, 3, 0, 4))
    assert bool((out[0] == 0).all())


# ------------------------------------------------------------------------------------------- interleaved Dh = 40 kernel
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("gain", [0.0, 3.0, 12.0])
def test_ext_attn_interleaved_form_full_oracle(dtype, gain):
    """The Dh = 40 interleaved kernel in its LDS-DMA form (il<40,8,ALL,4,2>: fp32 scaling, grids of >= 256 eight-wave
    workgroups, S % 64 == 0; 768 here, below the 1024 from which the mixed-shape form is the default) against the full
    oracle, K = 4 x S = 2048 x 8 heads, without injection (the injected forms: tests/test_kernel_forms_gpu.py).  gain > 0 plants spikes (one strongly aligned key per
    query, in LATE tiles of the bank): gain 3 keeps the score bound tight enough that no half tile looks at its
    maximum, gain 12 breaks it so that the deferred shift moves in the middle of the software pipeline -- the
    half tile whose P.V runs beside that softmax was exponentiated against the OLD shift and must be rescaled
    exactly once (cdna_hip_programming.md T13 / rule 26).  Both the bank problems (K*S keys) and the source problems."""
    ops = _ops()
    K, S, h, d = 4, 2048, 8, 40
    D = h * d
    g = torch.Generator().manual_seed(int(gain) + 5)
    q, k, v = (torch.randn(3 * K, S, D, generator=g) for _ in range(3))
    if gain:
        qv, kv = q.view(3 * K, S, h, d), k.view(3 * K, S, h, d)
        for b in range(3 * K):
            for s_ in range(0, S, 3):
                kv[b, (s_ * 5 + 1500) % S] = qv[b, s_] * gain      # lands in tiles 0..31 of a frame, mostly late ones
    rnd = orc.bf16_round if dtype == torch.bfloat16 else (lambda x: x.half().float())
    q, k, v = rnd(q), rnd(k), rnd(v)
    refs = attn_ref(q, k, v, h, d ** -0.5, False, need_sigma=False)
    dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
    assert ops.attn_plan(K, K, S, h, d, False, dtype=dtype) == ["vt_pack", "il<40,8,ALL,4,2>"]
    out = ops.ext_attn(dq, dk, dv, h, d ** -0.5, False)
    assert bool(torch.isfinite(out.float()).all())
    assert_attn_close(out, refs, f"interleaved gain={gain} {dtype}", dtype=dtype)
    o32 = ops.ext_attn(dq, dk, dv, h, d ** -0.5, False, out_dtype=torch.float32)
    assert torch.equal(o32.to(dtype), out)
    src = ops.ext_attn(dq, dk, dv, h, d ** -0.5, False, part="source", out=torch.zeros_like(dq))
    assert torch.equal(src.view(3, -1)[0], out.view(3, -1)[0]) and bool((src.view(3, -1)[1:] == 0).all())


def test_ext_attn_interleaved_form_negative_first_tile():
    """The first tile 158 binades below the rest, at the interleaved kernel's size."""
    ops = _ops()
    K, S, h, d = 4, 2048, 8, 40
    D = h * d
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(3 * K, S, D, generator=g) for _ in range(3))
    u = torch.nn.functional.normalize(torch.randn(h, d, generator=g), dim=-1)
    amp = (110.0 * d ** 0.5) ** 0.5
    q = (amp * u.view(1, 1, h, d) + 0.05 * q.view(3 * K, S, h, d)).reshape(3 * K, S, D)
    kv = k.view(3 * K, S, h, d)
    kv[:, :64] = -amp * u.view(1, 1, h, d) + 0.05 * kv[:, :64]
    q, k, v = (orc.bf16_round(t) for t in (q, kv.reshape(3 * K, S, D), v))
    out = ops.ext_attn(q.bfloat16().cuda(), k.bfloat16().cuda(), v.bfloat16().cuda(), h, d ** -0.5, False)
    assert bool(torch.isfinite(out.float()).all())
    assert_attn_close(out, attn_ref(q, k, v, h, d ** -0.5, False, need_sigma=False), "interleaved, negative first tile")


# ------------------------------------------------------------------------------------------- SDEdit installer, K > 12
def test_sdedit_installer_many_keyframes():
    """`register_extended_attention` (the SDEdit driver's installer, tokenflow_utils.py:216-294: never injects, not
    even at t = 1000) + `set_tokenflow` on the stand-in UNet with K = 13 keyframes -- beyond the 12 up to which the
    reference batches the frames of a pass (165-168) -- one block per level, pivotal pass and two chunks, against
    pure fp32 `oracle.block_forward` (1e-3 of the output range, as in the config-1 test)."""
    K, n = 13, 2
    dev = torch.device("cuda")
    torch.manual_seed(1)
    pipe_cpu = fd.FakePipeline(dims=(320, 640, 1280), heads=8, cross_dim=32).eval()
    pipe_gpu = copy.deepcopy(pipe_cpu).to(dev)
    tfu.register_extended_attention(pipe_gpu)
    tfu.set_tokenflow(pipe_gpu.unet)
    tfu.register_time(pipe_gpu, 1000)
    blocks_c = pipe_cpu.unet.transformer_blocks_in_order()
    blocks_g = pipe_gpu.unet.transformer_blocks_in_order()
    g = torch.Generator().manual_seed(3)
    for idx, S in ((0, 256), (2, 64), (6, 16)):
        (lvl, bc), (_, bg) = blocks_c[idx], blocks_g[idx]
        D = (320, 640, 1280, 1280)[lvl]
        base = torch.randn(S, D, generator=g)

        def frames(m):
            perm = torch.stack([torch.randperm(S, generator=g) for _ in range(m)])
            return base[perm.reshape(-1)].view(m, S, D) + 0.1 * torch.randn(m, S, D, generator=g)
        x = torch.cat([frames(K), torch.randn(2 * K, S, D, generator=g)])
        enc, enc_n = torch.randn(3 * K, 7, 32, generator=g), torch.randn(3 * n, 7, 32, generator=g)
        st = orc.BlockState()
        with torch.no_grad():
            tfu.register_pivotal(pipe_gpu, True)
            got = bg(x.to(dev), encoder_hidden_states=enc.to(dev)).float().cpu()
            ref = orc.block_forward(bc, st, x, pivotal=True, inject=False, encoder_hidden_states=enc)
            assert float((got - ref).abs().max() / ref.abs().max()) <= 1e-3
            tfu.register_pivotal(pipe_gpu, False)
            for c in (0, 12):
                xc = torch.cat([frames(n), torch.randn(2 * n, S, D, generator=g)])
                tfu.register_batch_idx(pipe_gpu, c)
                got = bg(xc.to(dev), encoder_hidden_states=enc_n.to(dev)).float().cpu()
                ref = orc.block_forward(bc, st, xc, pivotal=False, batch_idx=c, encoder_hidden_states=enc_n)
                assert got.dtype == ref.dtype
                assert float((got - ref).abs().max() / ref.abs().max()) <= 1e-3, (idx, c)


def test_hooks_multi_chunk_pass_on_gpu():
    """`register_batch_idx(model, range(...))`: one pass over all chunks through the real kernels equals the
    per-chunk passes bit for bit (bf16 block under autocast, as the reference runs)."""
    holder, blk = _one_block_pipe(320, 8, "cuda", torch.bfloat16)
    K, n, S = 4, 2, 256
    g = torch.Generator().manual_seed(4)
    enc = torch.randn(3 * K, 7, 32, generator=g).cuda().bfloat16()
    enc_n = torch.randn(3 * n, 7, 32, generator=g).cuda().bfloat16()
    x_piv = torch.randn(3 * K, S, 320, generator=g).cuda().bfloat16()
    chunks = [torch.randn(3 * n, S, 320, generator=g).cuda().bfloat16() for _ in range(K)]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        tfu.register_pivotal(holder, True)
        blk(x_piv, encoder_hidden_states=enc)
        tfu.register_pivotal(holder, False)
        for first in (0, 1):
            ref = []
            for c in range(first, K):
                tfu.register_batch_idx(holder, c)
                ref.append(blk(chunks[c], encoder_hidden_states=enc_n).float().view(3, n, S, 320))
            C = K - first
            x_all = torch.stack([chunks[c].view(3, n, S, 320) for c in range(first, K)], dim=1).reshape(3 * C * n, S, 320)
            enc_all = enc_n.view(3, 1, n, 7, 32).expand(3, C, n, 7, 32).reshape(3 * C * n, 7, 32)
            tfu.register_batch_idx(holder, range(first, K))
            got = blk(x_all, encoder_hidden_states=enc_all).float().view(3, C, n, S, 320)
            want = torch.stack(ref, dim=1)
            # the propagation itself is bit-identical; the layers behind it (fp32 chunk-0 rows arrive widened instead
            # of bf16) may round differently in the last bf16 place
            assert float((got - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max()), first


# ------------------------------------------------------------------------------------------- row f4: DDIM update
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_ddim_step_bit_exact(dtype):
    """tf_ddim_step against the oracle's restatement of preprocess.py:224-225 (per-op rounding to the tensor dtype,
    fp32 scalars, no FMA, IEEE division): bit-exact, out of place and in place, at the reference's latents size
    (40 x 4 x 64 x 64) and at an odd element count."""
    ops = _ops()
    g = torch.Generator().manual_seed(7)
    for shape in ((40, 4, 64, 64), (3, 4, 9, 5)):
        x, eps = (torch.randn(*shape, generator=g).to(dtype) for _ in range(2))
        co = (0.9734, 0.2291, 0.9581, 0.2864)
        ref = orc.ddim_step(x, eps, *co)
        dx = x.cuda()
        out = ops.ddim_step(dx, eps.cuda(), *co)
        assert out.dtype == dtype and torch.equal(out.cpu(), ref)
        assert torch.equal(dx.cpu(), x)
        ops.ddim_step(dx, eps.cuda(), *co, out=dx)
        assert torch.equal(dx.cpu(), ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_ddim_step_vs_torch_gpu_sequence(dtype):
    """The same update as torch evaluates preprocess.py:224-225 ON THE GPU, coefficients as 0-dim CPU tensors the way
    `scheduler.alphas_cumprod[t] ** 0.5` arrives there.  torch's GPU true-divide by a host scalar multiplies by an
    fp32 reciprocal, the kernel divides (IEEE, = torch on the CPU, which the golden fixture pins): pred_x0 may differ
    by one rounding of the tensor dtype, which the last two ops carry through -- bound: 2 ulp of the dtype (4 in
    fp32) at the magnitude of the two summands (the sum itself may cancel), on a fraction of the elements."""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    x, eps = (torch.randn(40, 4, 64, 64, generator=g).to(dtype).cuda() for _ in range(2))
    a_prev, a_t = torch.tensor(0.9475), torch.tensor(0.9180)          # alphas_cumprod entries (CPU, fp32)
    mu_a, sg_a, mu_b, sg_b = a_prev ** 0.5, (1 - a_prev) ** 0.5, a_t ** 0.5, (1 - a_t) ** 0.5
    pred_x0 = (x - sg_a * eps) / mu_a                                   # the reference's lines, on the GPU
    ref = mu_b * pred_x0 + sg_b * eps
    out = ops.ddim_step(x, eps, float(mu_a), float(sg_a), float(mu_b), float(sg_b))
    assert out.dtype == ref.dtype == dtype
    ulp = {torch.float32: 2.0 ** -23, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}[dtype]
    err = (out.float() - ref.float()).abs()
    mag = (mu_b * pred_x0).float().abs() + (sg_b * eps).float().abs()
    tol = (4 if dtype == torch.float32 else 2) * ulp * mag.clamp_min(2.0 ** -6)
    assert bool((err <= tol).all()), float((err / tol).max())
    assert float((err > 0).float().mean()) < 0.25


def test_ddim_inversion_on_gpu_against_reference_golden(tmp_path):
    """The inversion + reconstruction loops of `tokenflow_amd.inversion` on the GPU (HIP update kernel, stand-in
    UNet evaluated by torch on the GPU) against the verbatim reference's CPU run: 2e-5 (the stand-in's tanh differs
    between the two devices in the last fp32 bits; the update itself is bit-exact, test above)."""
    import os
    from oracle import golden_cases as gc
    from oracle.golden_util import check
    from tests.conftest import load_golden
    from tokenflow_amd import inversion
    g = load_golden("inversion.pt")
    model = gc.InversionModel()
    model.w = model.w.cuda()
    latents, cond = gc.inversion_inputs()
    os.makedirs(tmp_path / "latents")
    inv = inversion.ddim_inversion(model, cond.cuda(), latents.cuda(), str(tmp_path), gc.INVERSION_CFG["batch_size"],
                                   save_latents=True, timesteps_to_save=model.scheduler.timesteps[::2])
    assert sorted(os.listdir(tmp_path / "latents")) == sorted(g["files"])
    for name, dg in g["files"].items():
        check(torch.load(tmp_path / "latents" / name).cpu(), dg, 2e-5, name)
    check(inv.cpu(), g["inverted"], 2e-5, "inverted")
    rec = inversion.ddim_sample(model, inv.clone(), cond.cuda(), gc.INVERSION_CFG["batch_size"])
    check(rec.cpu(), g["reconstructed"], 2e-4, "reconstructed")


def test_ext_attn_interleaved_form_query_frame_subset(monkeypatch):
    """The interleaved kernel with the queries of a frame subset against the full bank (what a rank of the
    bank-all-gather exchange computes: Kq = 2 of K = 4 frames, q_frame0 = 2): equal to the matching slices of the
    full call, bit for bit."""
    ops = _ops()
    monkeypatch.setattr(ops, "NO_SPLIT", True)
    K, S, h, d = 4, 4096, 8, 40
    g = torch.Generator(device="cuda").manual_seed(12)
    q, k, v = (torch.randn(3 * K, S, h * d, generator=g, device="cuda").bfloat16() for _ in range(3))
    full = ops.ext_attn(q, k, v, h, d ** -0.5, False).view(3, K, S, h * d)
    part = ops.ext_attn(q.view(3, K, S, h * d)[:, 2:4].reshape(6, S, h * d), k, v, h, d ** -0.5, False, q_frame0=2)
    assert torch.equal(part.view(3, 2, S, h * d), full[:, 2:4])


@pytest.mark.parametrize("inject", [False, True])
def test_ext_attn_d64_interleaved_query_frame_subset(inject, monkeypatch):
    """Head dim 64 (BASELINE configs 4 / 5: 5 heads do not divide over 8 ranks, so a rank takes the bank exchange): the
    queries of a frame subset against the full bank in the interleaved d = 64 kernel (LDS-DMA staged tiles, score bound,
    matrix-pipe denominator; with injection the dual-V image) equal the matching slices of the full call, bit for bit."""
    ops = _ops()
    monkeypatch.setattr(ops, "NO_SPLIT", True)
    K, S, h, d = 5, 1024, 5, 64
    g = torch.Generator(device="cuda").manual_seed(13)
    q, k, v = (torch.randn(3 * K, S, h * d, generator=g, device="cuda").bfloat16() for _ in range(3))
    full = ops.ext_attn(q, k, v, h, d ** -0.5, inject).view(3, K, S, h * d)
    part = ops.ext_attn(q.view(3, K, S, h * d)[:, 3:5].reshape(6, S, h * d), k, v, h, d ** -0.5, inject, q_frame0=3)
    assert torch.equal(part.view(3, 2, S, h * d), full[:, 3:5])
