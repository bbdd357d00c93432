"""Multi-edit batches (TEST INFRASTRUCTURE): E edits of one source video in one pass, B = 1 + 2E branches
[source | uncond_1 | cond_1 | ... | uncond_E | cond_E].

The definition every test uses: for every op of the path, the slices of the result that belong to edit e (source,
uncond_e, cond_e) are what the single-edit op computes on [source | uncond_e | cond_e].  The oracle (oracle/) knows
nothing of edits; everything here calls it once per edit on the sliced inputs.

  edit_slice / edit_scatter   [B*F, ...] <-> the [3*F, ...] tensor of one edit
  EditFakeOps                 tests/fake_ops.FakeOps plus the *_edits ops, answered by the oracle once per edit
  run_edits_cfg1              the config-1 hook harness for a multi-edit batch (CPU dry run over EditFakeOps, GPU run
                              over the HIP ops)
"""
import copy

import torch

import tokenflow_utils as tfu
from oracle import tokenflow_oracle as orc
from tests import fake_diffusers as fd
from tests.fake_ops import FakeOps
from tokenflow_amd import hooks

CFG1 = dict(K=4, n=2, S=(1024, 256, 64, 16), D=(320, 640, 1280, 1280), heads=8, cross=32, steps=20)
LEVELS = [0, 0, 1, 1, 2, 2, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0]      # UNet execution order of the 16 blocks


def branches_of(e: int):
    """Branch indices (source, uncond_e, cond_e) of edit e (0-based) in the multi-edit batch."""
    return [0, 1 + 2 * e, 2 + 2 * e]


def edit_slice(t: torch.Tensor, e: int, E: int) -> torch.Tensor:
    """[B*F, ...] -> [3*F, ...]: the single-edit tensor [source | uncond_e | cond_e]."""
    B = 1 + 2 * E
    F = t.shape[0] // B
    assert t.shape[0] == B * F
    return t.reshape(B, F, *t.shape[1:])[branches_of(e)].reshape(3 * F, *t.shape[1:])


def edit_scatter(dst: torch.Tensor, src3: torch.Tensor, e: int, E: int, source: bool = True) -> None:
    """Write the single-edit result [3*F, ...] into edit e's branches of dst [B*F, ...] (the source branch on request)."""
    B = 1 + 2 * E
    F = dst.shape[0] // B
    d = dst.view(B, F, *dst.shape[1:])
    s = src3.reshape(3, F, *dst.shape[1:])
    if source:
        d[0] = s[0]
    d[1 + 2 * e], d[2 + 2 * e] = s[1], s[2]


class EditFakeOps(FakeOps):
    """FakeOps that also answers the multi-edit ops, each by E calls of the single-edit oracle-backed op on the sliced
    inputs.  `calls` records the multi-edit call once (not the E inner ones); `nn_idx` keeps the indices of every search."""

    def __init__(self, round16: bool = False):
        super().__init__(round16)
        self.nn_idx = []

    def nn_search(self, tgt, piv, inv_norm, kf_ids):
        idx = super().nn_search(tgt, piv, inv_norm, kf_ids)
        self.nn_idx.append(idx)
        return idx

    def _quiet(self, fn, *a, **kw):
        calls, nn_idx = self.calls, self.nn_idx
        self.calls, self.nn_idx = [], []
        try:
            return fn(*a, **kw), self.nn_idx
        finally:
            self.calls, self.nn_idx = calls, nn_idx

    def ext_attn_edits(self, q, k, v, heads, scale, inject, n_edits, out=None, q_frame0=0, fold_scale=None,
                       out_dtype=None, no_split=None, fused=None, multi_v=None, hints=0):
        self.calls.append(("ext_attn_edits", tuple(q.shape), bool(inject), int(n_edits)))
        E = int(n_edits)
        res = None
        for e in range(E):
            o, _ = self._quiet(FakeOps.ext_attn, self, edit_slice(q, e, E), edit_slice(k, e, E), edit_slice(v, e, E),
                               heads, scale, inject, q_frame0=q_frame0, out_dtype=out_dtype)
            if res is None:
                res = torch.empty(q.shape, dtype=o.dtype)
            edit_scatter(res, o, e, E)
        return res if out is None else out.copy_(res)

    def propagate_chunks_edits(self, tgt, piv, inv_norm, kf_out, w, n, n_chunks, slot0, first_single, residual,
                               out_dtype, n_edits, norm=None):
        self.calls.append(("propagate_chunks_edits", tuple(tgt.shape), int(n_chunks), int(slot0), bool(first_single),
                           int(n_edits)))
        E = int(n_edits)
        res, idx0 = None, None
        for e in range(E):
            r = edit_slice(residual, e, E) if residual is not None else None
            if n_chunks == 1:
                ids = [slot0] if first_single else [slot0, slot0 - 1]
                o, idx = self._quiet(FakeOps.propagate, self, tgt, piv, inv_norm, ids, edit_slice(kf_out, e, E),
                                     None if first_single else w, n, r, out_dtype)
            else:
                o, idx = self._quiet(FakeOps.propagate_chunks, self, tgt, piv, inv_norm, edit_slice(kf_out, e, E), w, n,
                                     n_chunks, slot0, first_single, r, out_dtype)
            if res is None:
                res = torch.empty((1 + 2 * E) * n_chunks * n, *o.shape[1:], dtype=o.dtype)
                idx0 = idx
            edit_scatter(res, o, e, E)
        self.nn_idx.extend(idx0)           # the search is the same for every edit: recorded once
        return self._with_norm(res, norm)

    def inject_copy_edits_(self, x, n_edits):
        self.calls.append(("inject_copy_edits_", tuple(x.shape), int(n_edits)))
        E = int(n_edits)
        for e in range(E):
            edit_scatter(x, orc.conv_inject_(edit_slice(x, e, E).clone()), e, E)
        return x


# ------------------------------------------------------------------------------------------------ config-1 hook harness
def cfg1_timesteps():
    """20 DDIM timesteps (descending), the first 10 / 16 of which inject q/k / features (tests/test_baseline_configs_gpu.py)."""
    ts = [951 - 50 * i for i in range(CFG1["steps"])]
    return ts, ts[:10], ts[:16]


def cfg1_edit_inputs(step: int, E: int):
    """Per block: the multi-edit pivotal input [B*K,S,D] and the K chunk inputs [B*n,S,D]; the source branch video-like
    (frames = permutations of one token set + noise: nearest neighbours far from ties), the edits' branches random and
    different per edit."""
    K, n, B = CFG1["K"], CFG1["n"], 1 + 2 * E
    out = []
    for b, lvl in enumerate(LEVELS):
        g = torch.Generator().manual_seed(4321 + 16 * step + b)
        S, D = CFG1["S"][lvl], CFG1["D"][lvl]
        base = torch.randn(S, D, generator=g)

        def frames(m):
            perm = torch.stack([torch.randperm(S, generator=g) for _ in range(m)])
            return base[perm.reshape(-1)].view(m, S, D) + 0.1 * torch.randn(m, S, D, generator=g)
        piv = torch.cat([frames(K), torch.randn((B - 1) * K, S, D, generator=g)])
        chunks = [torch.cat([frames(n), torch.randn((B - 1) * n, S, D, generator=g)]) for _ in range(K)]
        out.append((piv, chunks))
    g = torch.Generator().manual_seed(77 + step)
    return dict(blocks=out, enc=torch.randn(B * K, 7, CFG1["cross"], generator=g),
                enc_n=torch.randn(B * n, 7, CFG1["cross"], generator=g),
                res_x=torch.randn(B * n, 1280, 8, 8, generator=g), res_temb=torch.randn(B * n, 16, generator=g))


def slice_inputs(inp, e: int, E: int):
    """The single-edit inputs [source | uncond_e | cond_e] of a multi-edit input set."""
    return dict(blocks=[(edit_slice(p, e, E), [edit_slice(c, e, E) for c in ch]) for p, ch in inp["blocks"]],
                enc=edit_slice(inp["enc"], e, E), enc_n=edit_slice(inp["enc_n"], e, E),
                res_x=edit_slice(inp["res_x"], e, E), res_temb=edit_slice(inp["res_temb"], e, E))


class SpyOps:
    """Records the calls of the ops the hooks make -- inputs and outputs on the host -- and forwards them."""
    NAMES = ("ext_attn", "propagate", "propagate_chunks", "inject_copy_", "ext_attn_edits", "propagate_chunks_edits",
             "inject_copy_edits_")

    def __init__(self, real, record=True):
        self._real, self.calls, self.record = real, [], record

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self.NAMES or not callable(fn):
            return fn

        def wrapped(*a, **kw):
            cpu = lambda t: t.detach().cpu().clone() if isinstance(t, torch.Tensor) else t
            args = [cpu(x) for x in a] if self.record else None
            kws = {k_: (tuple(cpu(x) for x in v_) if isinstance(v_, tuple) else cpu(v_)) for k_, v_ in kw.items()} \
                if self.record else None
            out = fn(*a, **kw)
            outs = tuple(cpu(o) for o in out) if isinstance(out, tuple) else cpu(out)
            self.calls.append((name, args, outs if self.record else None, kws))
            return out
        return wrapped


def drive(pipe, inp, t, dev):
    """One denoising step's hook traffic, block by block, as the reference driver issues it."""
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


def check_op_calls(calls, E, check_attn, nn_indices):
    """Every multi-edit op call against per-edit oracle calls on the inputs it received.
    check_attn(out3, q3, k3, v3, heads, scale, inject, what) -> the largest tolerated error: the attention comparison (exact
    over the oracle-backed ops, the kernel bound over the HIP ops); nn_indices(tgt, piv, inv, ids) -> the indices the ops
    under test find.  Returns the per-call attention tolerances (call order = block order)."""
    attn_tol = []
    for ci, (name, a, out, kw) in enumerate(calls):
        if name == "ext_attn_edits":
            q, k, v, heads, scale, inject, n_edits = a[:7]
            assert n_edits == E
            attn_tol.append(max(
                check_attn(edit_slice(out, e, E), edit_slice(q, e, E).float(), edit_slice(k, e, E).float(),
                           edit_slice(v, e, E).float(), heads, scale, inject, f"call {ci} ext_attn_edits edit {e}")
                for e in range(E)))
        elif name == "propagate_chunks_edits":
            tgt, piv, inv, kf, w, n, n_chunks, slot0, first_single, res, out_dtype, n_edits = a[:12]
            assert n_edits == E and n_chunks == 1
            ids = [slot0] if first_single else [slot0, slot0 - 1]
            D = piv.shape[-1]
            sim = orc.batch_cosine_sim(tgt.float(), piv[ids].float().reshape(-1, D))
            idx = [c.argmax(-1) for c in sim.chunk(len(ids), dim=1)]
            o = out[0] if isinstance(out, tuple) else out
            assert o.dtype == out_dtype
            for e in range(E):
                ref = orc.gather_blend(edit_slice(kf, e, E), idx, ids[0], n, residual=edit_slice(res, e, E))
                got = edit_slice(o, e, E)
                assert ref.dtype == got.dtype
                if not torch.equal(got, ref):       # only a near-tie of the search may differ: find the rows, check the gap,
                    found = nn_indices(tgt, piv, inv, ids)      # and hold the VALUES to a gather over the indices found
                    for p_, (r, s_) in enumerate(zip(idx, sim.chunk(len(ids), dim=1))):
                        assert orc.nn_mismatch_tie_aware(s_, r, found[p_].long(), 1e-5)[1] == 0, f"call {ci} edit {e}"
                    ref2 = orc.gather_blend(edit_slice(kf, e, E), [f.long() for f in found], ids[0], n,
                                            residual=edit_slice(res, e, E))
                    assert torch.equal(got, ref2), f"call {ci} edit {e}: gather differs on the indices the search found"
        elif name == "inject_copy_edits_":
            x_before, n_edits = a[:2]
            assert n_edits == E
            for e in range(E):
                assert torch.equal(edit_slice(out, e, E), orc.conv_inject_(edit_slice(x_before, e, E).clone()))
        else:
            raise AssertionError(f"a multi-edit pass called the single-edit op {name}")
    return attn_tol


def run_edits_cfg1(make_ops, dev, monkeypatch, E, steps, check_attn, nn_indices, block_tol=None):
    """Config 1 through the public hook API with a multi-edit batch of E edits (`register_edits`), one step per entry
    of `steps`:
      * call counts per step are the single-edit harness's -- 16 attention calls, one propagation per (block, chunk),
        one feature copy when scheduled: none of them multiplies by E;
      * every op call is checked against per-edit oracle calls on the inputs it received (check_op_calls);
      * every block: the multi-edit input sliced per edit goes through the same block of a SINGLE-EDIT copy of the
        pipeline; the NN-search inputs (norm1 of the source branch: a row-wise LayerNorm, bit-stable across batch
        sizes) and hence the indices must be EQUAL; the block outputs agree within 1e-5 of the output range (the
        tolerance of tests/test_driver_seam.py) where both pipelines run the same arithmetic per edit -- the
        oracle-backed ops.  block_tol(attn_tol) -> absolute tolerance replaces that where they do not: over the HIP ops
        the multi-edit attention is the composition of the bank / source PARTS and the single-edit pipeline's the
        one-call form, different launches whose results each lie within the kernel bound of the oracle.
    make_ops() -> a fresh ops object for one pipeline (EditFakeOps on the CPU, the HIP ops module on the GPU)."""
    torch.manual_seed(0)
    nblk = len(LEVELS)
    base = fd.FakePipeline(dims=CFG1["D"][:3], heads=CFG1["heads"], cross_dim=CFG1["cross"]).eval()
    ts, qk_sched, conv_sched = cfg1_timesteps()
    multi, single = copy.deepcopy(base).to(dev), copy.deepcopy(base).to(dev)
    for pipe in (multi, single):
        tfu.register_extended_attention_pnp(pipe, torch.tensor(qk_sched))
        tfu.register_conv_injection(pipe, torch.tensor(conv_sched))
        tfu.set_tokenflow(pipe.unet)
    tfu.register_edits(multi, E)
    worst = 0.0
    for step in steps:
        t = ts[step]
        inp = cfg1_edit_inputs(step, E)
        spy = SpyOps(make_ops())
        monkeypatch.setattr(hooks, "ops", spy)
        got = drive(multi, inp, t, dev)
        calls = list(spy.calls)
        attn = [c for c in calls if c[0] == "ext_attn_edits"]
        prop = [c for c in calls if c[0] == "propagate_chunks_edits"]
        assert len(attn) == nblk and len(prop) == nblk * CFG1["K"], (len(attn), len(prop))
        assert sum(1 for c in attn if c[1][5]) == (8 if t in qk_sched else 0), step
        assert len([c for c in calls if c[0] == "inject_copy_edits_"]) == (1 if t in conv_sched else 0)
        assert len(calls) == len(attn) + len(prop) + (1 if t in conv_sched else 0)
        for o in got["pivotal"] + sum(got["chunks"], []) + [got["resnet"]]:
            assert bool(torch.isfinite(o).all())
        attn_tol = check_op_calls(calls, E, check_attn, nn_indices)
        # ---- per edit: the same blocks of the single-edit pipeline on the sliced inputs
        for e in range(E):
            spy1 = SpyOps(make_ops())
            monkeypatch.setattr(hooks, "ops", spy1)
            ref = drive(single, slice_inputs(inp, e, E), t, dev)
            prop1 = [c for c in spy1.calls if c[0] == "propagate"]
            assert len(prop1) == len(prop) and not any(c[0].endswith("edits") or c[0].endswith("edits_") for c in spy1.calls)
            for cm, c1 in zip(prop, prop1):
                tgt_m, piv_m, inv_m = cm[1][0], cm[1][1], cm[1][2]
                tgt_1, piv_1, inv_1, ids_1 = c1[1][0], c1[1][1], c1[1][2], list(c1[1][3])
                slot0, first_single = cm[1][7], cm[1][8]
                assert ids_1 == ([slot0] if first_single else [slot0, slot0 - 1])
                # equal search inputs (bit for bit) => equal indices; the indices themselves are compared as well
                assert torch.equal(tgt_m, tgt_1) and torch.equal(piv_m, piv_1) and torch.equal(inv_m, inv_1)
            for cm, c1 in list(zip(prop, prop1))[::max(1, len(prop) // 8)]:
                a = nn_indices(cm[1][0], cm[1][1], cm[1][2], list(c1[1][3]))
                b = nn_indices(c1[1][0], c1[1][1], c1[1][2], list(c1[1][3]))
                assert torch.equal(a, b)
            pairs = [("resnet", got["resnet"], ref["resnet"], None)]
            for i in range(nblk):
                pairs.append((f"block {i} pivotal", got["pivotal"][i], ref["pivotal"][i], i))
                pairs += [(f"block {i} chunk {c}", got["chunks"][c][i], ref["chunks"][c][i], i) for c in range(CFG1["K"])]
            for what, m, r, i in pairs:
                err = float((edit_slice(m, e, E) - r).abs().max())
                rel = err / float(r.abs().max())
                worst = max(worst, rel)
                if block_tol is None or i is None:
                    assert rel <= 1e-5, f"step {step} edit {e} {what}: {rel:.3e} of the output range"
                else:
                    tol = block_tol(attn_tol[i])
                    assert err <= tol, f"step {step} edit {e} {what}: {err:.3e} > {tol:.3e}"
    print(f"multi-edit cfg1 (E={E}): worst block difference from the single-edit pipeline {worst:.3e} of the output range")
    return worst
