"""Sliding-window keyframe bank on the GPU (tf_ext_attn_fwd_windows, hooks.register_bank_window): the uncond / cond branches of
keyframe i attend to the keys of the bank frames of window i only.

  * q, k, v are independent per frame, so a launch that read a frame outside the window -- or missed one inside -- lands O(1)
    off.  Every frame is held to the oracle on its window's slices, within the attention bound of tests/test_kernels_gpu.py,
    on N(0,1) and on peaked inputs, with 16-bit and fp32 output, in the default mode (where small grids split the WINDOW into
    runs; a window shorter than the split leaves empty runs) and under no_split.
  * Frame i's OWN CALL is `ops.ext_attn` on the window's tensors with Kq = 1, q_frame0 = i - win_lo[i].  Under no_split the
    windowed call is bit-identical to it wherever the two plans name the same kernel form (asserted as a precondition on the
    CPU with the plan functions; the shapes are the smallest at which the windowed launch is the fused kernel, one<, il<, the
    ping-pong kernel, the Dh = 80 and Dh = 160 forms).
  * planted keys at the window's edge, a mid-size GPU-vs-GPU case, one block through `register_bank_window`."""
import re

import pytest
import torch

import tokenflow_utils as tfu
from oracle import golden_cases as gc
from tests import fake_diffusers as fd
from tests.test_kernels_gpu import assert_attn_close, attn_bound, attn_ref
from tokenflow_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
K_ATTN = 6
IRREGULAR = [(0, 1), (0, 3), (1, 4), (3, 1), (2, 4), (4, 2)]


def _ops():
    from tokenflow_amd import ops
    return ops


def _tables():
    ops = _ops()
    return {"R1": ops.bank_windows(K_ATTN, 1), "R2": ops.bank_windows(K_ATTN, 2), "irregular": IRREGULAR}


# (S, H, Dh, kwargs, form of the windowed launch under no_split)
ATTN_CASES = [
    (48, 2, 40, {}, "fused"),                                                      # ragged S
    (192, 2, 160, {}, "fused"),
    (320, 2, 64, {"fused": False}, "one<64"),                                      # one-tile streaming, ragged
    (512, 2, 40, {"fused": False, "hints": _lib.TF_ATTN_HINT_MIX}, "il<40"),       # interleaved (DUAL under injection)
    (576, 2, 64, {"fused": False}, "il<64"),                                       # interleaved, LDS-DMA staged (the cfg4 / cfg5 form)
    (520, 2, 64, {"fused": False}, "pp<64"),                                       # ping-pong: ragged S >= 512, one pass
    (320, 2, 80, {}, "il<80"),                                                     # Dh 80: fused in the default mode on this grid
    (128, 2, 160, {"fused": False}, "one<160"),                                    # Dh 160 streams in the ALL form under injection too
]


def _rnd(x, dtype):
    return x.to(dtype).float()


def _attn_inputs(K, S, D, kind, seed):
    """Independent q, k, v for every frame.  peaked: planted keys of gain 12 inside every frame, many in its last 64-key tile
    (the family of tests/test_segments_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(3 * K, S, D, generator=g) for _ in range(3))
    if kind == "peaked":
        s_ = torch.arange(0, S, 5)
        k[:, (s_ * 3 + S - 60) % S] = q[:, s_] * 12.0
    return q, k, v


def _win(t, K, f0, f1):
    return t.view(3, K, *t.shape[1:])[:, f0:f1].reshape(3 * (f1 - f0), *t.shape[1:])


def _frame_refs(q, k, v, K, windows, H, scale, inject):
    """Per frame: the oracle on the window's slices, frame i's rows -- (ref, softmax.|V|) as [3, S, D] each."""
    refs = []
    for i, (lo, n) in enumerate(windows):
        r, ra, _ = attn_ref(_win(q, K, lo, lo + n), _win(k, K, lo, lo + n), _win(v, K, lo, lo + n), H, scale, inject,
                            need_sigma=False)
        pick = lambda t: t.view(3, n, *t.shape[1:])[:, i - lo]      # noqa: E731
        refs.append((pick(r), pick(ra), None))
    return refs


def _own_call(ops, dq, dk, dv, K, i, lo, n, H, scale, inject, **kw):
    return ops.ext_attn(_win(dq, K, i, i + 1).contiguous(), _win(dk, K, lo, lo + n).contiguous(),
                        _win(dv, K, lo, lo + n).contiguous(), H, scale, inject, q_frame0=i - lo, **kw)


def _same_form(win_plan, own_plan):
    """The two plans name the same kernel form: the same launches but for the ',win' mark; fused launches agree in what their
    arithmetic depends on (KW and PREC: include/tokenflow_hip.h), whatever their query waves."""
    strip = lambda p: [re.sub(r"qw=\d,", "", t.replace(",win", "")) for t in p]      # noqa: E731
    return strip(win_plan) == strip(own_plan)


@pytest.mark.parametrize("S,H,Dh,kw,form", ATTN_CASES, ids=[f"S{c[0]}-Dh{c[2]}-{c[4].strip('<')}" for c in ATTN_CASES])
@pytest.mark.parametrize("table", ["R1", "R2", "irregular"])
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_windows(S, H, Dh, kw, form, table, inject, dtype):
    ops = _ops()
    K, windows = K_ATTN, _tables()[table]
    D, scale = H * Dh, Dh ** -0.5
    plans = {ns: ops.attn_windows_plan(K, windows, S, H, Dh, inject, dtype=dtype, no_split=ns, **kw) for ns in (False, True)}
    # the case is what its name says: one windowed launch of the named form under no_split, one pre-pass unless it is fused
    marked = [t for t in plans[True] if t.endswith(",win") or t.endswith(",win]")]
    want = "one<64" if inject and form == "pp<64" else form      # (injection at Dh 64, ragged S: the DUAL one-tile form)
    assert len(marked) == 1 and marked[0].startswith(want), plans[True]
    assert all(p.count("vt_pack") == (0 if p[0].startswith("fused") else 1) for p in plans.values()), plans
    if table == "irregular" and not plans[False][0].startswith("fused") and Dh != 160:      # (4 tiles at Dh 160, S 128: no split)
        assert any(t.startswith("merge[nseg=4]") for t in plans[False]), plans[False]      # empty runs: windows of 1 and 3 frames
    n_equal = 0
    for kind in ("randn", "peaked"):
        q, k, v = (_rnd(t, dtype) for t in _attn_inputs(K, S, D, kind, seed=S + Dh + len(kind)))
        dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
        refs = _frame_refs(q, k, v, K, windows, H, scale, inject)
        for no_split in (False, True):
            got = ops.ext_attn_windows(dq, dk, dv, H, scale, inject, windows, no_split=no_split, **kw)
            assert torch.isfinite(got.float()).all()
            got32 = ops.ext_attn_windows(dq, dk, dv, H, scale, inject, windows, no_split=no_split, out_dtype=torch.float32, **kw)
            assert got32.dtype == torch.float32 and torch.equal(got32.to(dtype), got)
            for i, (lo, n) in enumerate(windows):
                what = f"S{S} Dh{Dh} {table} inject={inject} no_split={no_split} {kind} {dtype} frame {i} window [{lo}, {lo + n})"
                err = assert_attn_close(_win(got, K, i, i + 1), refs[i], what, dtype=dtype)
                assert_attn_close(_win(got32, K, i, i + 1), refs[i], what + " fp32 out", dtype=dtype)
                if not no_split:
                    continue
                own_plan = ops.attn_plan(n, 1, S, H, Dh, inject, dtype=dtype, no_split=True, **kw)
                same_form = _same_form(plans[True], own_plan)
                alone = _own_call(ops, dq, dk, dv, K, i, lo, n, H, scale, inject, no_split=True, **kw)
                same = torch.equal(_win(got, K, i, i + 1), alone)
                print(f"{what}: max abs err {err:.3e}, same form as its own call: {same_form}, equal to it: {same}")
                assert same_form, (plans[True], own_plan)      # the shapes are chosen so that the precondition holds
                assert same, what
                n_equal += 1
    assert n_equal == 2 * K


def test_full_windows_and_refusals():
    ops = _ops()
    S, H, Dh, K = 64, 2, 40, K_ATTN
    q, k, v = (t.bfloat16().cuda() for t in _attn_inputs(K, S, H * Dh, "randn", 3))
    for R in (K - 1, K + 4):
        assert torch.equal(ops.ext_attn_windows(q, k, v, H, Dh ** -0.5, True, ops.bank_windows(K, R)),
                           ops.ext_attn(q, k, v, H, Dh ** -0.5, True))
    with pytest.raises(ValueError):
        ops.ext_attn_windows(q, k, v, H, Dh ** -0.5, True, ops.bank_windows(K - 1, 1))
    with pytest.raises(ValueError, match="own frame"):
        ops.ext_attn_windows(q, k, v, H, Dh ** -0.5, True, [(0, 2)] * K)
    with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_fwd_windows"):
        ops.ext_attn_windows(q, k, v, H, Dh ** -0.5, True, ops.bank_windows(K, 1), hints=_lib.TF_ATTN_MULTI_V)


@pytest.mark.parametrize("S,H,Dh,kw", [(48, 2, 40, {}), (320, 2, 64, {"fused": False}),
                                      (512, 2, 40, {"fused": False, "hints": _lib.TF_ATTN_HINT_MIX})],
                         ids=["fused", "one", "il"])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("inject", [False, True])
def test_planted_key_at_the_window_edge(S, H, Dh, kw, R, inject):
    """A gain-12 match for frame f's queries placed in frame f + R (the window's last frame) must dominate the output: the value
    planted beside it comes out.  The same match in frame f + R + 1 must leave no trace: bit for bit the unplanted result."""
    ops = _ops()
    K, f, D, scale = K_ATTN, 1, H * Dh, Dh ** -0.5
    windows = ops.bank_windows(K, R)
    q, k, v = (_rnd(t, torch.bfloat16) for t in _attn_inputs(K, S, D, "randn", seed=7 + R))
    rows = torch.arange(0, S, 3)
    qsrc = 0 if inject else None                                     # injection: the bank branches use the source's q and k

    def planted(frame):
        k2, v2 = k.clone().view(3, K, S, D), v.clone().view(3, K, S, D)
        for b in (1, 2):
            bq = b if qsrc is None else qsrc
            k2[bq, frame, (rows + 1) % S] = _rnd(q.view(3, K, S, D)[bq, f, rows] * 12.0, torch.bfloat16)
            v2[b, frame, (rows + 1) % S] = 100.0 + b
        return k2.view(3 * K, S, D), v2.view(3 * K, S, D)

    dq = q.bfloat16().cuda()
    for no_split in (False, True):
        run = lambda kk, vv: ops.ext_attn_windows(dq, kk.bfloat16().cuda(), vv.bfloat16().cuda(), H, scale, inject, windows,   # noqa: E731
                                                  no_split=no_split, **kw).float().view(3, K, S, D)
        base = run(k, v)
        inside = run(*planted(f + R))
        for b in (1, 2):
            # logit of the match: 12 |q|^2 scale ~ 12 sqrt(Dh) >= 75 above the N(0, 1) scores of <= 3000 other keys
            assert torch.allclose(inside[b, f, rows], torch.full_like(inside[b, f, rows], 100.0 + b), rtol=2.0 ** -7), (b, no_split)
            assert not torch.allclose(base[b, f, rows], inside[b, f, rows], rtol=0.5)
        k_out, v_out = planted(f + R + 1)
        outside = run(k_out, v_out)
        # frame f sees nothing of frame f + R + 1 (with injection its source keys were overwritten too: frame f's own source
        # branch reads frame f only)
        assert torch.equal(outside[:, f], base[:, f]), no_split
        assert not torch.equal(outside[1, f + 1], base[1, f + 1])      # ... which frame f + 1's window does hold


def test_midsize_against_the_frames_own_calls():
    """BASELINE config 2, level 0: K = 8, S = 1024, H = 8, Dh = 40, radius 2 -- no CPU oracle at this size; every frame against
    its own call on the GPU, within the attention bound of it (reference and softmax.|V| from own calls, the latter on |v|), in
    the default mode and under no_split.  Only the BOUND is checked at this size: the own calls (Kq = 1) have an eighth of the
    grid and take another kernel form than the 8-frame windowed launch (asserted below), so there is no bit-identity to ask for;
    that half of the contract is test_attention_windows' business, where every frame shares its own call's form."""
    ops = _ops()
    K, S, H, Dh, R = 8, 1024, 8, 40, 2
    D, scale, dtype = H * Dh, Dh ** -0.5, torch.bfloat16
    windows = ops.bank_windows(K, R)
    g = torch.Generator(device="cuda").manual_seed(5)
    dq, dk, dv = (torch.randn(3 * K, S, D, generator=g, device="cuda").to(dtype) for _ in range(3))
    for inject in (False, True):
        for no_split in (False, True):
            plan = ops.attn_windows_plan(K, windows, S, H, Dh, inject, dtype=dtype, no_split=no_split)
            assert plan[0] == "vt_pack" and plan[1].startswith("il<40") and plan[1].endswith(",win"), plan
            got = ops.ext_attn_windows(dq, dk, dv, H, scale, inject, windows, no_split=no_split)
            for i, (lo, n) in enumerate(windows):
                own = _own_call(ops, dq, dk, dv, K, i, lo, n, H, scale, inject, no_split=no_split, out_dtype=torch.float32)
                own_abs = _own_call(ops, dq, dk, dv.abs(), K, i, lo, n, H, scale, inject, no_split=no_split, out_dtype=torch.float32)
                err = (_win(got, K, i, i + 1).float() - own).abs()
                worst = float((err - attn_bound(own, own_abs, dtype)).max())
                assert worst <= 0, f"frame {i} inject={inject} no_split={no_split}: max abs err {float(err.max()):.3e}, over by {worst:.3e}"
                own_plan = ops.attn_plan(n, 1, S, H, Dh, inject, dtype=dtype, no_split=no_split)
                assert not _same_form(plan, own_plan), (plan, own_plan)
            print(f"cfg2 level 0, R = {R}, inject={inject}, no_split={no_split}: plan {plan}, every frame within the bound of its own call")


# -------------------------------------------------------------------------------------------------------------- hooks
def _hook_pipe():
    cfg = gc.BLOCKS_CFG
    torch.manual_seed(cfg["seed"])
    pipe = fd.FakePipeline(dims=cfg["dims"], heads=cfg["heads"], cross_dim=cfg["cross_dim"]).eval().cuda()
    tfu.register_extended_attention_pnp(pipe, [801])
    tfu.set_tokenflow(pipe.unet)
    tfu.register_time(pipe, 801)
    return pipe


@pytest.mark.parametrize("fp32_as", DTYPES)
@pytest.mark.parametrize("no_split", [True, False])
def test_hooks_bank_window(monkeypatch, fp32_as, no_split):
    """One block (it injects at this step) through `register_bank_window(pipe, 1)`: the attention of its pivotal pass against the
    oracle, frame by frame on the window's slices (the spy); the pass differs from the whole-bank pass, a covering radius
    reproduces the whole-bank pass bit for bit, and the chunk passes run as they always do."""
    ops = _ops()
    monkeypatch.setattr(ops, "FP32_AS", fp32_as)
    monkeypatch.setattr(ops, "NO_SPLIT", no_split)
    K, n, S, R = 5, 2, 48, 1
    checked = []
    real = ops.ext_attn_windows

    def spy(q, k, v, heads, scale, inject, windows, **kw):
        out = real(q, k, v, heads, scale, inject, windows, **kw)
        qc, kc, vc = (t.float().cpu().contiguous() for t in (q, k, v))
        refs = _frame_refs(qc, kc, vc, K, windows, heads, scale, inject)
        for i in range(K):
            assert_attn_close(_win(out, K, i, i + 1), refs[i], f"hooks frame {i}", dtype=q.dtype)
        checked.append((tuple(windows), bool(inject), q.dtype))
        return out
    monkeypatch.setattr(ops, "ext_attn_windows", spy)

    def run(pipe):
        blk = pipe.unet.up_blocks[2].attentions[0].transformer_blocks[0]
        D, cross = blk.norm1.normalized_shape[0], gc.BLOCKS_CFG["cross_dim"]
        g = torch.Generator().manual_seed(11)
        x_piv, enc_piv = torch.randn(3 * K, S, D, generator=g).cuda(), torch.randn(3 * K, 7, cross, generator=g).cuda()
        x_ch, enc_ch = torch.randn(3 * K * n, S, D, generator=g).cuda(), torch.randn(3 * K * n, 7, cross, generator=g).cuda()
        with torch.no_grad():
            tfu.register_pivotal(pipe, True)
            piv = blk(x_piv, encoder_hidden_states=enc_piv)
            tfu.register_pivotal(pipe, False)
            tfu.register_batch_idx(pipe, range(K))
            chunks = blk(x_ch, encoder_hidden_states=enc_ch)
        return piv.float(), chunks.float()

    pipe = _hook_pipe()
    tfu.register_bank_window(pipe, R)
    win_piv, win_chunks = run(pipe)
    assert checked == [(tuple(ops.bank_windows(K, R)), True, fp32_as)]
    assert torch.isfinite(win_piv).all() and torch.isfinite(win_chunks).all()
    full_piv, full_chunks = run(_hook_pipe())
    assert not torch.equal(win_piv, full_piv)                  # an opt-in that changes the result
    pipe = _hook_pipe()
    tfu.register_bank_window(pipe, K - 1)                      # ... and is the reference computation at a covering radius
    cov_piv, cov_chunks = run(pipe)
    assert len(checked) == 1
    assert torch.equal(cov_piv, full_piv) and torch.equal(cov_chunks, full_chunks)
