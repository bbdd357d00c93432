"""Frame-set keyframe bank on the GPU (tf_ext_attn_fwd_frame_sets, hooks.register_bank_window(anchors=...)): the uncond / cond
branches of keyframe i attend to the keys of the bank frames whose bits are set in mask i, in ascending frame order.

  * q, k, v are independent per frame, so a launch that read a frame outside the set -- a skipped frame between two members,
    say -- or missed a member lands O(1) off.  Every frame is held to the oracle on the GATHERED slices of its members, within
    the attention bound of tests/test_kernels_gpu.py, on N(0,1) and on peaked inputs, with 16-bit and fp32 output, in the
    default mode (small grids split the member list into runs; a set shorter than the split leaves empty runs) and under
    no_split.
  * Frame i's OWN CALL is `ops.ext_attn` on the gathered tensors with Kq = 1, q_frame0 = the rank of frame i among its members.
    Under no_split the frame-set call is bit-identical to it wherever the two plans name the same kernel form (asserted as a
    precondition with the plan functions; the tables hold largest sets of 4 and 5 frames and own calls of 1 to 5, the sizes at
    which tests/test_windows_gpu.py establishes it).
  * planted keys in an anchor and in a skipped frame, contiguous and full sets against the existing calls, a mid-size
    GPU-vs-GPU case, one block through `register_bank_window(pipe, 1, anchors=[0])`."""
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


def mask(*frames):
    m = 0
    for f in frames:
        m |= 1 << f
    return m


def members(m):
    return [j for j in range(64) if (m >> j) & 1]


TABLES = {
    "R1+a0": [mask(0, 1), mask(0, 1, 2), mask(0, 1, 2, 3), mask(0, 2, 3, 4), mask(0, 3, 4, 5), mask(0, 4, 5)],
    "R1+a0a5": [mask(0, 1, 5), mask(0, 1, 2, 5), mask(0, 1, 2, 3, 5), mask(0, 2, 3, 4, 5), mask(0, 3, 4, 5), mask(0, 4, 5)],
    # one-frame sets (empty runs at nseg = 4), skips of 2 and 3 frames, the own frame first, in the middle or last
    "scattered": [mask(0), mask(1, 3, 5), mask(0, 2, 4), mask(0, 3), mask(1, 2, 4, 5), mask(0, 5)],
}

# (S, H, Dh, kwargs, form of the frame-set launch under no_split): the cases of tests/test_windows_gpu.py
ATTN_CASES = [
    (48, 2, 40, {}, "fused"),                                                      # ragged S
    (192, 2, 160, {}, "fused"),
    (320, 2, 64, {"fused": False}, "one<64"),                                      # one-tile streaming, ragged
    (512, 2, 40, {"fused": False, "hints": _lib.TF_ATTN_HINT_MIX}, "il<40"),       # interleaved (DUAL under injection)
    (576, 2, 64, {"fused": False}, "il<64"),                                       # interleaved, LDS-DMA staged
    (520, 2, 64, {"fused": False}, "pp<64"),                                       # ping-pong: ragged S >= 512, one pass
    (320, 2, 80, {}, "il<80"),                                                     # Dh 80: fused in the default mode on this grid
    (128, 2, 160, {"fused": False}, "one<160"),                                    # Dh 160 streams in the ALL form under injection too
]


def _ops():
    from tokenflow_amd import ops
    return ops


def _rnd(x, dtype):
    return x.to(dtype).float()


def _attn_inputs(K, S, D, kind, seed):
    """Independent q, k, v for every frame.  peaked: planted keys of gain 12 inside every frame, many in its last 64-key tile
    (the family of tests/test_windows_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(3 * K, S, D, generator=g) for _ in range(3))
    if kind == "peaked":
        s_ = torch.arange(0, S, 5)
        k[:, (s_ * 3 + S - 60) % S] = q[:, s_] * 12.0
    return q, k, v


def _gather(t, K, frames):
    """[3K, S, D] -> the frames `frames` of every branch next to each other, [3 len(frames), S, D]."""
    idx = torch.as_tensor(list(frames), device=t.device)
    return t.view(3, K, *t.shape[1:])[:, idx].reshape(3 * len(frames), *t.shape[1:]).contiguous()


def _frame_refs(q, k, v, K, sets, H, scale, inject):
    """Per frame: the oracle on the gathered slices of its members, frame i's rows -- (ref, softmax.|V|) as [3, S, D] each."""
    refs = []
    for i, m in enumerate(sets):
        fr = members(m)
        r, ra, _ = attn_ref(_gather(q, K, fr), _gather(k, K, fr), _gather(v, K, fr), H, scale, inject, need_sigma=False)
        pick = lambda t: t.view(3, len(fr), *t.shape[1:])[:, fr.index(i)]      # noqa: E731
        refs.append((pick(r), pick(ra), None))
    return refs


def _own_call(ops, dq, dk, dv, K, i, m, H, scale, inject, **kw):
    fr = members(m)
    return ops.ext_attn(_gather(dq, K, [i]), _gather(dk, K, fr), _gather(dv, K, fr), H, scale, inject, q_frame0=fr.index(i), **kw)


def _same_form(set_plan, own_plan):
    """The two plans name the same kernel form: the same launches but for the ',set' mark; fused launches agree in what their
    arithmetic depends on (KW and PREC: include/tokenflow_hip.h), whatever their query waves."""
    strip = lambda p: [re.sub(r"qw=\d,", "", t.replace(",set", "")) for t in p]      # noqa: E731
    return strip(set_plan) == strip(own_plan)


@pytest.mark.parametrize("S,H,Dh,kw,form", ATTN_CASES, ids=[f"S{c[0]}-Dh{c[2]}-{c[4].strip('<')}" for c in ATTN_CASES])
@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_frame_sets(S, H, Dh, kw, form, table, inject, dtype):
    ops = _ops()
    K, sets = K_ATTN, TABLES[table]
    D, scale = H * Dh, Dh ** -0.5
    plans = {ns: ops.attn_frame_sets_plan(K, sets, S, H, Dh, inject, dtype=dtype, no_split=ns, **kw) for ns in (False, True)}
    # the case is what its name says: one frame-set launch of the named form under no_split, one pre-pass unless it is fused
    marked = [t for t in plans[True] if t.endswith(",set") or t.endswith(",set]")]
    want = "one<64" if inject and form == "pp<64" else form      # (injection at Dh 64, ragged S: the DUAL one-tile form)
    assert len(marked) == 1 and marked[0].startswith(want), plans[True]
    assert all(p.count("vt_pack") == (0 if p[0].startswith("fused") else 1) for p in plans.values()), plans
    if table == "scattered" and not plans[False][0].startswith("fused") and Dh != 160:      # (4 tiles at Dh 160, S 128: no split)
        assert any(t.startswith("merge[nseg=4]") for t in plans[False]), plans[False]      # empty runs: sets of 1, 2 and 3 frames
    n_equal = 0
    for kind in ("randn", "peaked"):
        q, k, v = (_rnd(t, dtype) for t in _attn_inputs(K, S, D, kind, seed=S + Dh + len(kind)))
        dq, dk, dv = (t.to(dtype).cuda() for t in (q, k, v))
        refs = _frame_refs(q, k, v, K, sets, H, scale, inject)
        for no_split in (False, True):
            got = ops.ext_attn_frame_sets(dq, dk, dv, H, scale, inject, sets, no_split=no_split, **kw)
            assert torch.isfinite(got.float()).all()
            got32 = ops.ext_attn_frame_sets(dq, dk, dv, H, scale, inject, sets, no_split=no_split, out_dtype=torch.float32, **kw)
            assert got32.dtype == torch.float32 and torch.equal(got32.to(dtype), got)
            for i, m in enumerate(sets):
                what = f"S{S} Dh{Dh} {table} inject={inject} no_split={no_split} {kind} {dtype} frame {i} set {members(m)}"
                err = assert_attn_close(_gather(got, K, [i]), refs[i], what, dtype=dtype)
                assert_attn_close(_gather(got32, K, [i]), refs[i], what + " fp32 out", dtype=dtype)
                if not no_split:
                    continue
                own_plan = ops.attn_plan(len(members(m)), 1, S, H, Dh, inject, dtype=dtype, no_split=True, **kw)
                same_form = _same_form(plans[True], own_plan)
                alone = _own_call(ops, dq, dk, dv, K, i, m, H, scale, inject, no_split=True, **kw)
                same = torch.equal(_gather(got, K, [i]), alone)
                print(f"{what}: max abs err {err:.3e}, same form as its own call: {same_form}, equal to it: {same}")
                assert same_form, (plans[True], own_plan)      # the tables are chosen so that the precondition holds
                assert same, what
                n_equal += 1
    assert n_equal == 2 * K


def test_contiguous_and_full_sets_are_the_existing_calls():
    ops = _ops()
    K = K_ATTN
    for S, H, Dh, kw in ((64, 2, 40, {}), (320, 2, 64, {"fused": False}), (512, 2, 40, {"fused": False})):
        q, k, v = (t.bfloat16().cuda() for t in _attn_inputs(K, S, H * Dh, "randn", 3))
        for inject in (False, True):
            for windows in (ops.bank_windows(K, 1), ops.bank_windows(K, 2), [(0, 1), (0, 3), (1, 4), (3, 1), (2, 4), (4, 2)]):
                sets = [((1 << n) - 1) << lo for lo, n in windows]
                for no_split in (False, True):
                    assert torch.equal(ops.ext_attn_frame_sets(q, k, v, H, Dh ** -0.5, inject, sets, no_split=no_split, **kw),
                                       ops.ext_attn_windows(q, k, v, H, Dh ** -0.5, inject, windows, no_split=no_split, **kw))
            assert torch.equal(ops.ext_attn_frame_sets(q, k, v, H, Dh ** -0.5, inject, [mask(*range(K))] * K, **kw),
                               ops.ext_attn(q, k, v, H, Dh ** -0.5, inject, **kw))
            assert torch.equal(ops.ext_attn_frame_sets(q, k, v, H, Dh ** -0.5, inject, ops.bank_frame_sets(K, K + 2, [1]), **kw),
                               ops.ext_attn(q, k, v, H, Dh ** -0.5, inject, **kw))
    with pytest.raises(ValueError):
        ops.ext_attn_frame_sets(q, k, v, H, Dh ** -0.5, True, ops.bank_frame_sets(K - 1, 1, [0]))
    with pytest.raises(ValueError, match="own frame"):
        ops.ext_attn_frame_sets(q, k, v, H, Dh ** -0.5, True, [mask(0, 2)] * K)
    with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_fwd_frame_sets"):
        ops.ext_attn_frame_sets(q, k, v, H, Dh ** -0.5, True, TABLES["R1+a0"], hints=_lib.TF_ATTN_MULTI_V)


@pytest.mark.parametrize("S,H,Dh,kw", [(48, 2, 40, {}), (320, 2, 64, {"fused": False}),
                                      (512, 2, 40, {"fused": False, "hints": _lib.TF_ATTN_HINT_MIX})],
                         ids=["fused", "one", "il"])
@pytest.mark.parametrize("inject", [False, True])
def test_planted_key_in_the_anchor_and_in_a_skipped_frame(S, H, Dh, kw, inject):
    """Query frame 4 of R1+a0 has the set {0, 3, 4, 5}.  A gain-12 match for its queries placed in anchor frame 0 must dominate
    the output: the value planted beside it comes out.  The same match in frame 1 or 2 -- the frames its cursors skip -- must
    leave no trace, bit for bit the unplanted result, while it does change a frame whose set holds that frame."""
    ops = _ops()
    K, f, D, scale = K_ATTN, 4, H * Dh, Dh ** -0.5
    sets = TABLES["R1+a0"]
    assert members(sets[f]) == [0, 3, 4, 5]
    q, k, v = (_rnd(t, torch.bfloat16) for t in _attn_inputs(K, S, D, "randn", seed=19))
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
        run = lambda kk, vv: ops.ext_attn_frame_sets(dq, kk.bfloat16().cuda(), vv.bfloat16().cuda(), H, scale, inject, sets,   # noqa: E731
                                                     no_split=no_split, **kw).float().view(3, K, S, D)
        base = run(k, v)
        anchor = run(*planted(0))
        for b in (1, 2):
            # logit of the match: 12 |q|^2 scale ~ 12 sqrt(Dh) >= 75 above the N(0, 1) scores of <= 2100 other keys
            assert torch.allclose(anchor[b, f, rows], torch.full_like(anchor[b, f, rows], 100.0 + b), rtol=2.0 ** -7), (b, no_split)
            assert not torch.allclose(base[b, f, rows], anchor[b, f, rows], rtol=0.5)
        for skipped, holder in ((1, 2), (2, 3)):      # sets[2] = {0,1,2,3} holds frame 1, sets[3] = {0,2,3,4} holds frame 2
            assert (sets[holder] >> skipped) & 1 and not (sets[f] >> skipped) & 1
            outside = run(*planted(skipped))
            # frame 4 sees nothing of the skipped frame (with injection its source keys were overwritten too: frame 4's own source
            # branch reads frame 4 only)
            assert torch.equal(outside[:, f], base[:, f]), (skipped, no_split)
            assert not torch.equal(outside[1, holder], base[1, holder]), (skipped, no_split)


def test_midsize_against_the_frames_own_calls():
    """BASELINE config 2, level 0: K = 8, S = 1024, H = 8, Dh = 40, radius 2 with anchor 0 -- no CPU oracle at this size; every
    frame against its own call on the GPU (gathered members, Kq = 1), within the attention bound of it (reference and
    softmax.|V| from own calls, the latter on |v|), in the default mode and under no_split.  Only the BOUND is checked at this
    size: the own calls have an eighth of the grid and need not take the kernel form of the 8-frame launch."""
    ops = _ops()
    K, S, H, Dh, R = 8, 1024, 8, 40, 2
    D, scale, dtype = H * Dh, Dh ** -0.5, torch.bfloat16
    sets = ops.bank_frame_sets(K, R, [0])
    assert members(sets[5]) == [0, 3, 4, 5, 6, 7] and max(len(members(m)) for m in sets) == 6
    g = torch.Generator(device="cuda").manual_seed(5)
    dq, dk, dv = (torch.randn(3 * K, S, D, generator=g, device="cuda").to(dtype) for _ in range(3))
    for inject in (False, True):
        for no_split in (False, True):
            plan = ops.attn_frame_sets_plan(K, sets, S, H, Dh, inject, dtype=dtype, no_split=no_split)
            assert plan[0] == "vt_pack" and plan[1].startswith("il<40") and plan[1].endswith(",set"), plan
            got = ops.ext_attn_frame_sets(dq, dk, dv, H, scale, inject, sets, no_split=no_split)
            for i, m in enumerate(sets):
                own = _own_call(ops, dq, dk, dv, K, i, m, H, scale, inject, no_split=no_split, out_dtype=torch.float32)
                own_abs = _own_call(ops, dq, dk, dv.abs(), K, i, m, H, scale, inject, no_split=no_split, out_dtype=torch.float32)
                err = (_gather(got, K, [i]).float() - own).abs()
                worst = float((err - attn_bound(own, own_abs, dtype)).max())
                assert worst <= 0, f"frame {i} inject={inject} no_split={no_split}: max abs err {float(err.max()):.3e}, over by {worst:.3e}"
            print(f"cfg2 level 0, R = {R} + anchor 0, inject={inject}, no_split={no_split}: plan {plan}, every frame within the "
                  "bound of its own call")


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
def test_hooks_bank_window_anchors(monkeypatch, fp32_as, no_split):
    """One block (it injects at this step) through `register_bank_window(pipe, 1, anchors=[0])`: the attention of its pivotal
    pass against the oracle, frame by frame on the gathered members (the spy); the pass differs from the plain radius-1 pass
    and from the whole-bank pass, a covering radius reproduces the whole-bank pass bit for bit whatever the anchors, and
    anchors=None issues `ops.ext_attn_windows` as before."""
    ops = _ops()
    monkeypatch.setattr(ops, "FP32_AS", fp32_as)
    monkeypatch.setattr(ops, "NO_SPLIT", no_split)
    K, n, S, R = 5, 2, 48, 1
    checked, windowed = [], []
    real, real_win = ops.ext_attn_frame_sets, ops.ext_attn_windows

    def spy(q, k, v, heads, scale, inject, sets, **kw):
        out = real(q, k, v, heads, scale, inject, sets, **kw)
        qc, kc, vc = (t.float().cpu().contiguous() for t in (q, k, v))
        refs = _frame_refs(qc, kc, vc, K, sets, heads, scale, inject)
        for i in range(K):
            assert_attn_close(_gather(out, K, [i]), refs[i], f"hooks frame {i}", dtype=q.dtype)
        checked.append((tuple(sets), bool(inject), q.dtype))
        return out

    def spy_win(q, k, v, heads, scale, inject, windows, **kw):
        windowed.append(tuple(windows))
        return real_win(q, k, v, heads, scale, inject, windows, **kw)
    monkeypatch.setattr(ops, "ext_attn_frame_sets", spy)
    monkeypatch.setattr(ops, "ext_attn_windows", spy_win)

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
    tfu.register_bank_window(pipe, R, anchors=[0])
    anc_piv, anc_chunks = run(pipe)
    assert checked == [(tuple(ops.bank_frame_sets(K, R, [0])), True, fp32_as)] and not windowed
    assert torch.isfinite(anc_piv).all() and torch.isfinite(anc_chunks).all()
    pipe = _hook_pipe()
    tfu.register_bank_window(pipe, R, anchors=None)            # no anchors: the windowed op, as before
    win_piv, _ = run(pipe)
    assert windowed == [tuple(ops.bank_windows(K, R))] and len(checked) == 1
    full_piv, full_chunks = run(_hook_pipe())
    assert not torch.equal(anc_piv, win_piv) and not torch.equal(anc_piv, full_piv)      # an opt-in that changes the result
    pipe = _hook_pipe()
    tfu.register_bank_window(pipe, K - 1, anchors=[0, 2])      # ... and is the reference computation at a covering radius
    cov_piv, cov_chunks = run(pipe)
    assert len(checked) == 1 and len(windowed) == 1
    assert torch.equal(cov_piv, full_piv) and torch.equal(cov_chunks, full_chunks)
