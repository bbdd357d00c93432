"""The bank part of a windowed / frame-set MULTI-EDIT pass on the GPU: `ops.ext_attn_windows_edits_views` and
`ops.ext_attn_frame_sets_edits_views` (tf_ext_attn_fwd_windows_edits_part / tf_ext_attn_fwd_frame_sets_edits_part).

  * every edit's bank branches BIT-IDENTICAL to the existing single-edit part call (`ext_attn_windows_views` /
    `ext_attn_frame_sets_views`) on [source | uncond_e | cond_e] with inject = bit e of the mask, under no_split with the
    four-bank form off -- dense and compact q / k on the same values, the source slab of `out` untouched, the source slab of v
    absent.  S = 64 is the fused regime: ONE launch whose token carries 'sets=E,win' / 'sets=E,set' (checked first), equal to
    the E one-set launches; S = 320 the streaming regime.  No case is left out: the tokens of both sides are asserted equal
    (apart from the joint launch) before the bits are compared;
  * the composition bank part + source part == `ext_attn_windows_edits` / `ext_attn_frame_sets_edits(no_split, multi_v=False)`;
  * canonical forms: E = 1, range sets, whole-bank tables, part "all";
  * planted keys: a dominant key at the window edge (found by the one edit that holds it), one just outside (found by nobody),
    one in the anchor frame;
  * default mode and the forced four-bank form: every edit within `attn_bound` of `attn_ref` on its gathered member frames;
  * `ops.edit_halo_pack` against torch indexing;
  * sharded worlds of 2 (K = 5) and 3 (K = 7) ranks sharing cuda:0 over gloo, and K = 66 over 3: `FrameShard(window_edits=True)`
    and `NativeEditShard` against the EXISTING single-edit windowed / anchored shard pass per edit (I1, no case left out), the
    one-process composition (I2), the canonical forms (I4) and each other (I5); `attn_split` / the four-bank opt-in held to the
    bound (I6); a two-rank hooks pass with two edits and per-edit schedules.
q, k and v are independent per branch and per frame: a launch that read another slot, another edit's bank, another window entry
or another query frame lands O(1) off."""
import pytest
import torch

from tests.test_kernels_gpu import attn_bound, attn_ref
from tests.test_shard_window_gpu import CASES

pytestmark = pytest.mark.gpu

POISON = 7.0
K, KQ, F0 = 7, 3, 2
# the shapes of tests/test_shard_window_gpu.py (its inject flag is the mask here) plus head dim 160 in the fused regime
SHAPES = sorted({(S, H, Dh, dt) for S, H, Dh, _, dt in CASES} | {(64, 1, 160, torch.bfloat16)}, key=str)
EDITS = [(2, 0b00), (2, 0b11), (2, 0b01), (3, 0b00), (3, 0b11), (3, 0b01), (3, 0b101)]
IDS = [f"S{s[0]}-H{s[1]}-Dh{s[2]}-{str(s[3]).replace('torch.', '')}" for s in SHAPES]


def _ops():
    from tokenflow_amd import ops
    return ops


def _inputs(E, S, D, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return tuple(torch.randn(1 + 2 * E, K, S, D, generator=g, device="cuda").to(dtype) for _ in range(3))


def _compact(t, mask, E):
    """[source | the (uncond, cond) slots of the edits that do not inject, ascending]"""
    keep = [0] + [b for e in range(E) if not (mask >> e) & 1 for b in (1 + 2 * e, 2 + 2 * e)]
    return t[keep].contiguous()


def _tables(ops, kind):
    """(the table of query frames F0 .. F0 + KQ, the whole bank's table): radius 1, frame sets with anchors 0 and 6."""
    whole = ops.bank_windows(K, 1) if kind == "win" else ops.bank_frame_sets(K, 1, (0, 6))
    return whole[F0:F0 + KQ], whole


def _members(kind, entry):
    if kind == "win":
        return list(range(entry[0], entry[0] + entry[1]))
    return [j for j in range(K) if (entry >> j) & 1]


def _single(ops, kind):
    return ((ops.ext_attn_windows_views, ops.attn_windows_part_plan) if kind == "win"
            else (ops.ext_attn_frame_sets_views, ops.attn_frame_sets_part_plan))


def _multi(ops, kind):
    return ((ops.ext_attn_windows_edits_views, ops.attn_windows_edits_part_plan) if kind == "win"
            else (ops.ext_attn_frame_sets_edits_views, ops.attn_frame_sets_edits_part_plan))


def _per_edit_reference(ops, kind, tab, q, k, v, h, d, mask, E, **kw):
    """Every edit's bank branches through the EXISTING single-edit part call with its own flag; the source slab stays poisoned."""
    B, _, S, D = k.shape
    view, _ = _single(ops, kind)
    qf = q[:, F0:F0 + KQ]
    ref = torch.full((B, KQ, S, D), POISON, dtype=q.dtype, device=q.device)
    for e in range(E):
        lo = 1 + 2 * e
        if (mask >> e) & 1:
            view(qf[0:1], k[0:1], v[lo:lo + 2], ref[lo:lo + 2], h, d ** -0.5, True, tab, "bank", branch0=(0, 0, 1, 1),
                 q_frame0=F0, **kw)
        else:
            view(qf[lo:lo + 2], k[lo:lo + 2], v[lo:lo + 2], ref[lo:lo + 2], h, d ** -0.5, False, tab, "bank",
                 branch0=(1, 1, 1, 1), q_frame0=F0, **kw)
    return ref


def _bank_part(ops, kind, tab, q, k, v, h, d, mask, E, compact, **kw):
    """The bank part of all edits in one call; q / k hold only the slots the part reads."""
    B, _, S, D = k.shape
    view, _ = _multi(ops, kind)
    qq, kk = (_compact(t, mask, E) if compact else t for t in (q, k))
    qf = qq[:, F0:F0 + KQ]
    out = torch.full((B, KQ, S, D), POISON, dtype=q.dtype, device=q.device)
    if mask == 0:                       # no launch reads slot 0 of q / k: it need not exist
        view(qf[1:], kk[1:], v[1:], out[1:], h, d ** -0.5, E, mask, tab, "bank", compact, branch0=(1, 1, 1, 1), q_frame0=F0, **kw)
    elif mask == (1 << E) - 1:          # ... and nothing but slot 0 here
        view(qf[0:1], kk[0:1], v[1:], out[1:], h, d ** -0.5, E, mask, tab, "bank", compact, branch0=(0, 0, 1, 1), q_frame0=F0,
             **kw)
    else:
        view(qf, kk, v[1:], out, h, d ** -0.5, E, mask, tab, "bank", compact, branch0=(0, 0, 1, 0), q_frame0=F0, **kw)
    return out


def _expected_tokens(ops, kind, tab, S, h, d, mask, E, dtype):
    """The tokens the multi-edit part must name, built from the single-edit part plans: S <= 256 ONE joint launch; above, ONE
    pre-pass, then every injecting edit's launches, then the others'."""
    _, plan1 = _single(ops, kind)
    one = {inj: plan1(K, KQ, F0, tab, S, h, d, inj, dtype=dtype, no_split=True) for inj in (False, True)}
    if S <= 256:
        for p in one.values():
            assert len(p) == 1 and p[0].startswith("fused[") and p[0].endswith(f",{kind}]"), p
        assert one[False] == one[True]
        return [one[True][0].replace(f",{kind}]", f",sets={E},{kind}]")]
    n_inj = bin(mask).count("1")
    body = {inj: [t for t in p if t != "vt_pack"] for inj, p in one.items()}
    return ["vt_pack"] + body[True] * n_inj + body[False] * (E - n_inj)


@pytest.mark.parametrize("kind", ["win", "set"])
@pytest.mark.parametrize("S,H,Dh,dtype", SHAPES, ids=IDS)
def test_bank_part_equals_the_single_edit_part_calls(S, H, Dh, dtype, kind):
    """I1 / I3 in one process: K = 7 bank frames, the rank's Kq = 3 query frames from frame 2 on."""
    ops = _ops()
    tab, _ = _tables(ops, kind)
    _, plan_n = _multi(ops, kind)
    compared = 0
    for E, mask in EDITS:
        q, k, v = _inputs(E, S, H * Dh, dtype, seed=S + Dh + E)
        what = f"{kind} S{S} H{H} Dh{Dh} E{E} mask {mask:#b} {dtype}"
        want = _expected_tokens(ops, kind, tab, S, H, Dh, mask, E, dtype)
        for compact in (False, True):
            got = plan_n(K, KQ, F0, tab, S, H, Dh, E, mask, "bank", compact, dtype=dtype, no_split=True, multi_v=False)
            assert got == want, (what, compact, got, want)
        ref = _per_edit_reference(ops, kind, tab, q, k, v, H, Dh, mask, E, no_split=True)
        assert not bool((ref[1:] == POISON).any())
        for compact in (False, True):
            out = _bank_part(ops, kind, tab, q, k, v, H, Dh, mask, E, compact, no_split=True, multi_v=False)
            assert torch.equal(out[1:], ref[1:]), f"{what} compact {compact}: bank part"
            assert bool((out[0] == POISON).all()), f"{what} compact {compact}: the bank part wrote the source slab"
            compared += 1
    assert compared == 2 * len(EDITS)      # no case left out


@pytest.mark.parametrize("kind", ["win", "set"])
@pytest.mark.parametrize("S,H,Dh", [(64, 2, 40), (64, 2, 64), (320, 2, 40), (320, 1, 80)])
def test_parts_compose_to_the_multi_edit_call(S, H, Dh, kind):
    """I2 at K <= 64: bank part + source-only edits part on the full tensors == `ext_attn_windows_edits` /
    `ext_attn_frame_sets_edits(no_split=True, multi_v=False)`, whose per-edit launches name the same forms (asserted)."""
    ops = _ops()
    dtype = torch.bfloat16
    _, whole = _tables(ops, kind)
    view, plan_n = _multi(ops, kind)
    full, full_plan = ((ops.ext_attn_windows_edits, ops.attn_windows_edits_plan) if kind == "win"
                       else (ops.ext_attn_frame_sets_edits, ops.attn_frame_sets_edits_plan))
    strip = lambda plan: [t.replace(f",sets={E}", "") for t in plan]      # noqa: E731
    for E, mask in [(2, 0b01), (3, 0b101), (2, 0b11)]:
        q, k, v = _inputs(E, S, H * Dh, dtype, seed=S + Dh + E + 1)
        D = H * Dh
        bank = plan_n(K, K, 0, whole, S, H, Dh, E, mask, "bank", dtype=dtype, no_split=True, multi_v=False)
        src = ops.attn_edits_part_plan(K, K, S, H, Dh, E, mask, part="source", dtype=dtype, no_split=True)
        call = full_plan(K, whole, S, H, Dh, E, mask, dtype=dtype, no_split=True, multi_v=False)
        if S <= 256:      # the call: E one-set launches + the source launch; the parts: ONE joint launch + the source launch
            assert len(bank) == 1 and call == strip(bank) * E + src, (bank, src, call)
        else:             # (each part call packs the V^T image of the branches it streams: one pre-pass each)
            body = lambda plan: [t for t in plan if t != "vt_pack"]      # noqa: E731
            assert body(call) == body(bank) + body(src), (bank, src, call)
        out = torch.full_like(q, POISON)
        view(q, k, v[1:], out, H, Dh ** -0.5, E, mask, whole, "bank", branch0=(0, 0, 1, 0), no_split=True, multi_v=False)
        ops.ext_attn_edits_views(q[0:1], k[0:1], v[0:1], out[0:1], H, Dh ** -0.5, E, mask, "source", no_split=True)
        B = 1 + 2 * E
        want = full(q.view(B * K, S, D), k.view(B * K, S, D), v.view(B * K, S, D), H, Dh ** -0.5, False, E, whole,
                    inject_mask=mask, no_split=True, multi_v=False)
        assert torch.equal(out.view(B * K, S, D), want), (kind, S, Dh, E, mask)
        # part "all" IS the multi-edit call
        both = torch.full_like(q, POISON)
        view(q, k, v, both, H, Dh ** -0.5, E, mask, whole, "all", no_split=True, multi_v=False)
        assert torch.equal(both.view(B * K, S, D), want)
        assert plan_n(K, K, 0, whole, S, H, Dh, E, mask, "all", dtype=dtype, no_split=True, multi_v=False) == call


@pytest.mark.parametrize("S,H,Dh", [(64, 2, 40), (320, 2, 64)])
def test_canonical_forms(S, H, Dh):
    """I4 for the part entry points: E = 1, range sets and whole-bank tables give the parent call's bits and tokens."""
    ops = _ops()
    dtype, scale = torch.bfloat16, Dh ** -0.5
    kw = dict(no_split=True, multi_v=False)
    win, _ = _tables(ops, "win")
    sets, _ = _tables(ops, "set")
    ranges = [((1 << n) - 1) << lo for lo, n in win]
    full_w, full_s = [(0, K)] * KQ, [(1 << K) - 1] * KQ
    # E = 1: the single-edit part
    q, k, v = _inputs(1, S, H * Dh, dtype, seed=3)
    for kind, tab in (("win", win), ("set", sets)):
        view1, plan1 = _single(ops, kind)
        view, plan_n = _multi(ops, kind)
        for mask in (0, 1):
            assert (plan_n(K, KQ, F0, tab, S, H, Dh, 1, mask, "bank", dtype=dtype, no_split=True)
                    == plan1(K, KQ, F0, tab, S, H, Dh, bool(mask), dtype=dtype, no_split=True))
            kb, b0 = (k[0:1], (0, 0, 1, 0)) if mask else (k[1:3], (0, 1, 1, 0))
            a, b = (torch.full((3, KQ, S, H * Dh), POISON, dtype=dtype, device="cuda") for _ in range(2))
            view(q[:, F0:F0 + KQ], kb, v[1:3], a, H, scale, 1, mask, tab, "bank", branch0=b0, q_frame0=F0, no_split=True)
            view1(q[:, F0:F0 + KQ], kb, v[1:3], b, H, scale, bool(mask), tab, "bank", branch0=b0, q_frame0=F0, no_split=True)
            assert torch.equal(a, b) and not bool((a[1:] == POISON).any())
    # range sets ARE the windowed part; whole-bank tables ARE the edits part
    E, mask = 2, 0b01
    q, k, v = _inputs(E, S, H * Dh, dtype, seed=4)
    a = _bank_part(ops, "set", ranges, q, k, v, H, Dh, mask, E, True, **kw)
    b = _bank_part(ops, "win", win, q, k, v, H, Dh, mask, E, True, **kw)
    assert torch.equal(a, b)
    assert (ops.attn_frame_sets_edits_part_plan(K, KQ, F0, ranges, S, H, Dh, E, mask, dtype=dtype, **kw)
            == ops.attn_windows_edits_part_plan(K, KQ, F0, win, S, H, Dh, E, mask, dtype=dtype, **kw))
    want = torch.full_like(a, POISON)
    ops.ext_attn_edits_views(q[:, F0:F0 + KQ], k, v[1:], want, H, scale, E, mask, "bank", branch0=(0, 0, 1, 0), q_frame0=F0, **kw)
    for kind, tab in (("win", full_w), ("set", full_s)):
        assert torch.equal(_bank_part(ops, kind, tab, q, k, v, H, Dh, mask, E, False, **kw), want), kind
        assert (_multi(ops, kind)[1](K, KQ, F0, tab, S, H, Dh, E, mask, dtype=dtype, **kw)
                == ops.attn_edits_part_plan(K, KQ, S, H, Dh, E, mask, part="bank", dtype=dtype, **kw))


@pytest.mark.parametrize("S", [64, 320], ids=["fused", "streaming"])
@pytest.mark.parametrize("kind", ["win", "set"])
def test_planted_keys(kind, S):
    """Query (frame 3, token 5), radius 1: window [2, 4]; with sets, anchors 0 and 6 beside it.  Only edit 1's k holds the
    query's own vector times 12 at the window edge (frame 4, token 9; value -3): edit 1 returns -3 there, edit 0 and edit 2 do
    not.  Every edit's k holds the same dominant key just outside the window (frame 5, value 100): nobody returns 100.  With
    sets edit 2 holds the key in the anchor frame 6 (value 50), outside every window: only the set table finds it."""
    ops = _ops()
    H, Dh, E, mask, dtype = 2, 40, 3, 0b000, torch.bfloat16
    tab, _ = _tables(ops, kind)
    q, k, v = _inputs(E, S, H * Dh, dtype, seed=11)
    f, tok = 3, 5
    for b in range(1, 1 + 2 * E):
        key = (q[b, f, tok].float() * 12).to(dtype)
        k[b, 5, 9], v[b, 5, 9] = key, 100.0                     # outside every table of frame 3
        if b in (3, 4):
            k[b, 4, 9], v[b, 4, 9] = key, -3.0                  # the window edge, edit 1 only
        if b in (5, 6):
            k[b, 6, 9], v[b, 6, 9] = key, 50.0                  # the anchor, edit 2 only
    for compact in (False, True):
        out = _bank_part(ops, kind, tab, q, k, v, H, Dh, mask, E, compact, no_split=True, multi_v=False)
        row = out[:, f - F0, tok].float()
        assert float((row[3:5] + 3.0).abs().max()) < 0.05, (kind, S, row[3:5])
        if kind == "set":
            assert float((row[5:7] - 50.0).abs().max()) < 0.5, (kind, S, row[5:7])
        else:
            assert float(row[5:7].abs().max()) < 3.0, (kind, S, row[5:7])
        assert float(row[1:3].abs().max()) < 3.0 and float(row[1:].abs().max()) < 60.0, (kind, S)      # nobody finds the 100


def _assert_within_bound(ops, kind, tab, got, q, k, v, H, Dh, mask, E, dtype, what):
    """I6: every edit, every query frame, against the oracle on the frame's gathered members with the edit's own flag."""
    _, _, S, D = k.shape
    for e in range(E):
        sl = [0, 1 + 2 * e, 2 + 2 * e]
        for i in range(KQ):
            fr = _members(kind, tab[i])
            q3, k3, v3 = (t[sl][:, fr].reshape(3 * len(fr), S, D).float().cpu() for t in (q, k, v))
            r, ra, _ = attn_ref(q3, k3, v3, H, Dh ** -0.5, bool((mask >> e) & 1), need_sigma=False)
            pick = lambda t: t.view(3, len(fr), S, D)[1:, fr.index(F0 + i)]      # noqa: E731
            err = (got[sl[1:], i].float().cpu() - pick(r)).abs()
            worst = float((err - attn_bound(pick(r), pick(ra), dtype=dtype)).max())
            assert worst <= 0, f"{what} edit {e} frame {F0 + i}: exceeds the attention bound by {worst:.3e}"


@pytest.mark.parametrize("kind", ["win", "set"])
@pytest.mark.parametrize("S,H,Dh,hint,tok", [(64, 2, 40, {}, "fused["), (320, 2, 40, {}, None),
                                              (320, 2, 40, {"multi_v": True}, "one<40,1,4,MV4,2,fq0>"),
                                              (320, 2, 64, {"multi_v64": True}, "one<64,1,8,MV4,2,fq1>")])
def test_default_mode_and_four_bank_form_within_the_bound(S, H, Dh, hint, tok, kind):
    """The split-free-to-choose default mode and the forced four-bank form (a pair of injecting edits shares one softmax; the odd
    edit runs the DUAL launch): held to the oracle's bound only."""
    ops = _ops()
    dtype = torch.bfloat16
    E, mask = (3, 0b111) if hint else (2, 0b01)
    tab, _ = _tables(ops, kind)
    q, k, v = _inputs(E, S, H * Dh, dtype, seed=S + Dh)
    plan = _multi(ops, kind)[1](K, KQ, F0, tab, S, H, Dh, E, mask, "bank", True, dtype=dtype, **hint)
    if tok:
        assert sum(t.startswith(tok) for t in plan) == 1, plan
    out = _bank_part(ops, kind, tab, q, k, v, H, Dh, mask, E, True, **hint)
    assert bool((out[0] == POISON).all())
    _assert_within_bound(ops, kind, tab, out, q, k, v, H, Dh, mask, E, dtype, f"{kind} S{S} Dh{Dh} {hint}")


def test_view_and_argument_errors():
    from tokenflow_amd import _lib
    ops = _ops()
    E, S, H, Dh = 2, 64, 2, 40
    q, k, v = _inputs(E, S, H * Dh, torch.bfloat16, seed=1)
    out = torch.empty_like(q)
    win, sets = ops.bank_windows(K, 1), ops.bank_frame_sets(K, 1, (0,))
    for view, tab, word in ((ops.ext_attn_windows_edits_views, win, "window-free|table-free"),
                            (ops.ext_attn_frame_sets_edits_views, sets, "set-free|table-free")):
        with pytest.raises(ValueError, match=word):      # the source part is table-free
            view(q, k, v, out, H, Dh ** -0.5, E, 0, tab, "source")
        with pytest.raises(ValueError):                  # a mask bit above the edits
            view(q, k, v, out, H, Dh ** -0.5, E, 0b100, tab, "bank")
        with pytest.raises(ValueError):                  # compact q / k with part "all"
            view(q, k, v, out, H, Dh ** -0.5, E, 0b01, tab, "all", True)
        with pytest.raises(ValueError):                  # a table that misses a query frame
            view(q, k, v, out, H, Dh ** -0.5, E, 0, tab[:-1], "bank")
        with pytest.raises(_lib.TokenflowHipError):      # TF_ATTN_FOLD_SCALE has no windowed form (hints pass through)
            view(q, k, v, out, H, Dh ** -0.5, E, 0, tab, "bank", hints=_lib.TF_ATTN_FOLD_SCALE)


# ------------------------------------------------------------------------------------------------------ the pack kernel
def _pack_want(slabs, masks):
    frames = [f for m in masks for f in range(64) if (m >> f) & 1]
    return frames, (torch.stack([torch.stack([s[f] for s in slabs]) for f in frames]) if frames else None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ns", [3, 7, 32])
@pytest.mark.parametrize("nq", [0, 3])
def test_edit_halo_pack(dtype, ns, nq):
    """`ops.edit_halo_pack` against torch indexing: strided slab views (frame stride != S * ld, ld > D), an empty peer, a full
    peer, a frame sent to two and to three peers, a non-contiguous mask; the q staging in the same call."""
    ops = _ops()
    Kl, S, D = 3, 3, 8
    g = torch.Generator().manual_seed(3 + ns)
    buf = torch.randn(ns, Kl + 1, S + 2, 3 * D, generator=g).to(dtype).cuda()
    slabs = [buf[i, :Kl, 1:1 + S, D * (i % 3):D * (i % 3) + D] for i in range(ns)]
    qbuf = torch.randn(3, Kl, S + 1, 2 * D, generator=g).to(dtype).cuda()
    qs = [qbuf[i, :, :S, D:] for i in range(nq)]
    assert slabs[0].stride(0) != S * slabs[0].stride(1) and slabs[0].stride(1) > D
    for masks in ([0b000, 0b111, 0b101], [0b010, 0b010, 0b011, 0b110], [0b100], [0b111] * 5, [0, 0]):
        got, stage = ops.edit_halo_pack(slabs, masks, qs)
        frames, want = _pack_want(slabs, masks)
        assert got.shape == (len(frames), ns, S, D), masks
        assert want is None or torch.equal(got, want), masks
        assert (stage is None) if nq == 0 else torch.equal(stage, torch.stack(qs)), masks
    out = torch.full((3, ns, S, D), 7.0, dtype=dtype, device="cuda")      # into given buffers
    q_out = torch.full((nq, Kl, S, D), 7.0, dtype=dtype, device="cuda") if nq else None
    got, stage = ops.edit_halo_pack(slabs, [0b001, 0b110], qs, out=out, q_out=q_out)
    assert got is out and torch.equal(out, _pack_want(slabs, [1, 6])[1]) and (stage is q_out)
    assert nq == 0 or torch.equal(q_out, torch.stack(qs))


def test_edit_halo_pack_64_frames_large_rows_and_refusals():
    from tokenflow_amd import _lib
    ops = _ops()
    Kl, S, D = 64, 1, 8
    g = torch.Generator().manual_seed(5)
    slabs = [torch.randn(Kl, S, D, generator=g).bfloat16().cuda() for _ in range(4)]
    for masks in ([1 << 63], [(1 << 64) - 1], [1 << 63, (1 << 64) - 1, 0, 1]):
        got, stage = ops.edit_halo_pack(slabs, masks, slabs[:2])
        assert torch.equal(got, _pack_want(slabs, masks)[1]) and torch.equal(stage, torch.stack(slabs[:2])), masks
    # rows of more 16-byte pieces than one workgroup holds: several workgroups per column, each striding over it
    big = [torch.randn(5, 300, 320, generator=g).bfloat16().cuda() for _ in range(3)]
    masks = [0b10110, 0b00001, 0, 0b11111]
    got, stage = ops.edit_halo_pack(big, masks, big[1:])
    assert torch.equal(got, _pack_want(big, masks)[1]) and torch.equal(stage, torch.stack(big[1:]))
    small = [t[:3] for t in slabs]
    with pytest.raises(ValueError):
        ops.edit_halo_pack(small, [0b1000])      # a bit at or above Kl
    with pytest.raises(_lib.TokenflowHipError, match="tf_edit_halo_pack"):
        ops.edit_halo_pack(small * 9, [0b1])      # 36 slabs
    with pytest.raises(_lib.TokenflowHipError, match="tf_edit_halo_pack"):
        ops.edit_halo_pack([t.float() for t in small], [0b1])      # fp32
    mis = torch.zeros(3 * 1 * 16 + 8, dtype=torch.bfloat16, device="cuda")[4:4 + 48].view(3, 1, 16)      # 8 bytes off
    with pytest.raises(_lib.TokenflowHipError, match="aligned"):
        ops.edit_halo_pack([mis], [0b1])


# ------------------------------------------------------------------------------------------------------ sharded worlds
import datetime      # noqa: E402
import os            # noqa: E402
import re            # noqa: E402

import torch.distributed as dist      # noqa: E402
import torch.multiprocessing as mp    # noqa: E402

from tests.nn_families import spread_pivots              # noqa: E402
from tests.test_shard_frame_sets_gpu import CONFIGS      # noqa: E402
from tests.test_sharded_cpu import _free_port            # noqa: E402

TIMEOUT = datetime.timedelta(seconds=60)      # a rank that fails early ends the test instead of hanging its peer
WORLD_EDITS = [(2, 0b01), (2, 0b00), (3, 0b111), (3, 0b101)]
WORLD_SHAPES = [[(64, 2, 40, torch.bfloat16), (320, 2, 64, torch.bfloat16)],
                [(64, 2, 64, torch.bfloat16), (320, 2, 40, torch.bfloat16)],
                [(320, 1, 80, torch.bfloat16), (320, 2, 40, torch.float16)]]


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)


def _norm(plan):
    """Tokens with the marks that do not change a (query, head)'s arithmetic removed: the query waves, the number of sets."""
    return [re.sub(r",sets=\d+", "", re.sub(r"qw=\d,", "", t)) for t in plan]


def _rank_tokens(ops, sharded, K, world, r, R, anchors, S, H, Dh, dtype, E, mask):
    """(the bank tokens of rank r's multi-edit pass, the tokens its E single-edit passes name for the same work)."""
    if R >= K - 1:      # the bank pass of tf_rank_pivotal_edits against tf_rank_pivotal's
        Kl = K // world + (1 if r < K % world else 0)
        multi = ops.attn_edits_part_plan(K, Kl, S, H, Dh, E, mask, part="bank", qk_compact=True, dtype=dtype, no_split=True,
                                         multi_v=False)
        one = {inj: ops.attn_plan(K, Kl, S, H, Dh, inj, dtype=dtype, part="bank", no_split=True) for inj in (False, True)}
    else:
        pl = sharded.frame_set_halo_plan(K, world, r, R, anchors)
        if anchors:
            multi = ops.attn_frame_sets_edits_part_plan(pl.F, pl.Kl, pl.q_frame0, pl.sets, S, H, Dh, E, mask, "bank", True,
                                                        dtype=dtype, no_split=True, multi_v=False)
            one = {inj: ops.attn_frame_sets_part_plan(pl.F, pl.Kl, pl.q_frame0, pl.sets, S, H, Dh, inj, dtype=dtype,
                                                      no_split=True) for inj in (False, True)}
        else:
            multi = ops.attn_windows_edits_part_plan(pl.F, pl.Kl, pl.hl, pl.windows, S, H, Dh, E, mask, "bank", True,
                                                     dtype=dtype, no_split=True, multi_v=False)
            one = {inj: ops.attn_windows_part_plan(pl.F, pl.Kl, pl.hl, pl.windows, S, H, Dh, inj, dtype=dtype, no_split=True)
                   for inj in (False, True)}
    n_inj = bin(mask).count("1")
    body = {inj: [t for t in p if t != "vt_pack"] for inj, p in one.items()}
    if S <= 256:
        want = body[True] if n_inj else body[False]
    else:
        want = ["vt_pack"] + body[True] * n_inj + body[False] * (E - n_inj)
    return _norm(multi), _norm(want)


def _edit3(t, e, B, Kl):
    """[B*Kl, S, D] -> the single-edit tensor [source | uncond_e | cond_e] of the rank's frames."""
    return t.view(B, Kl, *t.shape[1:])[[0, 1 + 2 * e, 2 + 2 * e]].reshape(3 * Kl, *t.shape[1:]).contiguous()


def _full_composition(ops, q, k, v, K, H, scale, E, mask, R, anchors):
    """ONE process: the bank part call plus the source-only edits part on the full tensors (bit-stable mode)."""
    B = 1 + 2 * E
    _, S, D = q.shape
    q4, k4, v4 = (t.view(B, K, S, D) for t in (q, k, v))
    out = torch.empty_like(q4)
    ops.ext_attn_edits_views(q4[0:1], k4[0:1], v4[0:1], out[0:1], H, scale, E, mask, "source", no_split=True)
    if anchors:
        ops.ext_attn_frame_sets_edits_views(q4, k4, v4[1:], out, H, scale, E, mask, ops.bank_frame_sets(K, R, anchors), "bank",
                                            branch0=(0, 0, 1, 0), no_split=True, multi_v=False)
    else:
        ops.ext_attn_windows_edits_views(q4, k4, v4[1:], out, H, scale, E, mask, ops.bank_windows(K, R), "bank",
                                         branch0=(0, 0, 1, 0), no_split=True, multi_v=False)
    return out.view(B * K, S, D)


def _nan_fill(ext):
    for t in ext:
        if t.element_size() == 2:
            t.view(torch.int16).fill_(0x7fc0 if t.dtype == torch.bfloat16 else 0x7e00)
        else:
            t.fill_(float("nan"))


def _world_worker(rank, world, port, K, configs, shapes, ret):
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        bad, n, left_out, checked = [], 2, 0, 0
        comm = gloo_comm(rank, world)
        multi = [("python", sharded.FrameShard(K, comm=comm, window_edits=True)),
                 ("native-edit", sharded.NativeEditShard(K, comm, window_edits=True)),
                 ("dist", sharded.FrameShard(K, window_edits=True))]
        single = sharded.FrameShard(K, comm=comm)      # the EXISTING single-edit windowed / anchored pass
        Kl, f0, o = single.Kl, single.kf0, 1
        for ci, (S, H, Dh, dtype) in enumerate(shapes):
            D, scale = H * Dh, Dh ** -0.5
            for R, spec in configs:
                anchors = tuple(range(0, K, spec)) if isinstance(spec, int) else tuple(spec)
                cover = R >= K - 1
                for ei, (E, mask) in enumerate(WORLD_EDITS):
                    B = 1 + 2 * E
                    what = f"K{K} W{world} R{R} anchors{anchors} S{S} H{H} Dh{Dh} {dtype} E{E} mask {mask:#b} rank {rank}"
                    g = torch.Generator().manual_seed(100 * K + 10 * ci + E)
                    q, k, v = (torch.randn(B * K, S, D, generator=g).to(dtype).cuda() for _ in range(3))
                    loc = lambda t: t.view(B, K, S, D)[:, f0:f0 + Kl].reshape(B * Kl, S, D)      # noqa: E731
                    outs = {}
                    for name, sh in multi:
                        outs[name] = sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, False, n_edits=E, inject_mask=mask,
                                                          window=R, anchors=anchors or None)
                    torch.cuda.synchronize()
                    for name, _ in multi[1:]:      # I5: the same bits on the same transport
                        if not torch.equal(outs[name], outs["python"]):
                            bad.append(f"{what} {name}: != the python shard")
                    # ---- I1: every edit against the existing single-edit pass, where both plans name the same form
                    got_t, want_t = _rank_tokens(ops, sharded, K, world, rank, R, anchors, S, H, Dh, dtype, E, mask)
                    if got_t != want_t:
                        left_out += 1
                        bad.append(f"{what}: I1 left out, the plans name different forms: {got_t} / {want_t}")
                    else:
                        checked += 1
                        for e in range(E):
                            ref = single.pivotal_attention(_edit3(loc(q), e, B, Kl), _edit3(loc(k), e, B, Kl),
                                                           _edit3(loc(v), e, B, Kl), H, scale, bool((mask >> e) & 1), window=R,
                                                           anchors=anchors or None)
                            if not torch.equal(_edit3(outs["python"], e, B, Kl), ref):
                                bad.append(f"{what}: I1, edit {e} != the single-edit pass")
                    # ---- I4: the canonical forms
                    if cover:      # the multi-edit bank pass, whatever the anchors
                        for name, sh in multi[:2]:
                            par = sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, False, mode="bank", n_edits=E,
                                                       inject_mask=mask)
                            if not torch.equal(par, outs[name]):
                                bad.append(f"{what} {name}: I4, a covering radius != the bank pass")
                    elif ei == 0:
                        # ---- I2: one process issuing the two part calls on the full tensors (K <= 64); every rank names the
                        #      single process's forms at these shapes (asserted through the tokens)
                        comp = _full_composition(ops, q, k, v, K, H, scale, E, mask, R, anchors)
                        full_t, _ = _rank_tokens(ops, sharded, K, 1, 0, R, anchors, S, H, Dh, dtype, E, mask)
                        untab = lambda plan: [t.replace(",win", "").replace(",set", "") for t in plan]      # noqa: E731
                        if untab(full_t) != untab(got_t):      # (a rank whose sets are ranges in ITS bank names ',win': same form)
                            bad.append(f"{what}: I2 left out: {full_t} / {got_t}")
                        elif not torch.equal(outs["python"], loc(comp)):
                            bad.append(f"{what}: I2, != the one-process composition")
                        whole = (ops.ext_attn_frame_sets_edits(q, k, v, H, scale, False, E, ops.bank_frame_sets(K, R, anchors),
                                                               inject_mask=mask, no_split=True, multi_v=False) if anchors else
                                 ops.ext_attn_windows_edits(q, k, v, H, scale, False, E, ops.bank_windows(K, R),
                                                            inject_mask=mask, no_split=True, multi_v=False))
                        if not torch.equal(comp, whole):
                            bad.append(f"{what}: I2, the composition != the single-GPU multi-edit call")
                        # ---- I5: the block call and the propagation behind it
                        piv = spread_pivots(K, S, D, dtype, g)[0].cuda()
                        inv = ops.pivot_inv_norm(piv)
                        tgt = torch.cat([(piv[c].float()[torch.randperm(S, generator=g).cuda()].repeat(n, 1)
                                          + 0.1 * torch.randn(n * S, D, generator=g).cuda()).to(dtype) for c in range(f0, f0 + Kl)])
                        res = torch.randn(B * Kl * n, S, D, generator=g).to(dtype).cuda()
                        s = torch.arange(0, n)
                        w = torch.sigmoid(torch.abs(s + n - n // 2) / (torch.abs(s - n // 2) + torch.abs(s + n - n // 2))).cuda()
                        blocks = {}
                        for name, sh in multi[:2]:
                            ext = sh.ext_alloc(S, D, dtype, piv.device, n_edits=E)
                            _nan_fill(ext)
                            ext[0][o:].copy_(piv[f0:f0 + Kl])
                            pe, ie, ke, reqs = sh.pivotal_block(loc(q), loc(k), loc(v), H, scale, False, ext, inv_norm=True,
                                                                n_edits=E, inject_mask=mask, window=R, anchors=anchors or None)
                            first, _rest = sh.propagate_all(tgt, res, pe, ie, ke, w, n, halo_reqs=reqs, n_edits=E)
                            torch.cuda.synchronize()
                            ke4 = ke.view(B, Kl + o, S, D)
                            blocks[name] = (ke4, first)
                            if not torch.equal(ke4[:, o:].reshape(B * Kl, S, D), outs["python"]):
                                bad.append(f"{what} {name}: I5, pivotal_block state != pivotal_attention")
                            if not (torch.equal(pe[o:], piv[f0:f0 + Kl]) and torch.equal(ie[o:], inv[f0:f0 + Kl])):
                                bad.append(f"{what} {name}: I5, local pivots / inverse norms")
                            if rank > 0 and not (torch.equal(pe[0], piv[f0 - 1]) and torch.equal(ie[0], inv[f0 - 1])
                                                 and torch.equal(ke4[:, 0], comp.view(B, K, S, D)[:, f0 - 1])):
                                bad.append(f"{what} {name}: I5, halo slot")
                            if not torch.equal(first, blocks["python"][1]):
                                bad.append(f"{what} {name}: I5, first chunk != the python shard's")
                        # ---- I4: E = 1 IS the single-edit pass
                        q3, k3, v3 = (_edit3(loc(t), 0, B, Kl) for t in (q, k, v))
                        for name, sh in multi[:2]:
                            a = sh.pivotal_attention(q3, k3, v3, H, scale, bool(mask & 1), n_edits=1, window=R,
                                                     anchors=anchors or None)
                            if not torch.equal(a, single.pivotal_attention(q3, k3, v3, H, scale, bool(mask & 1), window=R,
                                                                           anchors=anchors or None)):
                                bad.append(f"{what} {name}: I4, n_edits = 1 != the single-edit pass")
        print(f"K{K} W{world} rank {rank}: I1 checked for {checked} cases, left out for {left_out}")
        if left_out:
            bad.append(f"I1 left out for {left_out} cases")
        multi[1][1].close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001  (reported once, through the shared dict; nothing is retried)
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,K", [(2, 5), (3, 7)], ids=["K5-W2", "K7-W3"])
@pytest.mark.parametrize("part", [0, 1, 2], ids=["d40-d64", "d64-d40", "d80-f16"])
def test_windowed_multi_edit_shard(world, K, part):
    """K = 5 over 2 ranks (3, 2) and K = 7 over 3 ranks (3, 2, 2) with the configurations of tests/test_shard_frame_sets_gpu.py:
    I1 (zero cases left out), I2, I4 and I5, several cases inside ONE spawn per world."""
    configs = [(R, a) for R, a in CONFIGS if isinstance(a, int) or all(x < K for x in a)]
    ret = mp.Manager().dict()
    mp.spawn(_world_worker, args=(world, _free_port(), K, configs, WORLD_SHAPES[part], ret), nprocs=world, join=True)
    assert dict(ret) == {r: [] for r in range(world)}, dict(ret)


def _big_worker(rank, world, port, ret):
    """K = 66 > 64 over 3 ranks, R = 2, anchors {0, 33}, E = 2: I1 against the existing K = 66 pass; native == python."""
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        K, R, anchors, dtype, E = 66, 2, (0, 33), torch.bfloat16, 2
        B = 1 + 2 * E
        comm = gloo_comm(rank, world)
        py, nat = sharded.FrameShard(K, comm=comm, window_edits=True), sharded.NativeEditShard(K, comm, window_edits=True)
        single = sharded.FrameShard(K, comm=comm)
        Kl, f0 = py.Kl, py.kf0
        bad = []
        for S, H, Dh, mask in ((64, 2, 40, 0b01), (320, 2, 64, 0b11)):
            D, scale = H * Dh, Dh ** -0.5
            g = torch.Generator().manual_seed(S + Dh + mask)
            q, k, v = (torch.randn(B * Kl, S, D, generator=g).to(dtype).cuda() for _ in range(3))      # the rank's own frames
            what = f"K66 S{S} Dh{Dh} mask {mask:#b} rank {rank}"
            got_t, want_t = _rank_tokens(ops, sharded, K, world, rank, R, anchors, S, H, Dh, dtype, E, mask)
            if got_t != want_t:
                bad.append(f"{what}: I1 left out: {got_t} / {want_t}")
                continue
            outs = [sh.pivotal_attention(q, k, v, H, scale, False, n_edits=E, inject_mask=mask, window=R, anchors=anchors).clone()
                    for sh in (py, nat)]
            torch.cuda.synchronize()
            if not torch.equal(*outs):
                bad.append(f"{what}: native != python")
            for e in range(E):
                ref = single.pivotal_attention(_edit3(q, e, B, Kl), _edit3(k, e, B, Kl), _edit3(v, e, B, Kl), H, scale,
                                               bool((mask >> e) & 1), window=R, anchors=anchors)
                if not torch.equal(_edit3(outs[0], e, B, Kl), ref):
                    bad.append(f"{what}: I1, edit {e} != the existing K = 66 pass")
        nat.close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_more_than_64_keyframes():
    ret = mp.Manager().dict()
    mp.spawn(_big_worker, args=(3, _free_port(), ret), nprocs=3, join=True)
    assert dict(ret) == {0: [], 1: [], 2: []}, dict(ret)


def _bound_worker(rank, world, port, ret):
    """I6: attn_split=True, and the four-bank launches of `window_edits_multi_v=True` at head dims 40 and 64 (S = 320): every edit
    is held to the ORACLE's attention bound on every frame's members with its own flag (not to the bit-stable pass); the native
    executor and the Python form issue the same launches: the same bits."""
    _init(rank, world, port)
    try:
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = False
        K, R = 7, 2
        comm = gloo_comm(rank, world)
        bad = []
        for kw, anchors, S, H, Dh, E, mask, tok in ((dict(attn_split=True), (0,), 320, 2, 40, 2, 0b01, None),
                                                    (dict(attn_split=True), (), 64, 2, 64, 3, 0b101, None),
                                                    (dict(window_edits_multi_v=True), (), 320, 2, 40, 3, 0b111, "MV4"),
                                                    (dict(window_edits_multi_v=True), (0,), 320, 2, 64, 2, 0b11, "MV4")):
            py = sharded.FrameShard(K, comm=comm, window_edits=True, **kw)
            nat = sharded.NativeEditShard(K, comm, window_edits=True, **kw)
            Kl, f0, B = py.Kl, py.kf0, 1 + 2 * E
            D, scale = H * Dh, Dh ** -0.5
            what = f"{kw} anchors{anchors} S{S} Dh{Dh} E{E} mask {mask:#b} rank {rank}"
            if tok:      # the forced form is really taken on this rank
                hint = py._window_edits_hints(Dh)
                plan = sharded.rank_window_edits_plan(world, rank, K, S, H, Dh, R, anchors, E, mask, no_halo=True, no_split=False,
                                                      flags=ops._multi_v_bits(hint.get("multi_v"), hint.get("multi_v64")))
                if not any(tok in t for t in plan):
                    bad.append(f"{what}: no four-bank launch in {plan}")
            g = torch.Generator().manual_seed(S + Dh + E)
            q, k, v = (torch.randn(B * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
            loc = lambda t: t.view(B, K, S, D)[:, f0:f0 + Kl].reshape(B * Kl, S, D)      # noqa: E731
            outs = [sh.pivotal_attention(loc(q), loc(k), loc(v), H, scale, False, n_edits=E, inject_mask=mask, window=R,
                                         anchors=anchors or None).clone() for sh in (py, nat)]
            torch.cuda.synchronize()
            if not torch.equal(*outs):
                bad.append(f"{what}: native != python")
            sets = ops.bank_frame_sets(K, R, anchors)
            got = outs[0].view(B, Kl, S, D)
            worst = float("-inf")
            for e in range(E):
                sl = [0, 1 + 2 * e, 2 + 2 * e]
                for i in range(f0, f0 + Kl):
                    fr = [j for j in range(K) if (sets[i] >> j) & 1]
                    q3, k3, v3 = (t.view(B, K, S, D)[sl][:, fr].reshape(3 * len(fr), S, D).float().cpu() for t in (q, k, v))
                    r, ra, _ = attn_ref(q3, k3, v3, H, scale, bool((mask >> e) & 1), need_sigma=False)
                    pick = lambda t: t.view(3, len(fr), S, D)[:, fr.index(i)]      # noqa: E731
                    err = (got[sl, i - f0].float().cpu() - pick(r)).abs()
                    worst = max(worst, float((err - attn_bound(pick(r), pick(ra), dtype=torch.bfloat16)).max()))
            print(f"{what}: worst excess over the attention bound {worst:.3e}")
            if worst > 0:
                bad.append(f"{what}: I6, exceeds the oracle's attention bound by {worst:.3e}")
            nat.close()
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_attn_split_and_four_bank_form_on_a_windowed_multi_edit_shard():
    ret = mp.Manager().dict()
    mp.spawn(_bound_worker, args=(3, _free_port(), ret), nprocs=3, join=True)
    assert dict(ret) == {0: [], 1: [], 2: []}, dict(ret)


@pytest.mark.parametrize("anchors", [(), (0, 5)], ids=["windows", "anchors"])
def test_world_one_is_the_single_gpu_call(anchors):
    """I4 in-process: a world of one (no communicator, a loopback communicator of one rank) is `ops.ext_attn_windows_edits` /
    `ops.ext_attn_frame_sets_edits(no_split=True, multi_v=False)` bit for bit, through `pivotal_attention` and `pivotal_block`."""
    from tokenflow_amd import sharded
    from tokenflow_amd.comm import HipComm
    ops = _ops()
    K, R, S, H, Dh, E, mask = 6, 1, 64, 2, 40, 2, 0b01
    D, B, scale = H * Dh, 1 + 2 * E, Dh ** -0.5
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(B * K, S, D, generator=g).bfloat16().cuda() for _ in range(3))
    piv = torch.randn(K, S, D, generator=g).bfloat16().cuda()
    want = (ops.ext_attn_frame_sets_edits(q, k, v, H, scale, False, E, ops.bank_frame_sets(K, R, anchors), inject_mask=mask,
                                          no_split=True, multi_v=False) if anchors else
            ops.ext_attn_windows_edits(q, k, v, H, scale, False, E, ops.bank_windows(K, R), inject_mask=mask, no_split=True,
                                       multi_v=False))
    for sh in (sharded.FrameShard(K, window_edits=True), sharded.NativeEditShard(K, None, window_edits=True),
               sharded.NativeEditShard(K, HipComm.loopback(0, 1), window_edits=True)):
        got = sh.pivotal_attention(q, k, v, H, scale, False, n_edits=E, inject_mask=mask, window=R, anchors=anchors or None)
        assert torch.equal(got, want), type(sh).__name__
        ext = sh.ext_alloc(S, D, torch.bfloat16, q.device, n_edits=E)
        ext[0].copy_(piv)
        _pe, ie, ke, reqs = sh.pivotal_block(q, k, v, H, scale, False, ext, inv_norm=True, n_edits=E, inject_mask=mask, window=R,
                                             anchors=anchors or None)
        torch.cuda.synchronize()
        assert reqs == [] and torch.equal(ke, want) and torch.equal(ie, ops.pivot_inv_norm(piv)), type(sh).__name__


def _hooks_worker(rank, world, port, K, ret):
    """`register_frame_shard` + `register_edits(E = 2)` + per-edit schedules + `register_bank_window(pipe, 1, edits=True,
    shard=True, edit_shard=True)` on the small fake pipeline with the REAL kernels under autocast: the pivotal pass of a decoder
    block equals the unsharded windowed multi-edit hook pass on the rank's keyframes (S = 192, Dh = 40: the fused form on both
    sides -- one launch per edit there, ONE joint launch here, the same bits)."""
    _init(rank, world, port)
    try:
        import tokenflow_utils as tfu
        from tests import fake_diffusers as fd
        from tests.gloo_transport import gloo_comm
        from tokenflow_amd import ops, sharded
        ops.NO_SPLIT = True
        S, h, dims, E = 192, 2, (80, 160, 320), 2
        D, B = dims[0], 1 + 2 * E

        def pipe(registered, **kw):
            torch.manual_seed(0)
            p = fd.FakePipeline(dims=dims, heads=h, cross_dim=32).eval().cuda().bfloat16()
            tfu.register_extended_attention_pnp(p, [1])
            tfu.set_tokenflow(p.unet)
            tfu.register_time(p, 1)
            tfu.register_edits(p, E)
            tfu.register_edit_schedules(p, qk_schedules=[[1], []])      # edit 0 injects at this step, edit 1 does not
            if registered is not None:
                tfu.register_frame_shard(p, registered)
            tfu.register_bank_window(p, 1, **kw)
            tfu.register_pivotal(p, True)
            return p, p.unet.up_blocks[3].attentions[1].transformer_blocks[0]
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B, K, S, D, generator=g).cuda().bfloat16()
        enc = torch.randn(B, K, 7, 32, generator=g).cuda().bfloat16()
        bad = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            comm = gloo_comm(rank, world)
            for anchors in (None, [0, K - 1]):
                ref_kw = dict(edits=True) if anchors is None else dict(edits=True, anchors=anchors, anchor_edits=True)
                sh_kw = dict(ref_kw, shard=True, edit_shard=True, **({} if anchors is None else dict(anchor_shard=True)))
                _, blk = pipe(None, **ref_kw)
                want = blk(x.reshape(B * K, S, D), encoder_hidden_states=enc.reshape(B * K, 7, 32)).view(B, K, S, D).clone()
                for name, sh in (("python", sharded.FrameShard(K, comm=comm, window_edits=True)),
                                 ("native-edit", sharded.NativeEditShard(K, comm, window_edits=True))):
                    lo, hi = sh.kf0, sh.kf0 + sh.Kl
                    xl, el = x[:, lo:hi].reshape(B * sh.Kl, S, D), enc[:, lo:hi].reshape(B * sh.Kl, 7, 32)
                    _, blk = pipe(sh, **sh_kw)
                    got = blk(xl, encoder_hidden_states=el).view(B, sh.Kl, S, D)
                    torch.cuda.synchronize()
                    if not torch.equal(got, want[:, lo:hi]):
                        bad.append(f"{name} anchors={anchors}: block output of the windowed multi-edit shard")
                    _, blk = pipe(sh, **{k_: v_ for k_, v_ in sh_kw.items() if k_ != "edit_shard"})      # the old error stays
                    try:
                        blk(xl, encoder_hidden_states=el)
                        bad.append(f"{name}: no error without edit_shard=True")
                    except ValueError as e:
                        if "runs one edit" not in str(e):
                            bad.append(f"{name}: {e}")
        ret[rank] = bad
    except Exception as e:      # noqa: BLE001
        import traceback
        ret[rank] = [f"{type(e).__name__}: {e}", traceback.format_exc()]
    finally:
        dist.destroy_process_group()


def test_hooks_two_ranks_two_edits_per_edit_schedules():
    ret = mp.Manager().dict()
    mp.spawn(_hooks_worker, args=(2, _free_port(), 4, ret), nprocs=2, join=True)
    assert dict(ret) == {0: [], 1: []}, dict(ret)
