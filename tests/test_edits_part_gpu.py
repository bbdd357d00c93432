"""The parts of a multi-edit attention call and the pack / unpack of a multi-edit batch on the GPU.

  * `head_pack` / `head_unpack` above the six slabs of one edit, bit-exact against the torch re-layout;
  * `ext_attn_edits_views(part=...)`: the bank part and the source part BIT-IDENTICAL to the per-edit `ext_attn_views` calls
    (four-bank form off), dense and compact q / k on the same values; bank + source written into one `out` equal the "all"
    call; the source slab of `out` survives the bank part and the source slab of `v` need not exist;
  * the fused regime: ONE launch over all parts (the plan token first), bit-identical to the per-edit calls under
    no_split=True, within the project's attention bound of the oracle in the default mode.
q, k and v are independent per branch and per frame: a launch that read another slot, another edit's bank or another query
frame lands O(1) off."""
import pytest
import torch

from tests.test_kernels_gpu import assert_attn_close, attn_ref

pytestmark = pytest.mark.gpu

MV4 = "one<40,1,4,MV4,2,fq0>"
DTYPES = [torch.bfloat16, torch.float16]
POISON = 7.0


def _ops():
    from tokenflow_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------------ pack / unpack
def _slabs(n, Kl, S, D, dtype, g):
    """n [Kl, S, D] slabs with three different frame strides (dense, every other frame of a larger tensor, padded frames)."""
    out = []
    for i in range(n):
        if i % 3 == 0:
            t = torch.randn(Kl, S, D, generator=g, device="cuda").to(dtype)
        elif i % 3 == 1:
            t = torch.randn(Kl, 2, S, D, generator=g, device="cuda").to(dtype)[:, 1]
        else:
            t = torch.randn(Kl, S + 3, D, generator=g, device="cuda").to(dtype)[:, :S]
        out.append(t)
    return out


@pytest.mark.parametrize("dtype,hd", [(torch.bfloat16, 8), (torch.float32, 4)])
@pytest.mark.parametrize("Kl", [1, 2])
@pytest.mark.parametrize("ns", [6, 7, 48])
def test_head_pack_many_slabs(ns, Kl, dtype, hd):
    ops = _ops()
    W, S = 2, 8
    g = torch.Generator(device="cuda").manual_seed(ns + Kl)
    slabs = _slabs(ns, Kl, S, W * hd, dtype, g)
    want = torch.stack([t.reshape(Kl, S, W, hd) for t in slabs], 0).permute(3, 1, 0, 2, 4).contiguous()   # [W,Kl,ns,S,hd]
    got = ops.head_pack(slabs, W)
    assert got.shape == (W, Kl, ns, S, hd) and torch.equal(got, want)


@pytest.mark.parametrize("dtype,hd", [(torch.bfloat16, 8), (torch.float32, 4)])
@pytest.mark.parametrize("Kl", [1, 2])
@pytest.mark.parametrize("nb", [6, 7, 16, 48])
def test_head_unpack_many_destinations(nb, Kl, dtype, hd):
    ops = _ops()
    W, S = 2, 8
    g = torch.Generator(device="cuda").manual_seed(nb + Kl)
    recv = torch.randn(W, Kl, nb, S, hd, generator=g, device="cuda").to(dtype)
    dsts = _slabs(nb, Kl, S, W * hd, dtype, g)
    ops.head_unpack(recv, dsts)
    for b, t in enumerate(dsts):
        assert torch.equal(t, recv[:, :, b].permute(1, 2, 0, 3).reshape(Kl, S, W * hd)), b


def test_head_pack_refuses_more_than_the_bound():
    from tokenflow_amd import _lib
    ops = _ops()
    slabs = [torch.zeros(1, 8, 16, device="cuda", dtype=torch.bfloat16)] * (6 * _lib.TF_MAX_EDITS + 1)
    with pytest.raises(_lib.TokenflowHipError):
        ops.head_pack(slabs, 2)


# ------------------------------------------------------------------------------------------------------ the part call
def _inputs(E, K, S, D, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    B = 1 + 2 * E
    return tuple(torch.randn(B, K, S, D, generator=g, device="cuda").to(dtype) for _ in range(3))


def _compact(t, mask, E):
    """[source | the (uncond, cond) slots of the edits that do not inject, ascending]"""
    keep = [0] + [b for e in range(E) if not (mask >> e) & 1 for b in (1 + 2 * e, 2 + 2 * e)]
    return t[keep].contiguous()


def _per_edit_reference(ops, q, k, v, Kq, f0, h, d, mask, E, **kw):
    """Every edit's bank branches through its own `ext_attn_views(part="bank")` call with its own flag, the source branch
    through the part="source" call (given inject iff every edit injects, as the composition does)."""
    B, K, S, D = k.shape
    qf = q[:, f0:f0 + Kq]
    ref = torch.full((B, Kq, S, D), POISON, dtype=q.dtype, device=q.device)
    for e in range(E):
        lo = 1 + 2 * e
        if (mask >> e) & 1:
            ops.ext_attn_views(qf[0:1], k[0:1], v[lo:lo + 2], ref[lo:lo + 2], h, d ** -0.5, True, "bank",
                               branch0=(0, 0, 1, 1), q_frame0=f0, **kw)
        else:
            ops.ext_attn_views(qf[lo:lo + 2], k[lo:lo + 2], v[lo:lo + 2], ref[lo:lo + 2], h, d ** -0.5, False, "bank",
                               branch0=(1, 1, 1, 1), q_frame0=f0, **kw)
    ops.ext_attn_views(qf[0:1], k[0:1], v[0:1], ref[0:1], h, d ** -0.5, mask == (1 << E) - 1, "source", q_frame0=f0, **kw)
    return ref


def _check_parts(ops, q, k, v, Kq, f0, h, d, mask, E, ref, what, **kw):
    """bank part (source slabs of v absent, of out poisoned), then the source part into the same `out`, against `ref`; the
    "all" call; dense and compact q / k."""
    B, K, S, D = k.shape
    all_inject, none_inject = mask == (1 << E) - 1, mask == 0
    for compact in (False, True):
        qq, kk = (_compact(t, mask, E) if compact else t for t in (q, k))
        qf = qq[:, f0:f0 + Kq]
        out = torch.full((B, Kq, S, D), POISON, dtype=q.dtype, device=q.device)
        if none_inject:      # no launch reads slot 0 of q / k: it need not exist
            ops.ext_attn_edits_views(qf[1:], kk[1:], v[1:], out[1:], h, d ** -0.5, E, mask, "bank", compact,
                                     branch0=(1, 1, 1, 1), q_frame0=f0, **kw)
        elif all_inject:     # ... and nothing but slot 0 here
            ops.ext_attn_edits_views(qf[0:1], kk[0:1], v[1:], out[1:], h, d ** -0.5, E, mask, "bank", compact,
                                     branch0=(0, 0, 1, 1), q_frame0=f0, **kw)
        else:
            ops.ext_attn_edits_views(qf, kk, v[1:], out, h, d ** -0.5, E, mask, "bank", compact, branch0=(0, 0, 1, 0),
                                     q_frame0=f0, **kw)
        assert torch.equal(out[1:], ref[1:]), f"{what} compact {compact}: bank part"
        assert bool((out[0] == POISON).all()), f"{what} compact {compact}: the bank part wrote the source slab"
        ops.ext_attn_edits_views(qf[0:1], kk[0:1], v[0:1], out[0:1], h, d ** -0.5, E, mask, "source", compact, q_frame0=f0,
                                 **kw)
        assert torch.equal(out, ref), f"{what} compact {compact}: source part"
        both = torch.full_like(out, POISON)
        ops.ext_attn_edits_views(qf, kk, v, both, h, d ** -0.5, E, mask, "all", compact, q_frame0=f0, **kw)
        assert torch.equal(both, ref), f"{what} compact {compact}: all parts"


def _assert_within_bound(got, q, k, v, Kq, f0, h, d, mask, E, dtype, what):
    """every edit against the oracle on [source | uncond_e | cond_e] with ITS flag, every element"""
    B, K, S, D = k.shape
    for e in range(E):
        sl = [0, 1 + 2 * e, 2 + 2 * e]
        q3, k3, v3 = (t[sl].reshape(3 * K, S, D).float().cpu() for t in (q, k, v))
        r = attn_ref(q3, k3, v3, h, d ** -0.5, bool((mask >> e) & 1), need_sigma=False)
        refs = tuple(x.view(3, K, S, D)[:, f0:f0 + Kq].reshape(3 * Kq, S, D) for x in r[:2]) + (None,)
        assert_attn_close(got[sl].reshape(3 * Kq, S, D), refs, f"{what} edit {e}", dtype=dtype)


STREAMING = [(40, 3, [0b000, 0b111, 0b101, 0b010]), (80, 2, [0b00, 0b11, 0b01])]


@pytest.mark.parametrize("d,E,masks", STREAMING)
@pytest.mark.parametrize("dtype", DTYPES)
def test_streaming_parts_equal_the_per_edit_calls(d, E, masks, dtype):
    """K = 4 bank frames, the rank's Kq = 2 query frames from frame 2 on, S = 320 (five 64-key tiles, the last ragged against
    the 128-token padding).  One-pass form (no_split: the mode a frame shard runs in) and the split form of a small grid."""
    ops = _ops()
    K, Kq, f0, S, h = 4, 2, 2, 320, 2
    q, k, v = _inputs(E, K, S, h * d, dtype, seed=d + E)
    for kw in (dict(no_split=True, multi_v=False), dict(fused=False, multi_v=False)):
        ref_kw = {x: y for x, y in kw.items() if x != "multi_v"}
        for mask in masks:
            what = f"d{d} E{E} mask {mask:#b} {dtype} {kw}"
            plan = ops.attn_edits_part_plan(K, Kq, S, h, d, E, mask, dtype=dtype, **kw)
            assert plan[0] == "vt_pack" and plan.count("vt_pack") == 1 and MV4 not in plan, (what, plan)
            assert not any(t.startswith("fused") for t in plan), (what, plan)
            ref = _per_edit_reference(ops, q, k, v, Kq, f0, h, d, mask, E, **ref_kw)
            _check_parts(ops, q, k, v, Kq, f0, h, d, mask, E, ref, what, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_four_bank_form_in_the_bank_part_vs_oracle(dtype):
    ops = _ops()
    K, Kq, f0, S, h, d, E, mask = 4, 2, 2, 320, 2, 40, 3, 0b111
    q, k, v = _inputs(E, K, S, h * d, dtype, seed=5)
    plan = ops.attn_edits_part_plan(K, Kq, S, h, d, E, mask, part="bank", dtype=dtype, multi_v=True)
    assert plan.count(MV4) == 1 and plan[0] == "vt_pack" and sum(",DUAL," in t for t in plan) == 1, plan
    for compact in (False, True):
        qq, kk = (_compact(t, mask, E) if compact else t for t in (q, k))
        out = torch.full((1 + 2 * E, Kq, S, h * d), POISON, dtype=dtype, device="cuda")
        ops.ext_attn_edits_views(qq[0:1, f0:f0 + Kq], kk[0:1], v[1:], out[1:], h, d ** -0.5, E, mask, "bank", compact,
                                 branch0=(0, 0, 1, 1), q_frame0=f0, multi_v=True)
        assert bool((out[0] == POISON).all())
        ops.ext_attn_edits_views(qq[0:1, f0:f0 + Kq], kk[0:1], v[0:1], out[0:1], h, d ** -0.5, E, mask, "source", compact,
                                 q_frame0=f0, multi_v=True)
        _assert_within_bound(out, q, k, v, Kq, f0, h, d, mask, E, dtype, f"four-bank {dtype} compact {compact}")


# S: a ragged last 32-key sub-tile / two sub-tiles / six; every head dim; mixed masks; nine sets once
FUSED = [(S, d, E, mask) for S, d in [(40, 40), (64, 160), (192, 80), (64, 64), (192, 40), (40, 80)]
         for E, mask in [(2, 0b01), (3, 0b101)]] + [(40, 160, 3, 0b010), (192, 64, 2, 0b10), (64, 40, 8, 0b10110101)]


@pytest.mark.parametrize("S,d,E,mask", FUSED)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_parts_share_one_launch(S, d, E, mask, dtype):
    ops = _ops()
    K, Kq, f0, h = 3, 2, 1, 2
    q, k, v = _inputs(E, K, S, h * d, dtype, seed=S + d + E)
    what = f"S{S} d{d} E{E} mask {mask:#b} {dtype}"
    prec = 1 if dtype == torch.bfloat16 else 0
    for part, n_sets in (("all", E + 1), ("bank", E), ("source", 1)):
        tok = f"fused[qw=1,kw=4,qb=1,prec={prec}" + (f",sets={n_sets}]" if n_sets > 2 else "]")
        for no_split in (True, None):
            assert ops.attn_edits_part_plan(K, Kq, S, h, d, E, mask, part=part, dtype=dtype, no_split=no_split) == [tok], what
    ref = _per_edit_reference(ops, q, k, v, Kq, f0, h, d, mask, E, no_split=True)
    _check_parts(ops, q, k, v, Kq, f0, h, d, mask, E, ref, what, no_split=True)
    for compact in (False, True):     # the default mode: held to the oracle
        qq, kk = (_compact(t, mask, E) if compact else t for t in (q, k))
        out = torch.full((1 + 2 * E, Kq, S, h * d), POISON, dtype=dtype, device="cuda")
        ops.ext_attn_edits_views(qq[:, f0:f0 + Kq], kk, v, out, h, d ** -0.5, E, mask, "all", compact, q_frame0=f0)
        _assert_within_bound(out, q, k, v, Kq, f0, h, d, mask, E, dtype, what + f" default mode compact {compact}")


def test_view_and_argument_errors():
    ops = _ops()
    E, K, S, h, d = 2, 3, 64, 2, 40
    q, k, v = _inputs(E, K, S, h * d, torch.bfloat16, seed=1)
    out = torch.empty_like(q)
    with pytest.raises(ValueError):      # a mask bit above the edits
        ops.ext_attn_edits_views(q, k, v, out, h, d ** -0.5, E, 0b100)
    with pytest.raises(ValueError):      # the bank part of a mixed mask reads slot 0 of q: a view from slot 1 cannot hold it
        ops.ext_attn_edits_views(q[1:], k, v, out, h, d ** -0.5, E, 0b01, "bank", branch0=(1, 0, 0, 0))
    with pytest.raises(ValueError):      # compact q of a mixed mask has 3 slots; the dense addressing needs 5
        ops.ext_attn_edits_views(q[:3], k, v, out, h, d ** -0.5, E, 0b01, "all", False)
    with pytest.raises(KeyError):
        ops.ext_attn_edits_views(q, k, v, out, h, d ** -0.5, E, 0, "both")
