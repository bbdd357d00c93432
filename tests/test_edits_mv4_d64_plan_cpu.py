"""Launch plans of the four-bank shared-softmax form at head dim 64 (TF_ATTN_MULTI_V64; host only: the library records the
launches it would make).

Under q/k injection every bank branch of every injecting edit has the source's softmax(QK^T); with the hint on, one launch
(token one<64,..,MV4,..>) computes the bank branches of a PAIR of injecting edits, an odd one takes the DUAL launch, the
others their own bank-only launches, the source branch runs last.  The hint of the head dim 40 form, TF_ATTN_MULTI_V,
keeps its meaning: at head dim 64 it selects nothing."""
import ctypes
import re

import pytest
import torch

from tokenflow_amd import _lib, ops

MV4_64 = re.compile(r"one<64,\d+,\d+,MV4,")
DTYPES = [torch.bfloat16, torch.float16]
# (K, Kq, S, H): BASELINE config 4 / 5 levels 0 and 1, a query-frame subset, the shapes of the GPU tests (ragged, short)
SHAPES = [(10, 10, 9216, 5), (25, 25, 4096, 5), (10, 10, 2304, 10), (25, 25, 1024, 10), (8, 3, 1024, 8), (3, 3, 192, 2),
          (2, 2, 77, 2), (2, 2, 320, 5)]


def _strip(plan):
    return [t for t in plan if t != "vt_pack"]


def _n_mv4(plan):
    return sum(1 for t in plan if MV4_64.match(t))


def test_the_flag_is_bit_21_and_additive():
    assert _lib.TF_ATTN_MULTI_V64 == 1 << 21
    assert _lib.ABI_VERSION == 11 and _lib.load().tf_abi_version() == 11
    others = [_lib.TF_ATTN_MULTI_V, _lib.TF_ATTN_NO_MULTI_V, _lib.TF_ATTN_HINT_MIX, _lib.TF_ATTN_FUSED, _lib.TF_ATTN_BANK_ONLY,
              _lib.TF_ATTN_SOURCE_ONLY, _lib.TF_ATTN_NO_SPLIT, _lib.TF_ATTN_NO_FUSED, _lib.TF_ATTN_FOLD_SCALE]
    assert all(not (_lib.TF_ATTN_MULTI_V64 & b) for b in others)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,Kq,S,H", SHAPES)
def test_forced_on_pairs_then_odd_dual_then_source(K, Kq, S, H, dtype):
    src = _strip(ops.attn_plan(K, Kq, S, H, 64, True, dtype=dtype, part="source"))
    for E in (2, 3, 4):
        plan = ops.attn_edits_plan(K, Kq, S, H, 64, True, E, dtype=dtype, multi_v64=True)
        assert plan[0] == "vt_pack" and plan.count("vt_pack") == 1, plan
        body = plan[1:]
        assert all(MV4_64.match(t) for t in body[:E // 2]) and _n_mv4(plan) == E // 2, plan
        odd = body[E // 2:len(body) - len(src)]
        assert len(odd) == E % 2 and all(",DUAL," in t for t in odd), plan
        assert body[len(body) - len(src):] == src, plan
        assert not any(t.startswith("merge") or t.startswith("fused") for t in body[:len(body) - len(src)]), plan
        # the uniform mask is the same call
        assert ops.attn_edits_plan(K, Kq, S, H, 64, False, E, dtype=dtype, multi_v64=True, inject_mask=(1 << E) - 1) == plan


@pytest.mark.parametrize("K,Kq,S,H", SHAPES)
@pytest.mark.parametrize("E,mask", [(3, 0b101), (4, 0b0111), (3, 0b010), (4, 0b1111), (3, 0b000)])
def test_masks_pair_the_injecting_edits(K, Kq, S, H, E, mask):
    """popcount // 2 four-bank launches, in front of everything else; a single injecting edit has no partner; the launches of
    the other parts are those of the composition."""
    n_inj = bin(mask).count("1")
    on = ops.attn_edits_plan(K, Kq, S, H, 64, False, E, inject_mask=mask, multi_v64=True)
    off = ops.attn_edits_plan(K, Kq, S, H, 64, False, E, inject_mask=mask, multi_v=False)
    assert _n_mv4(on) == n_inj // 2 and _n_mv4(off) == 0
    if n_inj < 2:
        assert on == off
        return
    body = _strip(on)
    assert all(MV4_64.match(t) for t in body[:n_inj // 2]), on
    assert sum(1 for t in body[n_inj // 2:n_inj // 2 + n_inj % 2] if ",DUAL," in t) == n_inj % 2, on
    # behind the injecting edits: the non-injecting edits' bank launches and the source launches, as without the hint
    non = _strip(ops.attn_plan(K, Kq, S, H, 64, False, part="bank"))
    src = _strip(ops.attn_plan(K, Kq, S, H, 64, mask == (1 << E) - 1, part="source"))
    tail = non * (E - n_inj) + src
    assert body[len(body) - len(tail):] == tail and _strip(off)[len(_strip(off)) - len(tail):] == tail, (on, off)
    assert len(body) == n_inj // 2 + n_inj % 2 + len(tail), on


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_op_where_the_form_does_not_exist(dtype):
    K, S, H = 8, 1024, 8
    for dh in (40, 80, 160):
        for inject in (False, True):
            for E in (1, 2, 3):
                assert ops.attn_edits_plan(K, K, S, H, dh, inject, E, dtype=dtype, multi_v64=True) == \
                    ops.attn_edits_plan(K, K, S, H, dh, inject, E, dtype=dtype), (dh, inject, E)
    for S_ in (77, 320, 1024, 4096):
        for E in (2, 3):    # without injection
            assert ops.attn_edits_plan(K, K, S_, H, 64, False, E, dtype=dtype, multi_v64=True) == \
                ops.attn_edits_plan(K, K, S_, H, 64, False, E, dtype=dtype)
        # one edit: the single-edit plan
        for inject in (False, True):
            assert ops.attn_edits_plan(K, K, S_, H, 64, inject, 1, dtype=dtype, multi_v64=True) == \
                ops.attn_plan(K, K, S_, H, 64, inject, dtype=dtype)
        # the folded scale
        assert ops.attn_edits_plan(K, K, S_, H, 64, True, 2, dtype=dtype, multi_v64=True, fold_scale=True) == \
            ops.attn_edits_plan(K, K, S_, H, 64, True, 2, dtype=dtype, fold_scale=True)
    # the Dh = 40 form keeps its own hint and its own token
    assert ops.attn_edits_plan(K, K, S, H, 40, True, 2, multi_v=True, multi_v64=True) == \
        ops.attn_edits_plan(K, K, S, H, 40, True, 2, multi_v=True)


def _in_default(K, Kq, S, H):
    """The measured shape classes (profiles/r13_attn_edits_d64_ab.txt): the box spanned by levels 0 and 1 of BASELINE
    configs 4 and 5."""
    return Kq == K and H in (5, 10) and 10 <= K <= 25 and S % 64 == 0 and 1024 <= S <= 9216


@pytest.mark.parametrize("K,Kq,S,H", SHAPES + [(8, 8, 1024, 8), (8, 8, 4096, 8), (4, 4, 1024, 8), (2, 2, 320, 2)])
def test_the_old_hint_and_no_hint(K, Kq, S, H):
    """TF_ATTN_MULTI_V at head dim 64 selects nothing: with it, as without a hint, the library's rule decides -- the
    composition outside the measured classes; TF_ATTN_NO_MULTI_V switches the form off everywhere."""
    bank = _strip(ops.attn_plan(K, Kq, S, H, 64, True, part="bank"))
    src = _strip(ops.attn_plan(K, Kq, S, H, 64, True, part="source"))
    for E in (2, 3):
        for kw in (dict(multi_v=True), dict(), dict(multi_v=False), dict(multi_v64=False), dict(multi_v64=None)):
            plan = ops.attn_edits_plan(K, Kq, S, H, 64, True, E, **kw)
            if _in_default(K, Kq, S, H) and kw.get("multi_v") is not False:
                assert plan == ops.attn_edits_plan(K, Kq, S, H, 64, True, E, multi_v64=True), (kw, plan)
            else:
                assert _strip(plan) == bank * E + src and _n_mv4(plan) == 0, (kw, plan)
        assert _n_mv4(ops.attn_edits_plan(K, Kq, S, H, 64, True, E, multi_v=True, multi_v64=True)) == E // 2


def test_default_covers_only_the_measured_shape_classes():
    """Without a hint: Kq = K, 5 or 10 heads, 10 to 25 keyframes, whole 64-key tiles, 1024 <= S <= 9216.  It requires every
    keyframe's queries and K >= 10, and covers no shape the existing tests run with the default; the hint reaches the rest."""
    cases = [(10, 10, 9216, 5, True), (25, 25, 4096, 5, True), (10, 10, 2304, 10, True), (25, 25, 1024, 10, True),
             (16, 16, 4096, 10, True), (10, 5, 9216, 5, False), (25, 24, 1024, 10, False), (9, 9, 4096, 5, False),
             (26, 26, 1024, 10, False), (10, 10, 9216, 8, False), (10, 10, 960, 10, False), (10, 10, 9280, 5, False),
             (10, 10, 2300, 10, False), (8, 8, 1024, 8, False), (8, 8, 4096, 8, False), (4, 4, 1024, 8, False),
             (2, 2, 320, 2, False)]
    for K, Kq, S, H, on in cases:
        assert on == _in_default(K, Kq, S, H)
        for E, mask in ((2, 0b11), (3, 0b111), (3, 0b101)):
            assert (_n_mv4(ops.attn_edits_plan(K, Kq, S, H, 64, False, E, inject_mask=mask)) > 0) == on, (K, Kq, S, H, E)
            assert _n_mv4(ops.attn_edits_plan(K, Kq, S, H, 64, False, E, inject_mask=mask, multi_v64=True)) == 1
            assert _n_mv4(ops.attn_edits_plan(K, Kq, S, H, 64, False, E, inject_mask=mask, multi_v=False)) == 0
        for dh in (40, 80, 160):    # the rule is the head dim 64 form's
            assert not any(",MV4," in t and "<64," in t for t in ops.attn_edits_plan(K, Kq, S, H, dh, True, 2))


def test_both_switches_are_an_error():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1024)
    both = _lib.TF_ATTN_MULTI_V64 | _lib.TF_ATTN_NO_MULTI_V
    for dh in (40, 64, 80):
        assert lib.tf_ext_attn_edits_plan(8, 8, 1024, 8, dh, 2, 1 | both, _lib.TF_BF16, buf, len(buf)) == -3   # TF_ERR_SHAPE
        assert lib.tf_ext_attn_edits_masked_plan(8, 8, 1024, 8, dh, 2, 0b11, both, _lib.TF_BF16, buf, len(buf)) == -3
        assert lib.tf_ext_attn_edits_part_plan(8, 8, 1024, 8, dh, 2, 0b11, 0, both, _lib.TF_BF16, buf, len(buf)) == -3
    with pytest.raises(_lib.TokenflowHipError, match="TF_ATTN_MULTI_V64 and TF_ATTN_NO_MULTI_V"):
        ops.attn_edits_plan(8, 8, 1024, 8, 64, True, 2, multi_v=False, multi_v64=True)
    with pytest.raises(_lib.TokenflowHipError, match="TF_ATTN_MULTI_V64 and TF_ATTN_NO_MULTI_V"):
        ops.attn_edits_part_plan(8, 8, 1024, 8, 64, 2, 0b11, multi_v=False, multi_v64=True)
    with pytest.raises(_lib.TokenflowHipError):       # no CPU fallback, and the keyword reaches the call
        ops.ext_attn_edits(torch.zeros(10, 8, 128), torch.zeros(10, 8, 128), torch.zeros(10, 8, 128), 2, 1.0, True, 2,
                           multi_v64=True)
    with pytest.raises(_lib.TokenflowHipError):
        z = torch.zeros(5, 2, 8, 128)
        ops.ext_attn_edits_views(z, z, z, z.clone(), 2, 1.0, 2, 0b11, multi_v64=True)


def test_the_run_entry_points_refuse_the_flag():
    """No partial epilogue in the four-bank kernel: as TF_ATTN_MULTI_V, TF_ERR_SHAPE before anything touches the device."""
    lib = _lib.load()
    K, Kq, q0, S, H, Dh, n_runs, E = 5, 2, 2, 256, 2, 64, 3, 2
    D = H * Dh
    dt = _lib.TF_BF16
    fs = S * D
    strides = (ctypes.c_int64 * 9)(Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, D)
    nbytes = lib.tf_ext_attn_runs_edits_workspace_bytes(K, Kq, S, H, Dh, n_runs, E, dt)
    assert nbytes > 0
    ph = 1 << 12   # placeholder pointers: aligned, never dereferenced by a refused call
    for flags in (_lib.TF_ATTN_MULTI_V64, _lib.TF_ATTN_MULTI_V64 | _lib.TF_ATTN_BANK_ONLY,
                  _lib.TF_ATTN_MULTI_V64 | _lib.TF_ATTN_MULTI_V):
        for E_, mask in ((E, 0b11), (1, 0b1)):
            rc = lib.tf_ext_attn_run_edits(ph, ph, ph, ph, K, Kq, q0, 2, 2, 0, n_runs, S, H, Dh, D,
                                           ctypes.cast(strides, ctypes.c_void_p), 1.0, flags, dt, E_, mask, 0, ph, nbytes, None)
            assert rc == -3 and "tf_ext_attn_run_edits" in lib.tf_last_error().decode(), (flags, E_, rc)
        rc = lib.tf_ext_attn_runs_merge_edits(ph, K, Kq, S, H, Dh, n_runs, E, 0b11, Kq * fs, fs, flags & ~_lib.TF_ATTN_BANK_ONLY,
                                              dt, ph, nbytes, None)
        assert rc == -3 and "tf_ext_attn_runs_merge_edits" in lib.tf_last_error().decode(), (flags, rc)
    with pytest.raises(_lib.TokenflowHipError, match="tf_ext_attn_run_edits_plan"):
        ops.attn_run_edits_plan(5, 2, 2, 3, 256, 2, 64, 2, 0b11, hints=_lib.TF_ATTN_MULTI_V64)


@pytest.mark.parametrize("K,Kq,S,H", SHAPES)
@pytest.mark.parametrize("E,mask", [(2, 0b11), (3, 0b111), (3, 0b101), (4, 0b0111), (3, 0b010)])
def test_the_part_call_cuts_the_masked_plan(K, Kq, S, H, E, mask):
    kw = dict(fused=False, multi_v64=True)
    masked = ops.attn_edits_plan(K, Kq, S, H, 64, False, E, inject_mask=mask, **kw)
    src = _strip(ops.attn_plan(K, Kq, S, H, 64, mask == (1 << E) - 1, part="source", fused=False))
    assert masked[0] == "vt_pack" and masked[-len(src):] == src
    assert _n_mv4(masked) == bin(mask).count("1") // 2
    assert ops.attn_edits_part_plan(K, Kq, S, H, 64, E, mask, part="bank", **kw) == masked[:-len(src)]
    assert ops.attn_edits_part_plan(K, Kq, S, H, 64, E, mask, part="source", **kw) == ["vt_pack"] + src
    for compact in (False, True):
        assert ops.attn_edits_part_plan(K, Kq, S, H, 64, E, mask, part="all", qk_compact=compact, **kw) == masked
