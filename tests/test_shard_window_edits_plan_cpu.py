"""Several prompts on a windowed / anchored frame shard, host side (no GPU): the native executor's recorded plan
(tf_rank_pivotal_frame_sets_edits_plan) against the Python geometry and the part plans, the part entry points' plans
(tf_ext_attn_windows_edits_part_plan / tf_ext_attn_frame_sets_edits_part_plan) against the single-edit part plans, the canonical
forms as token equality, and the refusals of the executor, of the part entry points and of the pack."""
import ctypes
import inspect

import pytest
import torch

from tokenflow_amd import _lib, ops, sharded

# every (K, W, R, anchors) of tests/test_shard_window_plan_cpu.py (no anchors) and tests/test_shard_frame_sets_plan_cpu.py
GEOMETRIES = ([(K, W, R, ()) for K, W, R in [(5, 2, 1), (7, 3, 1), (7, 3, 2), (7, 3, 3), (25, 8, 2)]] +
              [(5, 2, 1, (0,)), (7, 3, 1, (0,)), (7, 3, 1, (0, 3, 6)), (7, 3, 0, (0,)), (7, 3, 2, (0, 3, 6)), (25, 8, 2, (0,)),
               (25, 8, 2, (0, 8, 16, 24)), (66, 3, 2, (0, 33))])
SHAPES = [(64, 2, 40), (320, 2, 64), (320, 1, 80)]
EDITS = [(E, m) for E in (2, 3) for m in (0, (1 << E) - 1, 0b01)]      # masks: none, all, mixed


def _rows(token):
    """'a2a[slabs=N,send=a/b,recv=c/d]' -> (N, [a, b], [c, d])"""
    body = dict(kv.split("=") for kv in token[len("a2a["):-1].split(","))
    return int(body["slabs"]), [int(x) for x in body["send"].split("/")], [int(x) for x in body["recv"].split("/")]


def _slabs(E, mask):
    """(ns, nq) of the pack: the compact k slots (the source where some edit injects + 2 per non-injecting edit) and the 2E
    value slabs; the compact q slots are staged only under a mixed mask."""
    n_non = E - bin(mask).count("1")
    slots = (1 if mask else 0) + 2 * n_non
    return slots + 2 * E, (slots if mask and n_non else 0)


def _bank_plan(pl, anchors, S, H, Dh, E, mask, **kw):
    if anchors:
        return ops.attn_frame_sets_edits_part_plan(pl.F, pl.Kl, pl.q_frame0, pl.sets, S, H, Dh, E, mask, "bank", True, **kw)
    return ops.attn_windows_edits_part_plan(pl.F, pl.Kl, pl.hl, pl.windows, S, H, Dh, E, mask, "bank", True, **kw)


def _whole(pl, anchors):
    if anchors:
        return all(m == (1 << pl.F) - 1 for m in pl.sets)
    return all((lo, n) == (0, pl.F) for lo, n in pl.windows)


def _is_range(m):
    lo = (m & -m).bit_length() - 1
    return (m >> lo) & ((m >> lo) + 1) == 0


@pytest.mark.parametrize("K,W,R,anchors", GEOMETRIES)
@pytest.mark.parametrize("S,H,Dh", SHAPES)
def test_native_plan_is_the_composition(K, W, R, anchors, S, H, Dh):
    joint = 0
    for r in range(W):
        pl = sharded.frame_set_halo_plan(K, W, r, R, anchors)      # (no anchors: the windowed plan)
        for E, mask in EDITS:
            ns, nq = _slabs(E, mask)
            src = ops.attn_edits_part_plan(pl.Kl, pl.Kl, S, H, Dh, E, mask, part="source", no_split=True)
            bank = _bank_plan(pl, anchors, S, H, Dh, E, mask, no_split=True)
            what = f"K={K} W={W} R={R} anchors={anchors} rank {r} E={E} mask={mask:#b}"
            if S == 64 and not _whole(pl, anchors):      # ONE launch over all edits under the one table
                ranges = not anchors or all(_is_range(m) for m in pl.sets)
                assert len(bank) == 1 and bank[0].endswith(f",sets={E},{'win' if ranges else 'set'}]"), (what, bank)
                joint += 1
            for inv_norm in (False, True):
                got = sharded.rank_window_edits_plan(W, r, K, S, H, Dh, R, anchors, E, mask, inv_norm=inv_norm)
                head = (["inv_norm"] if inv_norm else []) + [f"edit_pack[ns={ns},nq={nq}]"]
                assert got[:len(head)] == head, (what, got)
                assert _rows(got[len(head)]) == (ns, pl.send_rows, pl.recv_rows), (what, got, pl)
                assert got[len(head) + 1:] == src + bank + [f"halo[n={2 + 1 + 2 * E}]"], (what, got, src, bank)
            got = sharded.rank_window_edits_plan(W, r, K, S, H, Dh, R, anchors, E, mask, no_halo=True)
            assert got[2:] == src + bank, (what, got)
    if S == 64:
        assert joint      # the joint launch occurs in every geometry of the list


@pytest.mark.parametrize("kind", ["win", "set"])
@pytest.mark.parametrize("S,H,Dh", SHAPES + [(64, 1, 160), (1024, 5, 64)])
def test_part_plan_against_the_single_edit_parts(S, H, Dh, kind):
    """The bank part of E edits names the launches of the E single-edit bank parts: S <= 256 ONE joint launch with their KW and
    PREC, above ONE pre-pass, then the injecting edits' launches, then the others'.  Dense and compact q / k: the same plan."""
    K, Kq, f0 = 7, 3, 2
    whole = ops.bank_windows(K, 1) if kind == "win" else ops.bank_frame_sets(K, 1, (0, 6))
    tab = whole[f0:f0 + Kq]
    plan1 = ops.attn_windows_part_plan if kind == "win" else ops.attn_frame_sets_part_plan
    plan_n = ops.attn_windows_edits_part_plan if kind == "win" else ops.attn_frame_sets_edits_part_plan
    one = {inj: plan1(K, Kq, f0, tab, S, H, Dh, inj, no_split=True) for inj in (False, True)}
    body = {inj: [t for t in p if t != "vt_pack"] for inj, p in one.items()}
    for E, mask in EDITS + [(3, 0b101), (8, 0b10110101)]:
        n_inj = bin(mask).count("1")
        if S <= 256:
            assert one[True] == one[False] and len(one[True]) == 1
            want = [one[True][0].replace(f",{kind}]", f",sets={E},{kind}]")]
        else:
            want = ["vt_pack"] + body[True] * n_inj + body[False] * (E - n_inj)
        for compact in (False, True):
            assert plan_n(K, Kq, f0, tab, S, H, Dh, E, mask, "bank", compact, no_split=True, multi_v=False) == want, (E, mask)


def test_part_plan_canonical_forms():
    K, Kq, f0, S, H, Dh = 7, 3, 2, 320, 2, 40
    win = ops.bank_windows(K, 1)[f0:f0 + Kq]
    sets = ops.bank_frame_sets(K, 1, (0, 6))[f0:f0 + Kq]
    ranges = [((1 << n) - 1) << lo for lo, n in win]
    kw = dict(no_split=True)
    for S in (64, 320):
        for mask in (0, 1):      # E = 1 IS the single-edit part, with TF_ATTN_INJECT iff mask = 1
            assert (ops.attn_windows_edits_part_plan(K, Kq, f0, win, S, H, Dh, 1, mask, **kw)
                    == ops.attn_windows_part_plan(K, Kq, f0, win, S, H, Dh, bool(mask), **kw))
            assert (ops.attn_frame_sets_edits_part_plan(K, Kq, f0, sets, S, H, Dh, 1, mask, **kw)
                    == ops.attn_frame_sets_part_plan(K, Kq, f0, sets, S, H, Dh, bool(mask), **kw))
        for E, mask in EDITS:
            # every set a range IS the windows part
            assert (ops.attn_frame_sets_edits_part_plan(K, Kq, f0, ranges, S, H, Dh, E, mask, **kw)
                    == ops.attn_windows_edits_part_plan(K, Kq, f0, win, S, H, Dh, E, mask, **kw))
            # every window / set the whole bank IS the edits part
            want = ops.attn_edits_part_plan(K, Kq, S, H, Dh, E, mask, part="bank", **kw)
            assert ops.attn_windows_edits_part_plan(K, Kq, f0, [(0, K)] * Kq, S, H, Dh, E, mask, **kw) == want
            assert ops.attn_frame_sets_edits_part_plan(K, Kq, f0, [(1 << K) - 1] * Kq, S, H, Dh, E, mask, **kw) == want
            # without a part flag the call IS the non-part call: one fused launch per edit there, as its plan tests pin
            w_all, s_all = ops.bank_windows(K, 1), ops.bank_frame_sets(K, 1, (0, 6))
            assert (ops.attn_windows_edits_part_plan(K, K, 0, w_all, S, H, Dh, E, mask, "all", **kw)
                    == ops.attn_windows_edits_plan(K, w_all, S, H, Dh, E, mask, **kw))
            assert (ops.attn_frame_sets_edits_part_plan(K, K, 0, s_all, S, H, Dh, E, mask, "all", **kw)
                    == ops.attn_frame_sets_edits_plan(K, s_all, S, H, Dh, E, mask, **kw))
    # the four-bank hints stay accepted, under the windowed rule: forced on, a pair of injecting edits shares one launch
    forced = ops.attn_windows_edits_part_plan(K, Kq, f0, win, 320, 2, 40, 3, 0b111, no_split=True, multi_v=True)
    assert sum(t.startswith("one<40,1,4,MV4,2,fq0>") and t.endswith(",win") for t in forced) == 1, forced
    forced = ops.attn_frame_sets_edits_part_plan(K, Kq, f0, sets, 320, 2, 64, 2, 0b11, no_split=True, multi_v64=True)
    assert sum(t.startswith("one<64,1,8,MV4,2,fq1>") and t.endswith(",set") for t in forced) == 1, forced


@pytest.mark.parametrize("K,W", [(5, 2), (7, 3), (25, 8)])
def test_canonical_forms_of_the_native_plan(K, W):
    for r in range(W):
        for S in (64, 320):
            for anchors in ((), (0,), (0, K - 1)):
                for mask in (0, 1):      # E = 1 IS the single-edit anchored / windowed pass
                    assert (sharded.rank_window_edits_plan(W, r, K, S, 2, 40, 1, anchors, 1, mask, inv_norm=True)
                            == sharded.rank_frame_sets_plan(W, r, K, S, 2, 40, 1, anchors, inject=bool(mask), inv_norm=True))
                for E, mask in EDITS:      # a covering radius IS the multi-edit bank pass whatever the anchors
                    want = sharded.rank_edits_plan(W, r, K, S, 2, 40, E, mask, mode="bank")
                    for R in (K - 1, K, 1000):
                        assert sharded.rank_window_edits_plan(W, r, K, S, 2, 40, R, anchors, E, mask) == want, (R, anchors)


def test_world_one_is_the_single_gpu_call():
    K, R = 6, 1
    for S in (64, 320):
        for E, mask in EDITS:
            assert (sharded.rank_window_edits_plan(1, 0, K, S, 2, 40, R, (), E, mask)
                    == ops.attn_windows_edits_plan(K, ops.bank_windows(K, R), S, 2, 40, E, mask, no_split=True))
            assert (sharded.rank_window_edits_plan(1, 0, K, S, 2, 40, R, (0, 5), E, mask)
                    == ops.attn_frame_sets_edits_plan(K, ops.bank_frame_sets(K, R, (0, 5)), S, 2, 40, E, mask, no_split=True))


def _plan_rc(fn, *args):
    buf = ctypes.create_string_buffer(4096)
    return fn(*args, buf, len(buf))


def test_refusals_of_the_executor():
    lib = _lib.load()
    anc = lambda *a: (ctypes.cast((ctypes.c_int * max(len(a), 1))(*a), ctypes.c_void_p), len(a))      # noqa: E731
    plan = lambda W, r, K, R, a, E=2, mask=0, mode=_lib.TF_RANK_BANK, flags=0, dtype=_lib.TF_BF16: _plan_rc(      # noqa: E731
        lib.tf_rank_pivotal_frame_sets_edits_plan, W, r, K, 64, 2, 40, R, *anc(*a), E, mask, mode, flags, dtype)
    assert plan(2, 0, 5, 1, (0,)) > 0 and plan(2, 0, 5, 1, ()) > 0
    # what tf_rank_pivotal_frame_sets refuses
    for bad in ((5,), (-1,)):
        assert plan(2, 0, 5, 1, bad) == -3 and b"anchor" in lib.tf_last_error()
    assert plan(9, 0, 200, 2, tuple(range(30, 200, 4))) == -3 and b"64" in lib.tf_last_error()
    assert plan(9, 0, 200, 2, tuple(range(30, 200, 5))) > 0
    assert plan(2, 0, 5, -1, (0,)) == -3 and b"radius" in lib.tf_last_error()
    Kl = _lib.TF_MAX_WINDOW_FRAMES + 1
    assert plan(2, 0, 2 * Kl, 1, (0,)) == -3 and b"local keyframes" in lib.tf_last_error()
    assert plan(2, 0, 5, 1, (0,), flags=_lib.TF_ATTN_BANK_ONLY) == -3
    assert plan(2, 0, 5, 1, (0,), flags=_lib.TF_ATTN_FOLD_SCALE) == -3
    assert plan(2, 0, 5, 1, (0,), dtype=_lib.TF_F32) == -2
    # what tf_rank_pivotal_edits refuses
    assert plan(2, 0, 5, 1, (0,), E=0) == -3 and plan(2, 0, 5, 1, (0,), E=_lib.TF_MAX_EDITS + 1) == -3
    assert plan(2, 0, 5, 1, (0,), E=2, mask=0b100) == -3 and b"inject_mask" in lib.tf_last_error()
    assert plan(2, 0, 5, 1, (0,), flags=_lib.TF_ATTN_INJECT) == -3
    # every mode but TF_RANK_BANK
    for mode in (_lib.TF_RANK_HEADS, _lib.TF_RANK_BANK_RUNS, _lib.TF_RANK_BANK_EDIT_RUNS):
        assert plan(2, 0, 5, 1, (0,), mode=mode) == -3 and b"mode" in lib.tf_last_error()
        assert plan(2, 0, 5, 1, (), mode=mode) == -3
    assert plan(2, 0, 5, 1, (0,), mode=_lib.TF_RANK_BANK | _lib.TF_RANK_NO_HALO | _lib.TF_RANK_INV_NORM) == -3      # both
    assert plan(2, 0, 5, 1, (0,), mode=_lib.TF_RANK_BANK | _lib.TF_RANK_NO_HALO) > 0


def test_refusals_of_the_part_entry_points():
    lib = _lib.load()
    K = 7
    lo, n = (ctypes.c_int * K)(*[w[0] for w in ops.bank_windows(K, 1)]), (ctypes.c_int * K)(*[w[1] for w in ops.bank_windows(K, 1)])
    sets = (ctypes.c_uint64 * K)(*ops.bank_frame_sets(K, 1, (0, 6)))
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    win = lambda flags, E=2, mask=0, compact=0, lo_=lo, n_=n: _plan_rc(      # noqa: E731
        lib.tf_ext_attn_windows_edits_part_plan, K, K, 0, 64, 2, 40, E, mask, compact, flags, _lib.TF_BF16, vp(lo_), vp(n_))
    fset = lambda flags, E=2, mask=0, compact=0, tab=sets: _plan_rc(      # noqa: E731
        lib.tf_ext_attn_frame_sets_edits_part_plan, K, K, 0, 64, 2, 40, E, mask, compact, flags, _lib.TF_BF16, vp(tab))
    bad_n = (ctypes.c_int * K)(*([0] + [w[1] for w in ops.bank_windows(K, 1)][1:]))      # an empty window
    bad_lo = (ctypes.c_int * K)(*([1] + [w[0] for w in ops.bank_windows(K, 1)][1:]))     # window 0 without its own frame
    bad_sets = [(ctypes.c_uint64 * K)(*([0] + ops.bank_frame_sets(K, 1, (0, 6))[1:])),               # an empty set
                (ctypes.c_uint64 * K)(*([1 << K | 1] + ops.bank_frame_sets(K, 1, (0, 6))[1:])),      # a bit at or above K
                (ctypes.c_uint64 * K)(*([2] + ops.bank_frame_sets(K, 1, (0, 6))[1:]))]               # set 0 without frame 0
    for call, bad_tables in ((win, [dict(n_=bad_n), dict(lo_=bad_lo)]), (fset, [dict(tab=t) for t in bad_sets])):
        assert call(_lib.TF_ATTN_BANK_ONLY) == 1 and call(_lib.TF_ATTN_BANK_ONLY, compact=1) == 1
        assert call(0) > 1                                                 # the non-part call: one launch per edit + the source
        assert call(_lib.TF_ATTN_SOURCE_ONLY) == -3 and b"TF_ATTN_SOURCE_ONLY" in lib.tf_last_error()
        assert call(_lib.TF_ATTN_BANK_ONLY | _lib.TF_ATTN_SOURCE_ONLY) == -3
        assert call(_lib.TF_ATTN_BANK_ONLY, mask=0b100) == -3 and b"inject_mask" in lib.tf_last_error()
        assert call(_lib.TF_ATTN_BANK_ONLY, E=0) == -3 and call(_lib.TF_ATTN_BANK_ONLY, E=_lib.TF_MAX_EDITS + 1) == -3
        assert call(_lib.TF_ATTN_BANK_ONLY, compact=2) == -3 and b"qk_compact" in lib.tf_last_error()
        assert call(0, compact=1) == -3 and b"qk_compact" in lib.tf_last_error()      # the whole call reads dense q / k
        assert call(_lib.TF_ATTN_BANK_ONLY | _lib.TF_ATTN_INJECT) == -3
        assert call(_lib.TF_ATTN_BANK_ONLY | _lib.TF_ATTN_FOLD_SCALE) == -3
        assert call(_lib.TF_ATTN_BANK_ONLY | _lib.TF_ATTN_MULTI_V | _lib.TF_ATTN_NO_MULTI_V) == -3
        assert call(_lib.TF_ATTN_BANK_ONLY | _lib.TF_ATTN_NO_MULTI_V) == 1      # the hints stay accepted
        for bad in bad_tables:
            assert call(_lib.TF_ATTN_BANK_ONLY, **bad) == -3, bad
    assert _plan_rc(lib.tf_ext_attn_windows_edits_part_plan, K, K, 0, 64, 2, 40, 2, 0, 0, _lib.TF_ATTN_BANK_ONLY, _lib.TF_BF16,
                    None, None) == -1


def test_refusals_of_the_pack():
    lib = _lib.load()
    p16 = ctypes.c_void_p(1 << 12)
    cast = lambda a: [ctypes.cast(x, ctypes.c_void_p) if isinstance(x, ctypes.Array) else x for x in a]      # noqa: E731

    def args(ns=1, nq=0, **kw):
        slabs = kw.get("slabs", (ctypes.c_void_p * max(ns, 1))(*[1 << 12] * ns))
        fs = (ctypes.c_int64 * max(ns, 1))(*[64 * 80] * ns)
        qs = kw.get("qs", (ctypes.c_void_p * max(nq, 1))(*[1 << 12] * nq))
        qfs = (ctypes.c_int64 * max(nq, 1))(*[64 * 80] * nq)
        return cast([slabs, fs, ns, kw.get("send", p16), 2, (ctypes.c_uint64 * 2)(*kw.get("masks", (0, 0))), qs, qfs, nq,
                     kw.get("stage", p16), 2, 64, 80, kw.get("ld", 80), kw.get("ld_q", 80), kw.get("dtype", _lib.TF_BF16), None])
    pack = lib.tf_edit_halo_pack
    assert pack(*args()) == 0 and pack(*args(ns=4 * _lib.TF_MAX_EDITS)) == 0      # nothing to send, nothing to stage: no launch
    assert pack(*args(dtype=_lib.TF_F32)) == -2
    assert pack(*args(send=ctypes.c_void_p((1 << 12) + 2))) == -4
    assert pack(*args(slabs=(ctypes.c_void_p * 1)((1 << 12) + 2))) == -4
    assert pack(*args(ns=4 * _lib.TF_MAX_EDITS + 1)) == -3 and pack(*args(ns=0)) == -3      # ns = 33
    assert pack(*args(masks=(3, 4))) == -3 and b"at or above" in lib.tf_last_error()
    assert pack(*args(ld=84)) == -3
    assert pack(*args(nq=2 * _lib.TF_MAX_EDITS + 2)) == -3 and pack(*args(nq=-1)) == -3
    assert pack(*args(nq=1, ld_q=84)) == -3
    assert pack(*args(nq=1, stage=ctypes.c_void_p((1 << 12) + 2))) == -4
    assert pack(*args(nq=1, qs=(ctypes.c_void_p * 1)((1 << 12) + 2))) == -4
    assert pack(*args(nq=1, stage=None)) == -1


def test_python_opt_in_and_signatures():
    for cls, want in ((sharded.FrameShard, True), (sharded.NativeShard, False), (sharded.NativeEditShard, True)):
        assert cls.supports_window_edits is want
    for cls in (sharded.FrameShard, sharded.NativeEditShard):
        for name in ("window_edits", "window_edits_multi_v"):
            assert name in inspect.signature(cls.__init__).parameters, (cls.__name__, name)
    # an object made with __new__, or without the keyword, keeps raising the "one edit" error
    t = torch.zeros(5 * 4, 2, 16)
    for cls in (sharded.FrameShard, sharded.NativeEditShard):
        sh = cls.__new__(cls)
        sh.K, sh.Kl, sh.world = 8, 4, 2
        with pytest.raises(ValueError, match="one edit"):
            sh.pivotal_attention(t, t, t, 2, 1.0, False, n_edits=2, inject_mask=0, window=1)
        with pytest.raises(ValueError, match="one edit"):
            sh.pivotal_attention(t, t, t, 2, 1.0, False, n_edits=2, inject_mask=0, window=1, anchors=(0,))
        assert sh._window(7, 2) is None      # a covering radius is the pass without the keyword, as before
    off = sharded.FrameShard(8)
    assert off.window_edits is False and off.window_edits_multi_v is False
    with pytest.raises(ValueError, match="one edit"):
        off._window(1, 2)
    on = sharded.FrameShard(8, window_edits=True)
    assert on._window(1, 2) == 1 and on._window(1, 1) == 1 and on._window(7, 2) is None
    with pytest.raises(ValueError, match="mode="):
        on._window(1, 2, "heads")
    assert on._window_edits_hints(40) == dict(multi_v=False) == on._window_edits_hints(64)
    mv = sharded.FrameShard(8, window_edits=True, window_edits_multi_v=True)
    assert mv._window_edits_hints(40) == dict(multi_v=True) and mv._window_edits_hints(64) == dict(multi_v64=True)
    assert mv._window_edits_hints(80) == {}


def test_environment_opt_in(monkeypatch):
    monkeypatch.setenv("TOKENFLOW_SHARD_WINDOW_EDITS", "1")
    monkeypatch.setenv("TOKENFLOW_SHARD_WINDOW_EDITS_MULTI_V", "1")
    sh = sharded.FrameShard(8)
    assert sh.window_edits and sh.window_edits_multi_v
    assert not sharded.FrameShard(8, window_edits=False).window_edits
