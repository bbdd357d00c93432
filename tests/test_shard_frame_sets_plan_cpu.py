"""Anchor keyframes on a windowed frame shard, host side (no GPU): the exchange geometry `sharded.frame_set_halo_plan` against
a brute-force restatement, the native executor's recorded plan (tf_rank_pivotal_frame_sets_plan) and
`ops.attn_frame_sets_part_plan` against the geometry, the canonical forms and the refusals."""
import ctypes

import pytest
import torch

from tokenflow_amd import _lib, ops, sharded


def _own(K, W, p):
    counts = [K // W + (1 if r < K % W else 0) for r in range(W)]
    f0 = sum(counts[:p])
    return list(range(f0, f0 + counts[p]))


def _window(K, g, R):
    return {f for f in range(K) if abs(f - g) <= R}


def _reads(K, W, r, R, anchors):
    """U_r, brute force: every frame a window of one of rank r's keyframes names, plus the anchors."""
    need = set(anchors)
    for g in _own(K, W, r):
        need |= _window(K, g, R)
    return sorted(need)


def _bits(mask):
    return [j for j in range(mask.bit_length()) if (mask >> j) & 1]


def _anchor_sets(K):
    return [(), (0,), (K - 1,), (0, K // 2), tuple(range(0, K, 3))]


def test_geometry_against_brute_force():
    for K in range(1, 11):
        for W in range(1, min(K, 4) + 1):
            for R in range(0, K + 1):
                for anchors in _anchor_sets(K):
                    plans = [sharded.frame_set_halo_plan(K, W, r, R, anchors) for r in range(W)]
                    for r, pl in enumerate(plans):
                        what = f"K={K} W={W} R={R} anchors={anchors} rank {r}"
                        if not anchors:      # the plan IS the windowed plan, field for field
                            assert pl == sharded.window_halo_plan(K, W, r, R), what
                            continue
                        own, U = _own(K, W, r), _reads(K, W, r, R, anchors)
                        assert (pl.kf0, pl.Kl, pl.F) == (own[0], len(own), len(U)) and list(pl.U) == U, what
                        # the receive rows in rank order are U ascending, no duplicate rows
                        got = [g for p in range(W) for g in pl.recv[p]]
                        assert got == U and len(set(got)) == len(got), what
                        assert pl.recv_rows == [len(x) for x in pl.recv], what
                        assert pl.send_rows == [len(_bits(m)) for m in pl.send] and pl.send[r] == (1 << pl.Kl) - 1, what
                        for p, other in enumerate(plans):      # what p sends to r is what r expects from p
                            sent = [other.kf0 + i for i in _bits(other.send[r])]
                            assert sent == pl.recv[p] == [g for g in U if g in _own(K, W, p)], what + f" peer {p}"
                        # the own frames are contiguous at q_frame0
                        assert U[pl.q_frame0:pl.q_frame0 + pl.Kl] == own, what
                        assert pl.q_frame0 == sum(1 for g in U if g < own[0]), what
                        # each set maps back to window | anchors
                        for i, m in enumerate(pl.sets):
                            assert {U[j] for j in _bits(m)} == _window(K, own[i], R) | set(anchors), what + f" query {i}"
                            assert m >> pl.F == 0 and (m >> (pl.q_frame0 + i)) & 1, what


def test_reference_values():
    f = sharded.frame_set_halo_plan
    want = {(7, 3, 1, (0,)): [([0, 1, 2, 3], 0), ([0, 2, 3, 4, 5], 2), ([0, 4, 5, 6], 2)],
            (7, 3, 1, (0, 3, 6)): [([0, 1, 2, 3, 6], 0), ([0, 2, 3, 4, 5, 6], 2), ([0, 3, 4, 5, 6], 3)]}
    for (K, W, R, anchors), ranks in want.items():
        for r, (U, q0) in enumerate(ranks):
            assert _reads(K, W, r, R, anchors) == U      # the brute-force side names the same frames
            pl = f(K, W, r, R, anchors)
            assert (list(pl.U), pl.q_frame0) == (U, q0), (K, W, R, anchors, r)
    pl = f(7, 3, 0, 1, (0,))
    assert (pl.send_rows, pl.recv_rows) == ([3, 2, 1], [3, 1, 0])
    # contiguity is judged in the extended bank's coordinates: rank 0's sets are ranges, rank 1's query 4 is not
    assert [_bits(m) for m in f(7, 3, 0, 1, (0,)).sets] == [[0, 1], [0, 1, 2], [0, 1, 2, 3]]
    assert [_bits(m) for m in f(7, 3, 1, 1, (0,)).sets] == [[0, 1, 2, 3], [0, 2, 3, 4]]
    # K > 64: the masks cover the rank's extended bank only
    got = [f(66, 3, r, 2, (0, 33)) for r in range(3)]
    assert [pl.F for pl in got] == [25, 27, 26] and [pl.q_frame0 for pl in got] == [0, 3, 4]
    assert [len(_reads(66, 3, r, 2, (0, 33))) for r in range(3)] == [25, 27, 26]
    assert f(66, 3, 0, 2, (0, 0, 33, 33)) == got[0]      # duplicates are fine


def test_geometry_refusals():
    f = sharded.frame_set_halo_plan
    for bad in ((4, 5, 0, 1), (4, 2, 2, 1), (4, 2, 0, -1), (4, 0, 0, 1)):
        with pytest.raises(ValueError):
            f(*bad, (0,))
    for anchors in ((4,), (-1,), (0, 7), (1.5,), (True,)):
        with pytest.raises(ValueError, match="anchor"):
            f(4, 2, 0, 1, anchors)
    with pytest.raises(ValueError, match="64"):      # F > 64: 22 + 2 reach + 41 anchors outside it
        f(200, 9, 0, 2, tuple(range(30, 200, 4)))
    assert f(200, 9, 0, 2, tuple(range(30, 200, 5))).F <= 64
    with pytest.raises(ValueError, match="local keyframes"):
        f(2 * (_lib.TF_MAX_WINDOW_FRAMES + 1), 2, 0, 1, (0,))


def _rows(token):
    """'a2a[slabs=N,send=a/b,recv=c/d]' -> (N, [a, b], [c, d])"""
    body = dict(kv.split("=") for kv in token[len("a2a["):-1].split(","))
    return int(body["slabs"]), [int(x) for x in body["send"].split("/")], [int(x) for x in body["recv"].split("/")]


def _is_range(m):
    lo = (m & -m).bit_length() - 1
    return (m >> lo) & ((m >> lo) + 1) == 0


def _suffix(plan, s):
    return any(t.endswith("," + s) or t.endswith("," + s + "]") for t in plan)


@pytest.mark.parametrize("K,W,R,anchors", [(5, 2, 1, (0,)), (7, 3, 1, (0,)), (7, 3, 1, (0, 3, 6)), (7, 3, 0, (0,)),
                                           (7, 3, 2, (0, 3, 6)), (25, 8, 2, (0,)), (25, 8, 2, (0, 8, 16, 24)),
                                           (66, 3, 2, (0, 33))])
@pytest.mark.parametrize("S,H,Dh", [(64, 2, 40), (320, 2, 64), (320, 1, 80)])
@pytest.mark.parametrize("inject", [False, True])
def test_native_plan_is_the_composition(K, W, R, anchors, S, H, Dh, inject):
    kinds = set()
    for r in range(W):
        pl = sharded.frame_set_halo_plan(K, W, r, R, anchors)
        ns = 3 if inject else 4
        src = ops.attn_plan(pl.Kl, pl.Kl, S, H, Dh, inject, part="source", no_split=True)
        bank = ops.attn_frame_sets_part_plan(pl.F, pl.Kl, pl.q_frame0, pl.sets, S, H, Dh, inject, part="bank", no_split=True)
        ranges = all(_is_range(m) for m in pl.sets)
        kinds.add(ranges)
        if all(m == (1 << pl.F) - 1 for m in pl.sets):      # every set the rank's whole extended bank: the plain bank part
            assert bank == ops.attn_plan(pl.F, pl.Kl, S, H, Dh, inject, part="bank", no_split=True), (r, bank)
        else:
            assert _suffix(bank, "win" if ranges else "set") and not _suffix(bank, "set" if ranges else "win"), (r, bank)
        if ranges:      # the windowed part on the equivalent table: the same tokens
            table = [((m & -m).bit_length() - 1, bin(m).count("1")) for m in pl.sets]
            assert bank == ops.attn_windows_part_plan(pl.F, pl.Kl, pl.q_frame0, table, S, H, Dh, inject, no_split=True)
        for inv_norm in (False, True):
            got = sharded.rank_frame_sets_plan(W, r, K, S, H, Dh, R, anchors, inject=inject, inv_norm=inv_norm)
            head = (["inv_norm"] if inv_norm else []) + [f"set_pack[ns={ns}]"]
            assert got[:len(head)] == head, got
            assert _rows(got[len(head)]) == (ns, pl.send_rows, pl.recv_rows), (got, pl)
            assert got[len(head) + 1:] == src + bank + ["halo[n=5]"], (got, src, bank)
        got = sharded.rank_frame_sets_plan(W, r, K, S, H, Dh, R, anchors, inject=inject, no_halo=True)
        assert got[2:] == src + bank, got
    if (K, W, R, anchors) == (7, 3, 1, (0,)):
        assert kinds == {True, False}      # rank 0 is all ranges, ranks 1 and 2 are not


@pytest.mark.parametrize("K,W", [(5, 2), (7, 3), (25, 8)])
def test_canonical_forms_of_the_native_plan(K, W):
    for r in range(W):
        for inject in (False, True):
            for R in (0, 1, 2):      # no anchors: the token list of the windowed call
                assert (sharded.rank_frame_sets_plan(W, r, K, 320, 2, 40, R, (), inject=inject)
                        == sharded.rank_window_plan(W, r, K, 320, 2, 40, R, inject=inject))
            want = sharded.rank_edits_plan(W, r, K, 320, 2, 40, 1, 1 if inject else 0, mode="bank")
            for R in (K - 1, K, 1000):      # a covering radius: the bank pass whatever the anchors
                assert sharded.rank_frame_sets_plan(W, r, K, 320, 2, 40, R, (0, K - 1), inject=inject) == want, (R, want)


def test_world_one_is_the_frame_set_call():
    K, R, anchors = 6, 1, (0, 5)
    assert (sharded.rank_frame_sets_plan(1, 0, K, 320, 2, 40, R, anchors)
            == ops.attn_frame_sets_plan(K, ops.bank_frame_sets(K, R, anchors), 320, 2, 40, False, no_split=True))


def test_part_plan_canonical_forms():
    K = 4
    full = [(1 << K) - 1] * 2
    assert (ops.attn_frame_sets_part_plan(K, 2, 1, full, 320, 2, 40, True, no_split=True)
            == ops.attn_plan(K, 2, 320, 2, 40, True, part="bank", no_split=True))
    sets = ops.bank_frame_sets(7, 1, (0, 6))
    assert (ops.attn_frame_sets_part_plan(7, 7, 0, sets, 320, 2, 40, False, part="all", no_split=True)
            == ops.attn_frame_sets_plan(7, sets, 320, 2, 40, False, no_split=True))
    with pytest.raises(ValueError):
        ops.attn_frame_sets_part_plan(7, 7, 0, sets, 320, 2, 40, False, part="source")


def _plan_rc(fn, *args):
    buf = ctypes.create_string_buffer(4096)
    return fn(*args, buf, len(buf))


def test_refusals():
    lib = _lib.load()
    K = 7
    tab = ctypes.cast((ctypes.c_uint64 * K)(*ops.bank_frame_sets(K, 1, (0, 6))), ctypes.c_void_p)
    # tf_ext_attn_fwd_frame_sets keeps refusing the part flags; the part entry point takes TF_ATTN_BANK_ONLY, not _SOURCE_ONLY
    for flag in (_lib.TF_ATTN_BANK_ONLY, _lib.TF_ATTN_SOURCE_ONLY):
        assert _plan_rc(lib.tf_ext_attn_frame_sets_plan, K, K, 0, 320, 2, 40, flag, _lib.TF_BF16, tab) < 0
    assert _plan_rc(lib.tf_ext_attn_frame_sets_part_plan, K, K, 0, 320, 2, 40, _lib.TF_ATTN_BANK_ONLY, _lib.TF_BF16, tab) > 0
    assert _plan_rc(lib.tf_ext_attn_frame_sets_part_plan, K, K, 0, 320, 2, 40, _lib.TF_ATTN_SOURCE_ONLY, _lib.TF_BF16, tab) < 0
    assert b"TF_ATTN_SOURCE_ONLY" in lib.tf_last_error()
    # the executor: a bad anchor, F > 64, a bad radius, too many local keyframes, a part flag, the runs mode
    anc = lambda *a: (ctypes.cast((ctypes.c_int * len(a))(*a), ctypes.c_void_p), len(a))      # noqa: E731
    plan = lambda W, r, K, R, a, mode=_lib.TF_RANK_BANK, flags=0: _plan_rc(      # noqa: E731
        lib.tf_rank_pivotal_frame_sets_plan, W, r, K, 64, 2, 40, R, *anc(*a), mode, flags, _lib.TF_BF16)
    assert plan(2, 0, 5, 1, (0,)) > 0
    for bad in ((5,), (-1,)):
        assert plan(2, 0, 5, 1, bad) == -3 and b"anchor" in lib.tf_last_error()
    assert plan(9, 0, 200, 2, tuple(range(30, 200, 4))) == -3 and b"64" in lib.tf_last_error()
    assert plan(9, 0, 200, 2, tuple(range(30, 200, 5))) > 0
    assert plan(2, 0, 5, -1, (0,)) == -3 and b"radius" in lib.tf_last_error()
    Kl = _lib.TF_MAX_WINDOW_FRAMES + 1
    assert plan(2, 0, 2 * Kl, 1, (0,)) == -3 and b"local keyframes" in lib.tf_last_error()
    assert plan(2, 0, 5, 1, (0,), flags=_lib.TF_ATTN_BANK_ONLY) == -3
    assert plan(2, 0, 5, 1, (0,), mode=_lib.TF_RANK_BANK_RUNS) == -3
    # the pack entry point refuses before any launch: dtype, alignment, a bit at or above Kl
    p16 = ctypes.c_void_p(1 << 12)
    slabs, fs = (ctypes.c_void_p * 1)(1 << 12), (ctypes.c_int64 * 1)(64 * 80)
    cast = lambda a: [ctypes.cast(x, ctypes.c_void_p) if isinstance(x, ctypes.Array) else x for x in a]      # noqa: E731
    args = lambda **kw: cast([kw.get("slabs", slabs), fs, 1, kw.get("send", p16), 2,      # noqa: E731
                              (ctypes.c_uint64 * 2)(*kw.get("masks", (3, 1))), 2, 64, 80, kw.get("ld", 80),
                              kw.get("dtype", _lib.TF_BF16), None])
    assert lib.tf_frame_set_halo_pack(*args(dtype=_lib.TF_F32)) == -2
    assert lib.tf_frame_set_halo_pack(*args(send=ctypes.c_void_p((1 << 12) + 2))) == -4
    assert lib.tf_frame_set_halo_pack(*args(slabs=(ctypes.c_void_p * 1)((1 << 12) + 2))) == -4
    assert lib.tf_frame_set_halo_pack(*args(masks=(3, 4))) == -3 and b"at or above" in lib.tf_last_error()
    assert lib.tf_frame_set_halo_pack(*args(ld=84)) == -3
    assert lib.tf_frame_set_halo_pack(*args(masks=(0, 0))) == 0      # nothing to send: no launch


def test_workspace_is_never_below_the_windowed_one():
    """On a rank object without a communicator of W > 1 there is no device work to size; the arithmetic is checked through the
    plan geometry instead: the anchored exchange moves at least the windowed rows."""
    for K, W, R, anchors in ((7, 3, 1, (0,)), (25, 8, 2, (0, 8, 16, 24))):
        for r in range(W):
            a, w = sharded.frame_set_halo_plan(K, W, r, R, anchors), sharded.window_halo_plan(K, W, r, R)
            assert a.F >= w.F and all(x >= y for x, y in zip(a.send_rows, w.send_rows))


def test_python_refusals_and_signatures():
    import inspect
    for cls in (sharded.FrameShard, sharded.NativeShard, sharded.NativeEditShard):
        assert cls.supports_window_anchors
        for fn in (cls.pivotal_attention, cls.pivotal_block):
            assert "anchors" in inspect.signature(fn).parameters, (cls.__name__, fn.__name__)
    sh = sharded.FrameShard.__new__(sharded.FrameShard)
    sh.K, sh.Kl, sh.world = 8, 4, 2
    assert sh._anchors(None, None) == () and sh._anchors(1, ()) == () and sh._anchors(1, [3, 0, 3]) == (0, 3)
    with pytest.raises(ValueError, match="without window"):
        sh._anchors(None, (0,))
    with pytest.raises(ValueError, match="anchor"):
        sh._anchors(1, (8,))
    t = torch.zeros(3 * 4, 2, 16)
    with pytest.raises(ValueError, match="without window"):
        sh.pivotal_attention(t, t, t, 2, 1.0, False, anchors=(0,))
    with pytest.raises(ValueError, match="mode="):      # an explicit mode beside the window, as today
        sh.pivotal_attention(t, t, t, 2, 1.0, False, mode="heads", window=1, anchors=(0,))
    ed = sharded.NativeEditShard.__new__(sharded.NativeEditShard)
    ed.K, ed.Kl, ed.world = 8, 4, 2
    t = torch.zeros(5 * 4, 2, 16)
    with pytest.raises(ValueError, match="one edit"):
        ed.pivotal_attention(t, t, t, 2, 1.0, False, n_edits=2, inject_mask=0, window=1, anchors=(0,))
