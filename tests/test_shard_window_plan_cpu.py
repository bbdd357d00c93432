"""Sliding-window keyframe bank on a frame shard, host side (no GPU): the exchange geometry `sharded.window_halo_plan` against a
brute-force set computation, the native executor's recorded plan (tf_rank_pivotal_window_plan) against the geometry and the
composition of the two attention plans, the refusals, and the delegation of a covering radius to today's "bank" pass."""
import ctypes

import pytest
import torch

from tokenflow_amd import _lib, ops, sharded


def _own(K, W, p):
    counts = [K // W + (1 if r < K % W else 0) for r in range(W)]
    f0 = sum(counts[:p])
    return set(range(f0, f0 + counts[p]))


def _needs(K, W, r, R):
    """The frames the windows of rank r's keyframes name: the brute-force side."""
    need = set()
    for g in _own(K, W, r):
        need |= {f for f in range(K) if abs(f - g) <= R}
    return need


def test_geometry_against_sets():
    for K in range(1, 13):
        for W in range(1, K + 1):
            for R in range(0, K + 1):
                plans = [sharded.window_halo_plan(K, W, r, R) for r in range(W)]
                table = ops.bank_windows(K, R)
                for r, pl in enumerate(plans):
                    what = f"K={K} W={W} R={R} rank {r}"
                    own, need = _own(K, W, r), _needs(K, W, r, R)
                    assert set(range(pl.kf0, pl.kf0 + pl.Kl)) == own, what
                    # exactly the frames the local windows name arrive, in ascending order, and no others
                    got = [f for f0, n in pl.recv for f in range(f0, f0 + n)]
                    assert got == sorted(need) == list(range(pl.lo, pl.hi)), what
                    assert (pl.hl, pl.hr, pl.F) == (pl.kf0 - pl.lo, pl.hi - pl.kf0 - pl.Kl, len(need)), what
                    assert pl.recv_rows == [n for _, n in pl.recv] and pl.send_rows == [n for _, n in pl.send], what
                    assert pl.send[r] == (0, pl.Kl) and pl.recv[r] == (pl.kf0, pl.Kl), what      # the self rows
                    for p, other in enumerate(plans):
                        # what p sends to r is what r expects from p: the same global frames
                        f0, n = other.send[r]
                        sent = [other.kf0 + f for f in range(f0, f0 + n)]
                        g0, m = pl.recv[p]
                        assert sent == list(range(g0, g0 + m)) == sorted(_own(K, W, p) & need), what + f" peer {p}"
                    # local windows shifted back by lo are the rows of bank_windows(K, R); every query inside its window
                    assert [(w0 + pl.lo, n) for w0, n in pl.windows] == table[pl.kf0:pl.kf0 + pl.Kl], what
                    assert all(w0 <= pl.hl + i < w0 + n and w0 >= 0 and w0 + n <= pl.F
                               for i, (w0, n) in enumerate(pl.windows)), what
                    assert pl.F - pl.Kl <= 2 * R, what      # at most 2R remote frames


def test_geometry_refusals():
    for bad in ((4, 5, 0, 1), (4, 2, 2, 1), (4, 2, 0, -1), (4, 0, 0, 1)):
        with pytest.raises(ValueError):
            sharded.window_halo_plan(*bad)


def _rows(token):
    """'a2a[slabs=N,send=a/b,recv=c/d]' -> (N, [a, b], [c, d])"""
    body = dict(kv.split("=") for kv in token[len("a2a["):-1].split(","))
    return int(body["slabs"]), [int(x) for x in body["send"].split("/")], [int(x) for x in body["recv"].split("/")]


@pytest.mark.parametrize("K,W,R", [(5, 2, 1), (7, 3, 1), (7, 3, 2), (7, 3, 3), (25, 8, 2)])
@pytest.mark.parametrize("S,H,Dh", [(64, 2, 40), (320, 2, 64), (320, 1, 80), (1024, 5, 64)])
@pytest.mark.parametrize("inject", [False, True])
def test_native_plan_is_the_composition(K, W, R, S, H, Dh, inject):
    for r in range(W):
        pl = sharded.window_halo_plan(K, W, r, R)
        ns = 3 if inject else 4
        src = ops.attn_plan(pl.Kl, pl.Kl, S, H, Dh, inject, part="source", no_split=True)
        bank = ops.attn_windows_part_plan(pl.F, pl.Kl, pl.hl, pl.windows, S, H, Dh, inject, part="bank", no_split=True)
        assert any(t.endswith(",win") or t.endswith(",win]") for t in bank), bank
        for inv_norm in (False, True):
            got = sharded.rank_window_plan(W, r, K, S, H, Dh, R, inject=inject, inv_norm=inv_norm)
            head = (["inv_norm"] if inv_norm else []) + [f"halo_pack[ns={ns}]"]
            assert got[:len(head)] == head, got
            assert _rows(got[len(head)]) == (ns, pl.send_rows, pl.recv_rows), (got, pl)
            assert got[len(head) + 1:] == src + bank + ["halo[n=5]"], (got, src, bank)
        got = sharded.rank_window_plan(W, r, K, S, H, Dh, R, inject=inject, no_halo=True)
        assert got[2:] == src + bank, got


@pytest.mark.parametrize("K,W", [(5, 2), (7, 3)])
def test_covering_radius_is_the_bank_pass(K, W):
    for r in range(W):
        for inject in (False, True):
            want = sharded.rank_edits_plan(W, r, K, 320, 2, 40, 1, 1 if inject else 0, mode="bank")
            for R in (K - 1, K, 1000):
                assert sharded.rank_window_plan(W, r, K, 320, 2, 40, R, inject=inject) == want, (R, want)
            assert sharded.rank_window_plan(W, r, K, 320, 2, 40, K - 2, inject=inject) != want


def test_world_one_is_the_windowed_call():
    K, R = 6, 1
    assert (sharded.rank_window_plan(1, 0, K, 320, 2, 40, R)
            == ops.attn_windows_plan(K, ops.bank_windows(K, R), 320, 2, 40, False, no_split=True))
    assert sharded.rank_window_plan(1, 0, K, 320, 2, 40, K - 1) == ops.attn_plan(K, K, 320, 2, 40, False, no_split=True)


def test_full_windows_are_the_plain_part_call():
    K = 4
    full = [(0, K)] * 2
    assert (ops.attn_windows_part_plan(K, 2, 1, full, 320, 2, 40, True, no_split=True)
            == ops.attn_plan(K, 2, 320, 2, 40, True, part="bank", no_split=True))
    assert (ops.attn_windows_part_plan(K, K, 0, ops.bank_windows(K, 1), 320, 2, 40, False, part="all", no_split=True)
            == ops.attn_windows_plan(K, ops.bank_windows(K, 1), 320, 2, 40, False, no_split=True))


def _plan_rc(fn, *args):
    buf = ctypes.create_string_buffer(4096)
    return fn(*args, buf, len(buf))


def test_refusals():
    lib = _lib.load()
    K = 4
    lo, n = (ctypes.c_int * K)(0, 0, 1, 2), (ctypes.c_int * K)(2, 3, 3, 2)
    tab = (ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p))
    # tf_ext_attn_fwd_windows keeps refusing the part flags; the part entry point takes TF_ATTN_BANK_ONLY, not _SOURCE_ONLY
    for flag in (_lib.TF_ATTN_BANK_ONLY, _lib.TF_ATTN_SOURCE_ONLY):
        assert _plan_rc(lib.tf_ext_attn_windows_plan, K, K, 0, 320, 2, 40, flag, _lib.TF_BF16, *tab) < 0
        assert b"no windowed form" in lib.tf_last_error()
    assert _plan_rc(lib.tf_ext_attn_windows_part_plan, K, K, 0, 320, 2, 40, _lib.TF_ATTN_BANK_ONLY, _lib.TF_BF16, *tab) > 0
    assert _plan_rc(lib.tf_ext_attn_windows_part_plan, K, K, 0, 320, 2, 40, _lib.TF_ATTN_SOURCE_ONLY, _lib.TF_BF16, *tab) < 0
    with pytest.raises(ValueError):
        ops.attn_windows_part_plan(K, K, 0, ops.bank_windows(K, 1), 320, 2, 40, False, part="source")
    # the executor: a bad radius, more than TF_MAX_WINDOW_FRAMES local keyframes, a part flag, the heads mode
    assert _plan_rc(lib.tf_rank_pivotal_window_plan, 2, 0, 5, 320, 2, 40, -1, _lib.TF_RANK_BANK, 0, _lib.TF_BF16) < 0
    assert b"radius" in lib.tf_last_error()
    Kl = _lib.TF_MAX_WINDOW_FRAMES + 1
    assert _plan_rc(lib.tf_rank_pivotal_window_plan, 2, 0, 2 * Kl, 64, 2, 40, 1, _lib.TF_RANK_BANK, 0, _lib.TF_BF16) < 0
    assert b"local keyframes" in lib.tf_last_error()
    assert _plan_rc(lib.tf_rank_pivotal_window_plan, 2, 0, 2 * Kl - 2, 64, 2, 40, 1, _lib.TF_RANK_BANK, 0, _lib.TF_BF16) > 0
    assert _plan_rc(lib.tf_rank_pivotal_window_plan, 2, 0, 5, 320, 2, 40, 1, _lib.TF_RANK_BANK, _lib.TF_ATTN_BANK_ONLY,
                    _lib.TF_BF16) < 0
    assert _plan_rc(lib.tf_rank_pivotal_window_plan, 2, 0, 5, 320, 2, 40, 1, _lib.TF_RANK_BANK_RUNS, 0, _lib.TF_BF16) < 0
    # the pack entry point refuses before any launch: dtype, alignment, a segment outside the local frames
    p16 = ctypes.c_void_p(1 << 12)
    slabs, fs = (ctypes.c_void_p * 1)(1 << 12), (ctypes.c_int64 * 1)(64 * 80)
    seg0, segn = (ctypes.c_int * 2)(0, 1), (ctypes.c_int * 2)(2, 1)
    args = lambda **kw: [kw.get("slabs", slabs), fs, 1, kw.get("send", p16), 2, seg0, kw.get("segn", segn), 2, 64, 80,  # noqa: E731
                         kw.get("ld", 80), kw.get("dtype", _lib.TF_BF16), None]
    cast = lambda a: [ctypes.cast(x, ctypes.c_void_p) if isinstance(x, ctypes.Array) else x for x in a]      # noqa: E731
    TF_ERR_DTYPE, TF_ERR_SHAPE, TF_ERR_ALIGN = -2, -3, -4      # include/tokenflow_hip.h
    assert lib.tf_window_halo_pack(*cast(args(dtype=_lib.TF_F32))) == TF_ERR_DTYPE
    assert lib.tf_window_halo_pack(*cast(args(send=ctypes.c_void_p((1 << 12) + 2)))) == TF_ERR_ALIGN
    assert lib.tf_window_halo_pack(*cast(args(segn=(ctypes.c_int * 2)(2, 2)))) == TF_ERR_SHAPE
    assert b"outside" in lib.tf_last_error()
    assert lib.tf_window_halo_pack(*cast(args(ld=84))) == TF_ERR_SHAPE


def test_python_refusals():
    sh = sharded.FrameShard.__new__(sharded.FrameShard)
    sh.K, sh.Kl, sh.world = 8, 4, 2
    assert sh._window(None) is None and sh._window(7) is None and sh._window(100, n_edits=3) is None
    assert sh._window(2) == 2
    with pytest.raises(ValueError):
        sh._window(2, n_edits=2)
    with pytest.raises(ValueError):
        sh._window(-1)
    with pytest.raises(ValueError):
        sh._window(2, mode="heads")      # the windowed pass has one exchange pattern: an explicit mode is not ignored
    assert sh._window(7, mode="heads") is None


def test_every_shard_type_that_reports_window_support_takes_the_keyword():
    """The hooks hand `window=` to any shard whose type says `supports_window`: every such class of the package takes it in both
    entry points (`NativeEditShard` with one edit is `NativeShard`'s windowed pass; with several it raises ValueError)."""
    import inspect
    for cls in (sharded.FrameShard, sharded.NativeShard, sharded.NativeEditShard):
        assert cls.supports_window
        for fn in (cls.pivotal_attention, cls.pivotal_block):
            assert "window" in inspect.signature(fn).parameters, (cls.__name__, fn.__name__)
    ed = sharded.NativeEditShard.__new__(sharded.NativeEditShard)
    ed.K, ed.Kl, ed.world = 8, 4, 2
    t = torch.zeros(5 * 4, 2, 16)
    for call in (lambda: ed.pivotal_attention(t, t, t, 2, 1.0, False, n_edits=2, inject_mask=0, window=1),
                 lambda: ed.pivotal_block(t, t, t, 2, 1.0, False, None, n_edits=2, inject_mask=0, window=1)):
        with pytest.raises(ValueError, match="one edit"):
            call()
