"""Every copy and row kernel whose launcher caps its grid, run past the cap: the grid-stride loop takes a second trip (and a
ragged last one) as it does at the model's real sizes.

The payloads are index-coded: an int32 counter over the whole source, viewed as the tensor's dtype, compared as integers -- a
16-byte piece that lands in the wrong place names the piece it came from.  Each test asserts the launch arithmetic that makes
it stride (pieces, cap, trips) with the cap quoted from the launcher.

  * tf_inject_copy, tf_inject_copy_edits (E = 3), tf_inject_copy_edits_masked (mask 0b101: the other edit's branches untouched);
  * tf_head_pack (six slabs, and seven: the wide parameter block) / tf_head_unpack, strided source slabs;
  * tf_window_halo_pack; tf_frame_set_halo_pack and tf_edit_halo_pack with so many send rows that a row's few workgroups stride
    over it (the q staging of the edit form as well);
  * tf_pivot_inv_norm on the exact family of tests/ln_exact.py: 1/||row|| bit equal to the IEEE fp32 1 / sqrt(ss).

tf_ddim_step and the gather kernels stride in tests of their own (tests/test_kernels_gpu.py, tests/test_nn_exact_gpu.py)."""
import math

import pytest
import torch

from tests import ln_exact as lx

pytestmark = pytest.mark.gpu

INJECT_CAP = 256 * 8       # gather_blend.hip:732 (tf_inject_copy) and :757 (inject_copy_edits_impl): workgroups of 256 pieces
HEAD_CAP = 256 * 16        # head_exchange.hip:221 (tf_head_pack) and :243 (tf_head_unpack): workgroups of 256 pieces
WINDOW_CAP = 2048          # head_exchange.hip:293 (tf_window_halo_pack): workgroups of 256 pieces
SET_WGS = 2048             # head_exchange.hip:333 (tf_frame_set_halo_pack) and :437 (tf_edit_halo_pack): ny = ceil(2048 / columns)
PIVOT_CAP = 4096           # nn_search.hip:1324 (tf_pivot_inv_norm): workgroups of 4 rows


def _ops():
    from tokenflow_amd import ops
    return ops


def _coded(shape, dtype, start=0):
    """An int32 counter (from `start`) over a contiguous tensor of `shape`, viewed as `dtype`."""
    per = 4 // torch.empty((), dtype=dtype).element_size()
    n = math.prod(shape)
    assert n % per == 0
    return torch.arange(start, start + n // per, dtype=torch.int32, device="cuda").view(dtype).view(shape)


def _ints(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _assert_pieces(got, want, what):
    """Bit equality of two tensors of one shape; a failure names the first wrong 16-byte piece and the source piece found there."""
    g, w = _ints(got.contiguous()).flatten().view(torch.int32), _ints(want.contiguous()).flatten().view(torch.int32)
    if not torch.equal(g, w):
        bad = (g != w).nonzero().flatten()
        i = int(bad[0])
        pytest.fail(f"{what}: {bad.numel()} of {w.numel()} words differ; first in piece {i // 4} of {w.numel() // 4}: holds word "
                    f"{int(g[i])} (source piece {int(g[i]) // 4}), wants word {int(w[i])} (source piece {int(w[i]) // 4})")


# ------------------------------------------------------------------------------------------------------------ inject copies
@pytest.mark.parametrize("form", ["plain", "edits", "masked"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_inject_copies_past_the_grid_cap(form, dtype):
    ops = _ops()
    pieces = 2 * INJECT_CAP * 256 + 3 * 256 + 5        # per branch: two full trips, three full workgroups, a ragged one
    trips = -(-pieces // (INJECT_CAP * 256))
    assert pieces > INJECT_CAP * 256 and trips == 3
    nbr = 3 if form == "plain" else 7                   # E = 3
    per_branch = pieces * 16 // torch.empty((), dtype=dtype).element_size()
    x = _coded((nbr, per_branch), dtype)
    before = x.clone()
    assert x.numel() * x.element_size() == nbr * pieces * 16
    if form == "plain":
        out, takes = ops.inject_copy_(x), [1, 2]
    elif form == "edits":
        out, takes = ops.inject_copy_edits_(x, 3), [1, 2, 3, 4, 5, 6]
    else:
        out, takes = ops.inject_copy_edits_(x, 3, edit_mask=0b101), [1, 2, 5, 6]
    assert out is x
    for b in range(nbr):
        _assert_pieces(x[b], before[0 if b in takes else b], f"inject copy ({form}, {dtype}) branch {b}")


# ------------------------------------------------------------------------------------------------------- head pack / unpack
def test_head_pack_unpack_past_the_grid_cap():
    """(W 8, Kl 2, S 4096, D 320, bf16), column slabs of a fused projection output as in test_head_pack_unpack, against the same
    torch re-layout.  Six slabs are 1966080 pieces: two trips, the second partial; seven take the wide parameter block.  Two
    unpacked slabs (the model's call) stay under the cap, four stride."""
    ops = _ops()
    W, Kl, S, D, dtype = 8, 2, 4096, 320, torch.bfloat16
    hd = D // W
    hd_pieces = hd * 2 // 16
    fused = _coded((3 * Kl, S, 3 * D), dtype)
    q3, k3, v3 = (fused[..., i * D:(i + 1) * D].unflatten(0, (3, Kl)) for i in range(3))
    six = [q3[1], q3[2], k3[1], k3[2], v3[1], v3[2]]
    for slabs in (six, six + [q3[0]]):
        ns = len(slabs)
        pieces = W * Kl * ns * S * hd_pieces
        assert pieces > HEAD_CAP * 256 and -(-pieces // (HEAD_CAP * 256)) >= 2 and (ns != 6 or pieces == 1966080)
        send = ops.head_pack(slabs, W)
        want = torch.stack([_ints(t).reshape(Kl, S, W, hd) for t in slabs], dim=1).permute(3, 0, 1, 2, 4)
        assert send.shape == (W, Kl, ns, S, hd)
        _assert_pieces(send, want, f"head_pack of {ns} slabs")
    for nb in (2, 4):
        pieces = W * Kl * nb * S * hd_pieces
        assert (pieces > HEAD_CAP * 256 and -(-pieces // (HEAD_CAP * 256)) == 2) if nb == 4 else pieces == 655360
        recv = _coded((W, Kl, nb, S, hd), dtype, start=1 << 24)
        out = torch.zeros(nb + 1, Kl, S, D, dtype=dtype, device="cuda")
        ops.head_unpack(recv, [out[1 + i] for i in range(nb)])
        _assert_pieces(out[1:].view(nb, Kl, S, W, hd), _ints(recv).permute(2, 1, 3, 0, 4), f"head_unpack of {nb} slabs")
        assert bool((_ints(out[0]) == 0).all())


# ---------------------------------------------------------------------------------------------------------------- halo packs
def test_window_halo_pack_past_the_grid_cap():
    ops = _ops()
    Kl, S, D = 3, 512, 320
    qkv = _coded((3, Kl, S, 3 * D), torch.bfloat16)
    k3, v3 = qkv[..., D:2 * D], qkv[..., 2 * D:]
    slabs = [k3[1], k3[2], v3[1], v3[2]]
    segs = [(0, 3), (1, 2), (0, 0), (2, 1), (0, 1)]      # 7 send rows: frames in several segments, an empty peer
    frames = [f for f0, n in segs for f in range(f0, f0 + n)]
    pieces = len(frames) * len(slabs) * S * (D * 2 // 16)
    assert len(frames) == 7 and pieces == 573440 and pieces > WINDOW_CAP * 256 and -(-pieces // (WINDOW_CAP * 256)) == 2
    got = ops.window_halo_pack(slabs, segs)
    want = torch.stack([torch.stack([_ints(s)[f] for s in slabs]) for f in frames])
    assert got.shape == (7, 4, S, D)
    _assert_pieces(got, want, "window_halo_pack")


def _pack_want(slabs, masks):
    frames = [f for m in masks for f in range(64) if (m >> f) & 1]
    return frames, torch.stack([torch.stack([_ints(s)[f] for s in slabs]) for f in frames])


def _set_slabs(ns, Kl, S, D):
    """ns strided [Kl, S, D] views (frame stride != S * ld, ld > D) of index-coded buffers, as test_frame_set_halo_pack."""
    buf = _coded((ns, Kl + 1, S + 2, 2 * D), torch.bfloat16)
    slabs = [buf[i, :Kl, 1:1 + S, D * (i % 2):D * (i % 2) + D] for i in range(ns)]
    assert slabs[0].stride(0) != S * slabs[0].stride(1) and slabs[0].stride(1) > D
    return slabs


def test_frame_set_halo_pack_rows_stride():
    """80 send rows leave ny = ceil(2048 / 80) = 26 workgroups per row of 3 * 300 * 40 = 36000 pieces: six trips of the y loop."""
    ops = _ops()
    Kl, S, D, ns = 5, 300, 320, 3
    masks = [0b11111] * 16
    rows = sum(bin(m).count("1") for m in masks)
    per_row = ns * S * (D * 2 // 16)
    ny = min(-(-SET_WGS // rows), -(-per_row // 256))
    assert rows == 80 and ny == 26 and per_row == 36000 and -(-per_row // (ny * 256)) == 6
    slabs = _set_slabs(ns, Kl, S, D)
    got = ops.frame_set_halo_pack(slabs, masks)
    frames, want = _pack_want(slabs, masks)
    assert got.shape == (rows, ns, S, D)
    _assert_pieces(got, want, "frame_set_halo_pack")


def test_edit_halo_pack_rows_and_q_staging_stride():
    """80 send rows and 2 * 5 q columns leave ny = ceil(2048 / 90) = 23 workgroups per column: the rows of 36000 pieces take seven
    trips, the q frames of 300 * 40 = 12000 pieces three."""
    ops = _ops()
    Kl, S, D, ns, nq = 5, 300, 320, 3, 2
    masks = [0b11111] * 15 + [0b01111, 0b10000]       # a non-full peer; 80 rows in all
    rows = sum(bin(m).count("1") for m in masks)
    cols = rows + nq * Kl
    per_row, per_q = ns * S * (D * 2 // 16), S * (D * 2 // 16)
    ny = min(-(-SET_WGS // cols), -(-per_row // 256))
    assert rows == 80 and ny == 23 and -(-per_row // (ny * 256)) == 7 and per_q > ny * 256 and -(-per_q // (ny * 256)) == 3
    slabs = _set_slabs(ns, Kl, S, D)
    qbuf = _coded((nq, Kl, S + 1, 2 * D), torch.bfloat16, start=1 << 26)
    qs = [qbuf[i, :, :S, D:] for i in range(nq)]
    got, stage = ops.edit_halo_pack(slabs, masks, qs)
    frames, want = _pack_want(slabs, masks)
    assert got.shape == (rows, ns, S, D) and stage.shape == (nq, Kl, S, D)
    _assert_pieces(got, want, "edit_halo_pack")
    _assert_pieces(stage, torch.stack([_ints(t) for t in qs]), "edit_halo_pack q staging")


# ------------------------------------------------------------------------------------------------------------ pivot norms
@pytest.mark.parametrize("D", [8, 520])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_pivot_inv_norm_past_the_grid_cap(D, dtype):
    """rows = 2 * 16384 + 3: three trips of a wave's row loop, the last of 3 rows; D = 520 is a second pass over the row with 63
    idle lanes.  Rows a_r * (k_r + s) of tests/ln_exact.py: sum of squares a_r^2 * D * (k_r^2 + 1), an exact fp32 value in
    every order, so 1/||row|| is one IEEE square root and one IEEE division (lx.inv_sqrt32)."""
    ops = _ops()
    rows = 2 * PIVOT_CAP * 4 + 3
    assert rows > PIVOT_CAP * 4 and -(-rows // (PIVOT_CAP * 4)) == 3
    fam = lx.make(D, rows, "scaled", device="cuda")
    x, a, k = fam["x"], fam["a"], fam["k"]
    ss = (x * x).sum(1)
    assert torch.equal(ss, a * a * D * (k * k + 1).double()) and float((ss / (a * a)).max()) < 2 ** 24
    assert float((ss[:-PIVOT_CAP * 4] != ss[PIVOT_CAP * 4:]).double().mean()) > 0.9      # a row of the wrong trip shows
    inv = ops.pivot_inv_norm(x.to(dtype))
    want = lx.inv_norm_expected(ss)
    got = inv.cpu()
    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero().flatten()
        r = int(bad[0])
        pytest.fail(f"pivot_inv_norm D={D} {dtype}: {bad.numel()} of {rows} rows differ from the IEEE fp32 1/sqrt(ss); first: row {r} "
                    f"(trip {r // (PIVOT_CAP * 4)}) ss {float(ss[r])} got {float(got[r]).hex()} want {float(want[r]).hex()}")
