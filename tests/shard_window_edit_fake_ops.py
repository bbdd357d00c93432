"""Torch stand-ins for the ops a windowed / anchored frame shard issues for a MULTI-EDIT batch (TEST INFRASTRUCTURE, imported by
tests/test_shard_window_edits_cpu.py; beside tests/shard_edit_ops.py, tests/shard_frame_set_fake_ops.py and
tests/frame_set_edit_fake_ops.py): `edit_halo_pack` by indexing, `ext_attn_windows_edits_views` /
`ext_attn_frame_sets_edits_views` as one call of the SINGLE-EDIT stand-in view per edit, on that edit's slabs with that edit's
flag -- the definition of the multi-edit part -- while recording the calls."""
import torch

from tests.frame_set_edit_fake_ops import FrameSetEditFakeOps
from tests.shard_edit_ops import ShardEditFakeOps
from tests.shard_frame_set_fake_ops import ShardFrameSetFakeOps, members


class ShardWindowEditFakeOps(ShardEditFakeOps, FrameSetEditFakeOps, ShardFrameSetFakeOps):
    def edit_halo_pack(self, slabs, masks, q_slabs=(), out=None, q_out=None):
        masks = tuple(int(m) for m in masks)
        self.calls.append(("edit_halo_pack", len(slabs), len(q_slabs), masks))
        Kl, S, D = slabs[0].shape
        assert all(m >= 0 and not m >> Kl for m in masks) and len(slabs) <= 32 and len(q_slabs) <= 17
        frames = [f for m in masks for f in members(m)]
        res = torch.empty(len(frames), len(slabs), S, D, dtype=slabs[0].dtype)
        for r, f in enumerate(frames):
            for i, t in enumerate(slabs):
                res[r, i] = t[f]
        stage = torch.stack(list(q_slabs)) if len(q_slabs) else None
        if stage is not None and q_out is not None:
            stage = q_out.copy_(stage)
        return (res if out is None else out.copy_(res)), stage

    def _edits_table_views(self, name, single, q, k, v, out, heads, scale, n_edits, inject_mask, table, part, qk_compact, branch0,
                           q_frame0):
        E, mask = int(n_edits), int(inject_mask)
        assert 0 <= mask < (1 << E) and part == "bank", "the shard issues the bank part (the source part is table-free)"
        self.calls.append((name, tuple(q.shape), tuple(k.shape), E, mask, tuple(table), part, bool(qk_compact), int(q_frame0)))

        def br(t, i, lo, n=2):      # branches [lo, lo + n) of the tensor whose view `t` starts at branch branch0[i]
            a = lo - branch0[i]
            assert 0 <= a and a + n <= t.shape[0], f"the view does not hold branches [{lo}, {lo + n})"
            return t[a:a + n]
        n_non = 0
        for e in range(E):
            lo = 1 + 2 * e
            if (mask >> e) & 1:
                self._quiet(single, q=br(q, 0, 0, 1), k=br(k, 1, 0, 1), v=br(v, 2, lo), out=br(out, 3, lo), heads=heads,
                            scale=scale, inject=True, part="bank", branch0=(0, 0, 1, 1), q_frame0=q_frame0)
            else:
                slot = 1 + 2 * n_non if qk_compact else lo
                n_non += 1
                self._quiet(single, q=br(q, 0, slot), k=br(k, 1, slot), v=br(v, 2, lo), out=br(out, 3, lo), heads=heads,
                            scale=scale, inject=False, part="bank", branch0=(1, 1, 1, 1), q_frame0=q_frame0)
        return out

    def ext_attn_windows_edits_views(self, q, k, v, out, heads, scale, n_edits, inject_mask, windows, part="bank",
                                     qk_compact=False, branch0=(0, 0, 0, 0), q_frame0=0, no_split=None, fused=None,
                                     multi_v=None, hints=0, stream=None, multi_v64=None):
        windows = tuple((int(lo), int(n)) for lo, n in windows)
        single = lambda **kw: self.ext_attn_windows_views(windows=windows, **kw)      # noqa: E731
        return self._edits_table_views("ext_attn_windows_edits_views", single, q, k, v, out, heads, scale, n_edits, inject_mask,
                                       windows, part, qk_compact, branch0, q_frame0)

    def ext_attn_frame_sets_edits_views(self, q, k, v, out, heads, scale, n_edits, inject_mask, sets, part="bank",
                                        qk_compact=False, branch0=(0, 0, 0, 0), q_frame0=0, no_split=None, fused=None,
                                        multi_v=None, hints=0, stream=None, multi_v64=None):
        sets = tuple(int(m) for m in sets)
        single = lambda **kw: self.ext_attn_frame_sets_views(sets=sets, **kw)      # noqa: E731
        return self._edits_table_views("ext_attn_frame_sets_edits_views", single, q, k, v, out, heads, scale, n_edits,
                                       inject_mask, sets, part, qk_compact, branch0, q_frame0)
