"""Torch stand-ins for the two ops of an ANCHORED windowed frame shard (TEST INFRASTRUCTURE, beside
tests/shard_window_fake_ops.py and tests/frame_set_fake_ops.py): `frame_set_halo_pack` by indexing, `ext_attn_frame_sets_views`
as one plain `ext_attn` call per query frame on its member frames gathered in ascending order -- the definition of the
frame-set call -- while recording the calls."""
import torch

from tests.frame_set_fake_ops import FrameSetFakeOps
from tests.shard_window_fake_ops import ShardWindowFakeOps


def members(m):
    return [j for j in range(int(m).bit_length()) if (int(m) >> j) & 1]


class ShardFrameSetFakeOps(ShardWindowFakeOps, FrameSetFakeOps):
    def frame_set_halo_pack(self, slabs, masks, out=None):
        masks = tuple(int(m) for m in masks)
        self.calls.append(("frame_set_halo_pack", len(slabs), masks))
        Kl, S, D = slabs[0].shape
        assert all(m >= 0 and not m >> Kl for m in masks)
        frames = [f for m in masks for f in members(m)]
        res = torch.empty(len(frames), len(slabs), S, D, dtype=slabs[0].dtype)
        for r, f in enumerate(frames):
            for i, t in enumerate(slabs):
                res[r, i] = t[f]
        return res if out is None else out.copy_(res)

    def ext_attn_frame_sets_views(self, q, k, v, out, heads, scale, inject, sets, part="bank", branch0=(0, 0, 0, 0), q_frame0=0,
                                  no_split=None, stream=None, fused=None, hints=0):
        sets = tuple(int(m) for m in sets)
        self.calls.append(("ext_attn_frame_sets_views", tuple(q.shape), tuple(k.shape), bool(inject), sets, part, int(q_frame0)))
        assert part in ("bank", "all") and len(sets) == q.shape[1] and v.shape[1] == k.shape[1] <= 64
        S, D = k.shape[2], k.shape[3]
        computed = [1, 2] if part == "bank" else [0, 1, 2]

        def dense(t, b0, F):      # [3, F, S, D] with the slabs the call was not handed as readable zeros
            full = torch.zeros(3, F, S, D, dtype=t.dtype)
            full[b0:b0 + t.shape[0]] = t
            return full.view(3 * F, S, D)
        for i, m in enumerate(sets):
            own, fr = q_frame0 + i, members(m)
            assert fr and fr[-1] < k.shape[1] and own in fr
            res = self.ext_attn(dense(q[:, i:i + 1], branch0[0], 1), dense(k[:, fr], branch0[1], len(fr)),
                                dense(v[:, fr], branch0[2], len(fr)), heads, scale, inject, q_frame0=fr.index(own),
                                out_dtype=out.dtype).view(3, S, D)
            for b in computed:
                out[b - branch0[3], i] = res[b]
        return out
