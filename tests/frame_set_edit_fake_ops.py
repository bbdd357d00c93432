"""Oracle-backed stand-in for the frame-set attention op of a multi-edit batch (TEST INFRASTRUCTURE, beside
tests/window_edit_fake_ops.py and tests/frame_set_fake_ops.py): edit e's slices of keyframe i are, by definition, what the plain
op computes for that keyframe on the member frames of set i of [source | uncond_e | cond_e], gathered in ascending order, with
edit e's injection flag -- that is what this computes, from the plain FakeOps, while recording the calls the hooks make."""
import torch

from tests import edit_forms as ef
from tests.edit_schedule_forms import mask_bits
from tests.fake_ops import FakeOps
from tests.frame_set_fake_ops import bank_frame_sets
from tests.window_edit_fake_ops import WindowEditFakeOps


class FrameSetEditFakeOps(WindowEditFakeOps):
    bank_frame_sets = staticmethod(bank_frame_sets)

    def ext_attn_frame_sets_edits(self, q, k, v, heads, scale, inject, n_edits, sets, *, inject_mask=None, multi_v=None,
                                  multi_v64=None, no_split=None, fused=None, hints=0, out_dtype=None, out=None):
        E = int(n_edits)
        sets = tuple(int(m) for m in sets)
        mask = ((1 << E) - 1 if inject else 0) if inject_mask is None else int(inject_mask)
        assert inject_mask is None or not inject
        assert 0 <= mask < (1 << E)
        self.calls.append(("ext_attn_frame_sets_edits", tuple(q.shape), E, mask, sets))
        B = 1 + 2 * E
        K, S, D = k.shape[0] // B, k.shape[1], k.shape[2]
        assert len(sets) == K and q.shape == k.shape == v.shape and k.shape[0] == B * K
        res = torch.empty(q.shape, dtype=torch.float32 if out_dtype == torch.float32 else q.dtype)
        for e, inj in enumerate(mask_bits(mask, E)):
            q3, k3, v3 = (ef.edit_slice(t, e, E).reshape(3, K, S, D) for t in (q, k, v))
            o3 = torch.empty(3, K, S, D, dtype=res.dtype)
            for i, m in enumerate(sets):
                frames = [f for f in range(K) if (m >> f) & 1]
                assert m > 0 and not m >> K and i in frames
                n = len(frames)
                o, _ = self._quiet(FakeOps.ext_attn, self, q3[:, i:i + 1].reshape(3, S, D), k3[:, frames].reshape(3 * n, S, D),
                                   v3[:, frames].reshape(3 * n, S, D), heads, scale, inj, q_frame0=frames.index(i),
                                   out_dtype=out_dtype)
                o3[:, i] = o
            ef.edit_scatter(res, o3.view(3 * K, S, D), e, E)      # the source branch is the same whatever the edit's flag
        return res if out is None else out.copy_(res)
