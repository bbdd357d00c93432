"""Oracle-backed stand-in for the sliding-window attention op of a multi-edit batch (TEST INFRASTRUCTURE, beside
tests/window_fake_ops.py and tests/edit_schedule_forms.py): edit e's slices of keyframe i are, by definition, what the plain op
computes for that keyframe on window i's tensors of [source | uncond_e | cond_e] with edit e's injection flag -- that is what
this computes, from the plain FakeOps, while recording the calls the hooks make."""
import torch

from tests import edit_forms as ef
from tests.edit_schedule_forms import ScheduleEditFakeOps, mask_bits
from tests.fake_ops import FakeOps
from tests.window_fake_ops import bank_windows


class WindowEditFakeOps(ScheduleEditFakeOps):
    bank_windows = staticmethod(bank_windows)

    def ext_attn_windows_edits(self, q, k, v, heads, scale, inject, n_edits, windows, *, inject_mask=None, multi_v=None,
                               multi_v64=None, no_split=None, fused=None, hints=0, out_dtype=None, out=None):
        E = int(n_edits)
        windows = tuple((int(lo), int(n)) for lo, n in windows)
        mask = ((1 << E) - 1 if inject else 0) if inject_mask is None else int(inject_mask)
        assert inject_mask is None or not inject
        assert 0 <= mask < (1 << E)
        self.calls.append(("ext_attn_windows_edits", tuple(q.shape), E, mask, windows))
        B = 1 + 2 * E
        K, S, D = k.shape[0] // B, k.shape[1], k.shape[2]
        assert len(windows) == K and q.shape == k.shape == v.shape and k.shape[0] == B * K
        res = torch.empty(q.shape, dtype=torch.float32 if out_dtype == torch.float32 else q.dtype)
        for e, inj in enumerate(mask_bits(mask, E)):
            q3, k3, v3 = (ef.edit_slice(t, e, E).reshape(3, K, S, D) for t in (q, k, v))
            o3 = torch.empty(3, K, S, D, dtype=res.dtype)
            for i, (lo, n) in enumerate(windows):
                assert n >= 1 and 0 <= lo <= i < lo + n <= K
                o, _ = self._quiet(FakeOps.ext_attn, self, q3[:, i:i + 1].reshape(3, S, D), k3[:, lo:lo + n].reshape(3 * n, S, D),
                                   v3[:, lo:lo + n].reshape(3 * n, S, D), heads, scale, inj, q_frame0=i - lo, out_dtype=out_dtype)
                o3[:, i] = o
            ef.edit_scatter(res, o3.view(3 * K, S, D), e, E)      # the source branch is the same whatever the edit's flag
        return res if out is None else out.copy_(res)
