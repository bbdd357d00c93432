"""Oracle-backed stand-in for the frame-set attention op of `tokenflow_amd.ops` (TEST INFRASTRUCTURE, beside
tests/window_fake_ops.py): keyframe i's slices of a frame-set call are, by definition, what the plain op computes for that
keyframe on the member frames of set i gathered next to each other in ascending order -- that is what this computes, from the
plain FakeOps, while recording the calls the hooks make."""
import torch

from tests.segment_fake_ops import SegmentFakeOps
from tests.window_fake_ops import WindowFakeOps


def bank_frame_sets(K, radius, anchors=()):
    """Window plus anchors as one int mask per keyframe, written out independently of `ops.bank_frame_sets`."""
    anchors = list(anchors)
    if any(not 0 <= a < K for a in anchors):
        raise ValueError(f"bank_frame_sets: anchors {anchors} outside [0, {K})")
    return [sum(1 << f for f in range(K) if abs(f - i) <= radius or f in anchors) for i in range(K)]


class FrameSetFakeOps(WindowFakeOps):
    bank_frame_sets = staticmethod(bank_frame_sets)

    def ext_attn_frame_sets(self, q, k, v, heads, scale, inject, sets, *, no_split=None, fused=None, hints=0, out_dtype=None,
                            out=None):
        sets = tuple(int(m) for m in sets)
        self.calls.append(("ext_attn_frame_sets", tuple(q.shape), bool(inject), sets))
        K, S, D = k.shape[0] // 3, k.shape[1], k.shape[2]
        assert len(sets) == K and q.shape == k.shape == v.shape
        res = torch.empty(3, K, S, D, dtype=torch.float32 if out_dtype == torch.float32 else q.dtype)
        inner = SegmentFakeOps(self.round16)
        for i, m in enumerate(sets):
            frames = [f for f in range(K) if (m >> f) & 1]
            assert m > 0 and not m >> K and i in frames
            kw, vw = (t.reshape(3, K, S, D)[:, frames].reshape(3 * len(frames), S, D) for t in (k, v))
            qi = q.reshape(3, K, S, D)[:, i:i + 1].reshape(3, S, D)
            res[:, i] = inner.ext_attn(qi, kw, vw, heads, scale, inject, q_frame0=frames.index(i), out_dtype=out_dtype)
        res = res.view(3 * K, S, D)
        return res if out is None else out.copy_(res)
