"""Oracle-backed stand-in for the sliding-window attention op of `tokenflow_amd.ops` (TEST INFRASTRUCTURE, beside
tests/fake_ops.py and tests/segment_fake_ops.py): keyframe i's slices of a windowed call are, by definition, what the plain op
computes for that keyframe on window i's tensors alone -- that is what this computes, from the plain FakeOps, while recording
the calls the hooks make."""
import torch

from tests.segment_fake_ops import SegmentFakeOps


def bank_windows(K, radius):
    """The clamped symmetric windows, written out independently of `ops.bank_windows`."""
    out = []
    for i in range(K):
        frames = [f for f in range(K) if abs(f - i) <= radius]
        out.append((frames[0], len(frames)))
    return out


class WindowFakeOps(SegmentFakeOps):
    bank_windows = staticmethod(bank_windows)

    def ext_attn_windows(self, q, k, v, heads, scale, inject, windows, *, no_split=None, fused=None, hints=0, out_dtype=None,
                         out=None):
        windows = tuple((int(lo), int(n)) for lo, n in windows)
        self.calls.append(("ext_attn_windows", tuple(q.shape), bool(inject), windows))
        K, S, D = k.shape[0] // 3, k.shape[1], k.shape[2]
        assert len(windows) == K and q.shape == k.shape == v.shape
        res = torch.empty(3, K, S, D, dtype=torch.float32 if out_dtype == torch.float32 else q.dtype)
        inner = SegmentFakeOps(self.round16)
        for i, (lo, n) in enumerate(windows):
            assert n >= 1 and 0 <= lo <= i < lo + n <= K
            kw, vw = (t.reshape(3, K, S, D)[:, lo:lo + n].reshape(3 * n, S, D) for t in (k, v))
            qi = q.reshape(3, K, S, D)[:, i:i + 1].reshape(3, S, D)
            res[:, i] = inner.ext_attn(qi, kw, vw, heads, scale, inject, q_frame0=i - lo, out_dtype=out_dtype)
        res = res.view(3 * K, S, D)
        return res if out is None else out.copy_(res)
