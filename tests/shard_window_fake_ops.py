"""Torch stand-ins for the two ops of a windowed frame shard (TEST INFRASTRUCTURE, beside tests/window_fake_ops.py):
`window_halo_pack` by indexing, `ext_attn_windows_views` as one plain `ext_attn` call per query frame on its window's
frames -- the definition of the windowed call -- while recording the calls."""
import torch

from tests.window_fake_ops import WindowFakeOps


class ShardWindowFakeOps(WindowFakeOps):
    def window_halo_pack(self, slabs, segments, out=None):
        segments = [(int(f0), int(n)) for f0, n in segments]
        self.calls.append(("window_halo_pack", len(slabs), tuple(segments)))
        Kl, S, D = slabs[0].shape
        assert all(0 <= f0 and n >= 0 and f0 + n <= Kl for f0, n in segments)
        frames = [f for f0, n in segments for f in range(f0, f0 + n)]
        res = torch.empty(len(frames), len(slabs), S, D, dtype=slabs[0].dtype)
        for r, f in enumerate(frames):
            for i, t in enumerate(slabs):
                res[r, i] = t[f]
        return res if out is None else out.copy_(res)

    def ext_attn_windows_views(self, q, k, v, out, heads, scale, inject, windows, part="bank", branch0=(0, 0, 0, 0), q_frame0=0,
                               no_split=None, stream=None, fused=None, hints=0):
        windows = tuple((int(lo), int(n)) for lo, n in windows)
        self.calls.append(("ext_attn_windows_views", tuple(q.shape), tuple(k.shape), bool(inject), windows, part, int(q_frame0)))
        assert part in ("bank", "all") and len(windows) == q.shape[1] and v.shape[1] == k.shape[1]
        S, D = k.shape[2], k.shape[3]
        computed = [1, 2] if part == "bank" else [0, 1, 2]

        def dense(t, b0, F):      # [3, F, S, D] with the slabs the call was not handed as readable zeros
            full = torch.zeros(3, F, S, D, dtype=t.dtype)
            full[b0:b0 + t.shape[0]] = t
            return full.view(3 * F, S, D)
        for i, (lo, n) in enumerate(windows):
            own = q_frame0 + i
            assert n >= 1 and 0 <= lo <= own < lo + n <= k.shape[1]
            res = self.ext_attn(dense(q[:, i:i + 1], branch0[0], 1), dense(k[:, lo:lo + n], branch0[1], n),
                                dense(v[:, lo:lo + n], branch0[2], n), heads, scale, inject, q_frame0=own - lo,
                                out_dtype=out.dtype).view(3, S, D)
            for b in computed:
                out[b - branch0[3], i] = res[b]
        return out
