"""Oracle-backed stand-ins for the keyframe-segment ops of `tokenflow_amd.ops` (TEST INFRASTRUCTURE, beside tests/fake_ops.py):
a segmented op is, by definition, the single-clip op on every segment's tensors alone -- that is what these compute, from the
plain FakeOps, while recording the calls the hooks make."""
import torch

from tests.fake_ops import FakeOps


class SegmentFakeOps(FakeOps):
    def ext_attn_segments(self, q, k, v, heads, scale, inject, segments, out=None, out_dtype=None, no_split=None):
        segments = tuple(int(s) for s in segments)
        self.calls.append(("ext_attn_segments", tuple(q.shape), bool(inject), segments))
        K, S, D = k.shape[0] // 3, k.shape[1], k.shape[2]
        assert sum(segments) == K and q.shape == k.shape == v.shape
        res = torch.empty(3, K, S, D, dtype=torch.float32 if out_dtype == torch.float32 else q.dtype)
        inner = FakeOps(self.round16)
        f0 = 0
        for Kv in segments:
            win = [t.reshape(3, K, S, D)[:, f0:f0 + Kv].reshape(3 * Kv, S, D) for t in (q, k, v)]
            res[:, f0:f0 + Kv] = inner.ext_attn(*win, heads, scale, inject, out_dtype=out_dtype).view(3, Kv, S, D)
            f0 += Kv
        res = res.view(3 * K, S, D)
        return res if out is None else out.copy_(res)

    def propagate_chunks_segments(self, tgt, piv, inv_norm, kf_out, w, n, n_chunks, slot0, single_mask, residual, out_dtype,
                                  norm=None):
        """Chunk j of the run = one `propagate`: slot0 + j alone where bit j is set, else slots [slot0 + j, slot0 + j - 1]."""
        self.calls.append(("propagate_chunks_segments", tuple(tgt.shape), int(n_chunks), int(slot0), int(single_mask)))
        assert n_chunks > 1 and not single_mask >> n_chunks
        S, D = piv.shape[1:]
        res = residual.view(3, n_chunks, n, S, D) if residual is not None else None
        inner = FakeOps(self.round16)
        outs = []
        for j in range(n_chunks):
            single = bool((single_mask >> j) & 1)
            ids = [slot0 + j] if single else [slot0 + j, slot0 + j - 1]
            r = res[:, j].reshape(3 * n, S, D) if res is not None else None
            dt = out_dtype
            if single:
                dt = kf_out.dtype if r is None else torch.promote_types(kf_out.dtype, r.dtype)
            o = inner.propagate(tgt[j * n * S:(j + 1) * n * S], piv, inv_norm, ids, kf_out, None if single else w, n, r, dt)
            outs.append(o.to(out_dtype).view(3, n, S, D))
        return self._with_norm(torch.stack(outs, dim=1).reshape(3 * n_chunks * n, S, D), norm)

    def propagate(self, tgt, piv, inv_norm, kf_ids, kf_out, w, n, residual, out_dtype, norm=None):
        self.calls.append(("propagate", tuple(tgt.shape), tuple(int(i) for i in kf_ids)))
        return super().propagate(tgt, piv, inv_norm, kf_ids, kf_out, w, n, residual, out_dtype, norm=norm)

    def propagate_chunks(self, tgt, piv, inv_norm, kf_out, w, n, n_chunks, slot0, first_single, residual, out_dtype, norm=None):
        self.calls.append(("propagate_chunks", tuple(tgt.shape), int(n_chunks), int(slot0), bool(first_single)))
        return FakeOps(self.round16).propagate_chunks(tgt, piv, inv_norm, kf_out, w, n, n_chunks, slot0, first_single, residual,
                                                      out_dtype, norm=norm)
