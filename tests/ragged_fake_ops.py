"""Oracle-backed stand-in for `ops.propagate_chunks_ragged` (TEST INFRASTRUCTURE, beside tests/segment_fake_ops.py): a ragged
run is, by definition, the one-chunk op on every chunk's tensors alone with ITS frame count -- that is what this computes,
from the plain FakeOps, while recording the calls the hooks make."""
import torch

from oracle import tokenflow_oracle as orc
from tests.edit_forms import EditFakeOps, edit_scatter, edit_slice
from tests.fake_ops import FakeOps
from tests.segment_fake_ops import SegmentFakeOps


class RaggedFakeOps(SegmentFakeOps, EditFakeOps):
    def propagate_chunks_ragged(self, tgt, piv, inv_norm, kf_out, w, chunk_frames, slot0, single_mask, residual, out_dtype,
                                n_edits=1, norm=None):
        """Chunk j of the run = one `FakeOps.propagate` with n = chunk_frames[j] (per edit: on [source | uncond_e | cond_e])."""
        frames = tuple(int(n) for n in chunk_frames)
        E, C, F = int(n_edits), len(frames), sum(frames)
        self.calls.append(("propagate_chunks_ragged", tuple(tgt.shape), frames, int(slot0), int(single_mask), E))
        assert C > 1 and len(set(frames)) > 1 and not single_mask >> C and (E == 1 or single_mask <= 1)
        # one weight per frame of the run: every chunk's own blend weights, concatenated
        assert w.dtype == torch.float32 and torch.equal(w.cpu(), torch.cat([orc.blend_weights(n, 1) for n in frames]))
        S, D = piv.shape[1:]
        nb = 1 + 2 * E
        assert tgt.shape == (F * S, D) and kf_out.shape[0] == nb * piv.shape[0]
        res = torch.empty(nb * F, S, D, dtype=out_dtype)
        inner = FakeOps(self.round16)
        for e in range(E):
            kf_e = edit_slice(kf_out, e, E) if E > 1 else kf_out
            r_e = None if residual is None else (edit_slice(residual, e, E) if E > 1 else residual).view(3, F, S, D)
            outs, f0 = [], 0
            for j, n in enumerate(frames):
                single = bool((single_mask >> j) & 1)
                ids = [slot0 + j] if single else [slot0 + j, slot0 + j - 1]
                r = r_e[:, f0:f0 + n].reshape(3 * n, S, D) if r_e is not None else None
                dt = out_dtype
                if single:
                    dt = kf_out.dtype if r is None else torch.promote_types(kf_out.dtype, r.dtype)
                o = inner.propagate(tgt[f0 * S:(f0 + n) * S], piv, inv_norm, ids, kf_e, None if single else w[f0:f0 + n], n, r, dt)
                outs.append(o.to(out_dtype).view(3, n, S, D))
                f0 += n
            o3 = torch.cat(outs, dim=1).reshape(3 * F, S, D)
            if E > 1:
                edit_scatter(res, o3, e, E)
            else:
                res = o3
        return self._with_norm(res, norm)
