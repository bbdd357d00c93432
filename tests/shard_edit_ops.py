"""Oracle-backed stand-in for the ops a frame shard issues for a multi-edit batch (TEST INFRASTRUCTURE, imported by
tests/test_shard_edits_cpu.py): `ScheduleEditFakeOps` plus `ext_attn_edits_views`, the part form of the multi-edit attention
on strided 4-D views, answered by per-edit calls of the single-edit `FakeOps.ext_attn_views` -- which poisons every slab the
call may not read and asserts that every slab it must read was passed.  `calls` also records the pack / unpack launches with
their slab counts."""
import torch

from tests.edit_schedule_forms import ScheduleEditFakeOps
from tests.fake_ops import FakeOps


class ShardEditFakeOps(ScheduleEditFakeOps):
    def head_pack(self, slabs, W, out=None):
        self.calls.append(("head_pack", len(slabs), int(W)))
        return super().head_pack(slabs, W, out=out)

    def head_unpack(self, recv, dsts):
        self.calls.append(("head_unpack", len(dsts)))
        return super().head_unpack(recv, dsts)

    def ext_attn_edits_views(self, q, k, v, out, heads, scale, n_edits, inject_mask, part="all", qk_compact=False,
                             branch0=(0, 0, 0, 0), q_frame0=0, fold_scale=None, no_split=None, fused=None, multi_v=None,
                             hints=0, stream=None):
        E, mask = int(n_edits), int(inject_mask)
        assert 0 <= mask < (1 << E) and part in ("all", "bank", "source")
        self.calls.append(("ext_attn_edits_views", tuple(q.shape), E, mask, part, bool(qk_compact)))

        def br(t, i, lo, n=2):      # branches [lo, lo + n) of the tensor whose view `t` starts at branch branch0[i]
            a = lo - branch0[i]
            assert 0 <= a and a + n <= t.shape[0], f"the view does not hold branches [{lo}, {lo + n})"
            return t[a:a + n]
        def views(qv, kv, vv, ov, inject, prt, b0):
            # FakeOps answers a part call for every bank frame's queries only: embed a rank's query frames at their bank
            # positions (rows are independent per query, so the rank's rows are the same bits) and slice the result
            K, Kq = kv.shape[1], qv.shape[1]
            if prt == "source" or Kq == K:
                return self._quiet(FakeOps.ext_attn_views, self, qv, kv, vv, ov, heads, scale, inject, prt, branch0=b0,
                                   q_frame0=q_frame0)
            qf = torch.zeros(qv.shape[0], K, *qv.shape[2:], dtype=qv.dtype)
            qf[:, q_frame0:q_frame0 + Kq] = qv
            tmp = torch.empty(ov.shape[0], K, *ov.shape[2:], dtype=ov.dtype)
            self._quiet(FakeOps.ext_attn_views, self, qf, kv, vv, tmp, heads, scale, inject, prt, branch0=b0)
            ov.copy_(tmp[:, q_frame0:q_frame0 + Kq])
        if part != "source":
            n_non = 0
            for e in range(E):
                lo = 1 + 2 * e
                if (mask >> e) & 1:
                    views(br(q, 0, 0, 1), br(k, 1, 0, 1), br(v, 2, lo), br(out, 3, lo), True, "bank", (0, 0, 1, 1))
                else:
                    slot = 1 + 2 * n_non if qk_compact else lo
                    n_non += 1
                    views(br(q, 0, slot), br(k, 1, slot), br(v, 2, lo), br(out, 3, lo), False, "bank", (1, 1, 1, 1))
        if part != "bank":
            views(br(q, 0, 0, 1), br(k, 1, 0, 1), br(v, 2, 0, 1), br(out, 3, 0, 1), mask == (1 << E) - 1, "source",
                  (0, 0, 0, 0))
        return out
