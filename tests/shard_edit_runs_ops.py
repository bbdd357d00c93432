"""Oracle-backed stand-in for the run form of the multi-edit attention (TEST INFRASTRUCTURE, imported by
tests/test_shard_edit_runs_cpu.py): `ShardEditFakeOps` plus `ext_attn_runs_edits_views`, answered per edit by the single-edit
run form of tests/test_bank_runs_cpu.py (`RunsFakeOps.ext_attn_runs_views`: per-run scores in torch, log-sum-exp merge in
slot order) on exactly the views that edit may read -- a run that looked outside its frames, at a slab that was never sent
or at another edit's slot would poison its result with NaN."""
import torch

from tests.shard_edit_ops import ShardEditFakeOps
from tests.test_bank_runs_cpu import RunsFakeOps


class ShardEditRunsFakeOps(ShardEditFakeOps):
    ext_attn_runs_views = RunsFakeOps.ext_attn_runs_views      # one edit: the single-edit run form itself

    def ext_attn_runs_edits_views(self, q, kv_runs, out, heads, scale, n_edits, inject_mask, runs, K, branch0=(0, 0),
                                  q_frame0=0, q_compact=False, streams=None, fold_scale=None, no_split=False, hints=0,
                                  order=None):
        E, mask = int(n_edits), int(inject_mask)
        assert 0 <= mask < (1 << E) and len(kv_runs) == len(runs)
        self.calls.append(("ext_attn_runs_edits", tuple(runs), E, mask, tuple(bool(kv[4]) for kv in kv_runs), bool(q_compact)))
        assert not kv_runs[0][4], "the local run reads the caller's dense k"

        def br(t, b0, lo, n):      # branches [lo, lo + n) of the tensor whose view `t` starts at branch b0
            a = lo - b0
            assert 0 <= a and a + n <= t.shape[0], f"the view does not hold branches [{lo}, {lo + n})"
            return t[a:a + n]
        Kq = q.shape[1]
        src = None
        n_non = 0
        for e in range(E):
            inj = bool((mask >> e) & 1)
            lo = 1 + 2 * e
            c_lo = 1 + 2 * n_non      # the edit's slot in a compact tensor
            n_non += 0 if inj else 1
            qe = br(q, branch0[0], 0, 1) if inj else br(q, branch0[0], c_lo if q_compact else lo, 2)
            if not inj:               # run 0 also reads the source's q: [source | uncond_e | cond_e]
                qe = torch.cat([br(q, branch0[0], 0, 1), qe])
            kv_e = []
            for r, (kv, vv, kb0, vb0, k_compact) in enumerate(kv_runs):
                ke = br(kv, kb0, 0, 1) if inj else br(kv, kb0, c_lo if k_compact else lo, 2)
                ve = br(vv, vb0, lo, 2)
                if r == 0:            # the local run holds the source branch's k and v too
                    ke = ke if inj else torch.cat([br(kv, kb0, 0, 1), ke])
                    kv_e.append((ke, torch.cat([br(vv, vb0, 0, 1), ve]), 0, 0))
                else:
                    kv_e.append((ke, ve, 0 if inj else 1, 1))
            tmp = torch.full((3, Kq) + tuple(q.shape[2:]), float("nan"), dtype=out.dtype)
            calls, self.calls = self.calls, []
            try:
                RunsFakeOps.ext_attn_runs_views(self, qe, kv_e, tmp, heads, scale, inj, runs, K, branch0=(0, 0),
                                                q_frame0=q_frame0, order=order)
            finally:
                self.calls = calls
            out[lo - branch0[1]] = tmp[1]
            out[lo + 1 - branch0[1]] = tmp[2]
            assert src is None or torch.equal(src, tmp[0]), "the source branch does not depend on the edit"
            src = tmp[0]
        out[0 - branch0[1]] = src
        return out
