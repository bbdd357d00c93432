"""Per-edit injection schedules in a multi-edit batch (TEST INFRASTRUCTURE; tests/edit_forms.py has the batch layout).

The definition every test uses: for every op, the slices of edit e are what the single-edit op computes on
[source | uncond_e | cond_e] with edit e's OWN injection state.  A mask carries that state, bit e = edit e injects.

  mask_bits / popcount          the edits of a mask
  ScheduleEditFakeOps           tests/edit_forms.EditFakeOps plus `inject_mask=` / `edit_mask=`, answered by per-edit oracle
                                calls with each edit's own flag
  run_edit_schedules_cfg1       the config-1 hook harness of tests/edit_forms.run_edits_cfg1 re-stated for schedules: every
                                edit is held to a SINGLE-EDIT pipeline installed with THAT edit's two schedules
"""
import copy

import torch

import tokenflow_utils as tfu
from oracle import tokenflow_oracle as orc
from tests import edit_forms as ef
from tests import fake_diffusers as fd
from tests.fake_ops import FakeOps
from tokenflow_amd import hooks

E_SCHED = 3
STEPS = [0, 6, 12, 17]
QK_MASKS = {0: 0b101, 6: 0b001, 12: 0, 17: 0}        # what the schedules below give at these steps
CONV_MASKS = {0: 0b111, 6: 0b111, 12: 0b101, 17: 0}
INJECTED_BLOCKS = [8, 9, 10, 11, 12, 13, 14, 15]     # positions of the 8 injected decoder blocks in the UNet's execution order


def schedules():
    """20 DDIM timesteps; per edit the q/k schedule and the feature schedule (a pair of edits that are not neighbours
    injects q/k at step 0; edit 1 never does)."""
    ts = ef.cfg1_timesteps()[0]
    return ts, [ts[:10], [], ts[:4]], [ts[:16], ts[:8], ts[:16]]


def mask_bits(mask: int, E: int):
    return [bool((mask >> e) & 1) for e in range(E)]


def popcount(mask: int) -> int:
    return bin(mask).count("1")


class ScheduleEditFakeOps(ef.EditFakeOps):
    """EditFakeOps that also answers the masked forms.  `calls` records a masked call with the mask as a last element."""

    def ext_attn_edits(self, q, k, v, heads, scale, inject, n_edits, out=None, q_frame0=0, fold_scale=None,
                       out_dtype=None, no_split=None, fused=None, multi_v=None, hints=0, inject_mask=None):
        if inject_mask is None:
            return super().ext_attn_edits(q, k, v, heads, scale, inject, n_edits, out=out, q_frame0=q_frame0,
                                          out_dtype=out_dtype)
        E = int(n_edits)
        assert not inject and 0 <= inject_mask < (1 << E)
        self.calls.append(("ext_attn_edits", tuple(q.shape), False, E, int(inject_mask)))
        res = None
        for e, inj in enumerate(mask_bits(inject_mask, E)):
            o, _ = self._quiet(FakeOps.ext_attn, self, ef.edit_slice(q, e, E), ef.edit_slice(k, e, E), ef.edit_slice(v, e, E),
                               heads, scale, inj, q_frame0=q_frame0, out_dtype=out_dtype)
            if res is None:
                res = torch.empty(q.shape, dtype=o.dtype)
            ef.edit_scatter(res, o, e, E)       # the source branch is the same whatever the edit's flag
        return res if out is None else out.copy_(res)

    def inject_copy_edits_(self, x, n_edits, edit_mask=None):
        if edit_mask is None:
            return super().inject_copy_edits_(x, n_edits)
        E = int(n_edits)
        assert 0 <= edit_mask < (1 << E)
        self.calls.append(("inject_copy_edits_", tuple(x.shape), E, int(edit_mask)))
        for e, inj in enumerate(mask_bits(edit_mask, E)):
            if inj:
                ef.edit_scatter(x, orc.conv_inject_(ef.edit_slice(x, e, E).clone()), e, E)
        return x


def check_op_calls(calls, E, check_attn, nn_indices):
    """tests/edit_forms.check_op_calls with the masks: every attention / feature-copy call against per-edit oracle calls
    with the flag the call carries for THAT edit (the shared positional flag, or the edit's bit of the keyword mask);
    propagation as there.  Returns the per-call attention tolerances."""
    attn_tol = []
    for ci, (name, a, out, kw) in enumerate(calls):
        if name == "ext_attn_edits":
            q, k, v, heads, scale, inject, n_edits = a[:7]
            assert n_edits == E and len(a) == 7
            if "inject_mask" in kw:
                assert inject is False and set(kw) == {"inject_mask"}
                flags = mask_bits(kw["inject_mask"], E)
            else:
                assert not kw
                flags = [bool(inject)] * E
            attn_tol.append(max(
                check_attn(ef.edit_slice(out, e, E), ef.edit_slice(q, e, E).float(), ef.edit_slice(k, e, E).float(),
                           ef.edit_slice(v, e, E).float(), heads, scale, flags[e],
                           f"call {ci} ext_attn_edits edit {e} inject {flags[e]}")
                for e in range(E)))
        elif name == "inject_copy_edits_":
            x_before, n_edits = a[:2]
            assert n_edits == E and len(a) == 2
            flags = mask_bits(kw["edit_mask"], E) if "edit_mask" in kw else [True] * E
            assert set(kw) <= {"edit_mask"}
            for e in range(E):
                before = ef.edit_slice(x_before, e, E)
                want = orc.conv_inject_(before.clone()) if flags[e] else before
                assert torch.equal(ef.edit_slice(out, e, E), want), f"call {ci} inject_copy_edits_ edit {e}"
        else:
            assert name == "propagate_chunks_edits", f"a multi-edit pass called the single-edit op {name}"
            ef.check_op_calls([calls[ci]], E, check_attn, nn_indices)
    return attn_tol


def install(pipe, qk_sched, conv_sched):
    tfu.register_extended_attention_pnp(pipe, torch.tensor(qk_sched))
    tfu.register_conv_injection(pipe, torch.tensor(conv_sched))
    tfu.set_tokenflow(pipe.unet)


def run_edit_schedules_cfg1(make_ops, dev, monkeypatch, check_attn, nn_indices, block_tol=None, steps=STEPS):
    """Config 1 through the public hook API, E = 3 edits with the schedules of `schedules()`, one step per entry of `steps`:
      * call counts per step are the single-edit harness's (16 attention calls, one propagation per (block, chunk), at most
        one feature copy);
      * uniform masks arrive as today's positional calls, mixed masks as the keywords `inject_mask=` / `edit_mask=`, the
        attention's only on the 8 injected blocks;
      * every op call against per-edit oracle calls with each edit's own flag (check_op_calls);
      * for every edit, every block output and the resnet output against a SINGLE-EDIT pipeline installed with THAT edit's two
        schedules: within 1e-5 of the output range over the oracle-backed ops, block_tol(attn_tol) over the HIP ops (as
        tests/edit_forms.run_edits_cfg1); NN-search inputs and indices equal."""
    torch.manual_seed(0)
    E, K, nblk = E_SCHED, ef.CFG1["K"], len(ef.LEVELS)
    ts, qk, conv = schedules()
    base = fd.FakePipeline(dims=ef.CFG1["D"][:3], heads=ef.CFG1["heads"], cross_dim=ef.CFG1["cross"]).eval()
    multi = copy.deepcopy(base).to(dev)
    install(multi, ts[:10], ts[:16])                 # the installers' shared schedules: overridden per edit below
    tfu.register_edits(multi, E)
    tfu.register_edit_schedules(multi, qk_schedules=qk, conv_schedules=conv)
    singles = []
    for e in range(E):
        pipe = copy.deepcopy(base).to(dev)
        install(pipe, qk[e], conv[e])
        singles.append(pipe)
    all_ones = (1 << E) - 1
    worst = 0.0
    for step in steps:
        t = ts[step]
        qk_mask = sum(1 << e for e in range(E) if t in qk[e])
        conv_mask = sum(1 << e for e in range(E) if t in conv[e])
        assert qk_mask == QK_MASKS.get(step, qk_mask) and conv_mask == CONV_MASKS.get(step, conv_mask)
        inp = ef.cfg1_edit_inputs(step, E)
        spy = ef.SpyOps(make_ops())
        monkeypatch.setattr(hooks, "ops", spy)
        got = ef.drive(multi, inp, t, dev)
        calls = list(spy.calls)
        attn = [c for c in calls if c[0] == "ext_attn_edits"]
        prop = [c for c in calls if c[0] == "propagate_chunks_edits"]
        copies = [c for c in calls if c[0] == "inject_copy_edits_"]
        assert len(attn) == nblk and len(prop) == nblk * K, (len(attn), len(prop))
        assert len(copies) == (1 if conv_mask else 0) and len(calls) == len(attn) + len(prop) + len(copies)
        # ---- how the masks arrive
        for i, c in enumerate(attn):
            injected = i in INJECTED_BLOCKS
            if injected and qk_mask not in (0, all_ones):
                assert c[1][5] is False and c[3] == {"inject_mask": qk_mask}, (step, i, c[3])
            else:
                assert not c[3] and c[1][5] is (injected and qk_mask == all_ones), (step, i, c[3])
        for c in copies:
            assert c[3] == ({} if conv_mask == all_ones else {"edit_mask": conv_mask}), (step, c[3])
        for o in got["pivotal"] + sum(got["chunks"], []) + [got["resnet"]]:
            assert bool(torch.isfinite(o).all())
        attn_tol = check_op_calls(calls, E, check_attn, nn_indices)
        # ---- per edit: the single-edit pipeline that was installed with this edit's schedules
        for e in range(E):
            spy1 = ef.SpyOps(make_ops())
            monkeypatch.setattr(hooks, "ops", spy1)
            ref = ef.drive(singles[e], ef.slice_inputs(inp, e, E), t, dev)
            attn1 = [c for c in spy1.calls if c[0] == "ext_attn"]
            assert sum(1 for c in attn1 if c[1][5]) == (8 if (qk_mask >> e) & 1 else 0)
            assert len([c for c in spy1.calls if c[0] == "inject_copy_"]) == ((conv_mask >> e) & 1)
            prop1 = [c for c in spy1.calls if c[0] == "propagate"]
            assert len(prop1) == len(prop) and not any(c[0].endswith("edits") or c[0].endswith("edits_") for c in spy1.calls)
            for cm, c1 in zip(prop, prop1):
                assert all(torch.equal(cm[1][j], c1[1][j]) for j in range(3))      # equal search inputs => equal indices
            for cm, c1 in list(zip(prop, prop1))[::max(1, len(prop) // 8)]:
                ids = list(c1[1][3])
                assert torch.equal(nn_indices(cm[1][0], cm[1][1], cm[1][2], ids), nn_indices(c1[1][0], c1[1][1], c1[1][2], ids))
            pairs = [("resnet", got["resnet"], ref["resnet"], None)]
            for i in range(nblk):
                pairs.append((f"block {i} pivotal", got["pivotal"][i], ref["pivotal"][i], i))
                pairs += [(f"block {i} chunk {c}", got["chunks"][c][i], ref["chunks"][c][i], i) for c in range(K)]
            for what, m, r, i in pairs:
                err = float((ef.edit_slice(m, e, E) - r).abs().max())
                rel = err / float(r.abs().max())
                worst = max(worst, rel)
                if block_tol is None or i is None:
                    assert rel <= 1e-5, f"step {step} edit {e} {what}: {rel:.3e} of the output range"
                else:
                    tol = block_tol(attn_tol[i])
                    assert err <= tol, f"step {step} edit {e} {what}: {err:.3e} > {tol:.3e}"
    print(f"per-edit schedules cfg1 (E={E}): worst block difference from the single-edit pipelines {worst:.3e} of the output range")
    return worst
