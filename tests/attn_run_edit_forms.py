"""The GPU cases of the run form of the multi-edit attention (ops.ext_attn_runs_edits, tf_ext_attn_run_edits) and their
launch plans: run sets on the BASE geometry of tests/attn_run_forms.py (K = 5 bank frames, the queries of frames 2 and 3,
runs (2,2), (0,2), (4,1)).
"""
from tests.attn_run_forms import BASE

# (S, H, Dh): the one-tile kernels / interleaved and DUAL / the same plus the norm table / ragged, ping-pong / Dh 80 / Dh 160
SHAPES = [(200, 2, 40), (256, 2, 40), (576, 2, 64), (515, 1, 64), (256, 2, 80), (72, 1, 160)]
# (n_edits, inject_mask)
CONFIGS = [(2, 0b00), (2, 0b11), (2, 0b01), (3, 0b101)]

CASES = [dict(S=S, heads=H, dh=dh, n_edits=E, mask=m, **BASE) for S, H, dh in SHAPES for E, m in CONFIGS]


def case_id(c):
    return "S{S}-H{heads}-d{dh}-E{n_edits}-m{mask:b}".format(**c)


def case_plans(ops, c):
    """The plan of every run call of a case's run set (run 0 with the source branch, the others bank-only)."""
    return [ops.attn_run_edits_plan(c["K"], c["Kq"], n, len(c["runs"]), c["S"], c["heads"], c["dh"], c["n_edits"], c["mask"],
                                    bank_only=r != 0) for r, (f0, n) in enumerate(c["runs"])]
