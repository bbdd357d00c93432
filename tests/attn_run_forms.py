"""The kernel forms a run call of the attention over a bank in pieces (ops.ext_attn_runs, tf_ext_attn_run) can launch, and
the GPU cases that run each of them.

ops.attn_run_plan (tf_ext_attn_run_plan) lists the launches of ONE run call followed by the merge, recorded by the
library's own launch code.  Launches that leave partial results carry `,run` as their last template parameter; the
source branch of the query frames is a final result and carries none.

CASES maps every form the sweep reaches to the GPU cases that run it (tests/test_attn_runs_gpu.py); the CPU test
(tests/test_attn_run_plan_cpu.py) checks that every reachable form has a case and that every case plans its form.
A case is a run SET on a rank's geometry -- K = 5 bank frames, the queries of frames 2 and 3, runs (2,2), (0,2), (4,1),
the first of which computes the source branch -- unless it names another.
"""
HINT_MIX = 1 << 18   # _lib.TF_ATTN_HINT_MIX (kept literal: this module imports nothing of the package)

BASE = dict(K=5, Kq=2, q_frame0=2, runs=[(2, 2), (0, 2), (4, 1)])


def form(token: str) -> str:
    """`merge[runs=3]` -> `merge[runs]`; every other token is its own form."""
    return "merge[runs]" if token.startswith("merge[runs=") else token


# ------------------------------------------------------------------ the sweep
SWEEP_SHAPES = {
    # Dh: S values (ragged and tile multiples), heads
    40: ([45, 200, 256, 320, 576, 723, 1024, 4096], [1, 2, 8, 16]),
    64: ([45, 256, 515, 576, 700, 1024, 4096], [1, 5, 10]),
    80: ([64, 181, 256, 264, 1024, 1040], [1, 2, 8]),
    160: ([16, 45, 64, 72, 256, 320], [1, 8, 20]),
}
# (K, Kq, run_n): a rank's local run, a remote run, one frame per run, the whole bank, cfg5's and cfg2's rank geometry
SWEEP_GEOMETRY = [(5, 2, 2), (5, 2, 1), (8, 1, 1), (8, 8, 8), (4, 4, 4), (25, 4, 4), (25, 3, 21), (25, 3, 18), (8, 1, 6), (2, 1, 1)]


def sweep():
    """(key, kwargs of plan()) over the sweep grid."""
    for dh, (ss, hh) in SWEEP_SHAPES.items():
        for K, Kq, run_n in SWEEP_GEOMETRY:
            for S in ss:
                for H in hh:
                    for inject in (False, True):
                        for bank_only in (False, True):
                            if not bank_only and Kq > run_n:
                                continue   # the source branch needs the query frames inside the run
                            for fold in ((False, True) if dh == 40 else (False,)):
                                for out32 in (False, True):
                                    for hints in ((0, HINT_MIX) if dh == 40 else (0,)):
                                        for no_split in (False, True):
                                            kw = dict(K=K, Kq=Kq, run_n=run_n, n_runs=min(3, K), S=S, heads=H, dh=dh,
                                                      inject=inject, bank_only=bank_only, fold_scale=fold, out_f32=out32,
                                                      hints=hints, no_split=no_split)
                                            yield key(kw), kw


def key(kw) -> str:
    return ("run K{K} Kq{Kq} n{run_n}/{n_runs} S{S} H{heads} d{dh} inj{inject:d} bank{bank_only:d} fold{fold_scale:d} "
            "o32{out_f32:d} hints{hints} ns{no_split:d}").format(**kw)


def plan(ops, kw):
    import torch
    kw = dict(kw)
    out32 = kw.pop("out_f32", False)
    dtype = kw.pop("dtype", torch.bfloat16)
    return ops.attn_run_plan(kw.pop("K"), kw.pop("Kq"), kw.pop("run_n"), kw.pop("n_runs"), kw.pop("S"), kw.pop("heads"),
                             kw.pop("dh"), kw.pop("inject"), dtype=dtype, out_dtype=torch.float32 if out32 else None, **kw)


# ------------------------------------------------------------------ the table: form -> GPU cases (run sets) that run it
def R(S, H, dh, inject=False, hints=0, fold_scale=False, no_split=False, **geometry):
    """A run set: BASE geometry unless K / Kq / q_frame0 / runs are given."""
    g = dict(BASE)
    g.update(geometry)
    return dict(S=S, heads=H, dh=dh, inject=inject, hints=hints, fold_scale=fold_scale, no_split=no_split, **g)


def case_plans(ops, case):
    """The plan of every run call of a case's run set (run 0 with the source branch, the others bank-only)."""
    out = []
    for r, (f0, n) in enumerate(case["runs"]):
        out.append(plan(ops, dict(K=case["K"], Kq=case["Kq"], run_n=n, n_runs=len(case["runs"]), S=case["S"],
                                  heads=case["heads"], dh=case["dh"], inject=case["inject"], bank_only=r != 0,
                                  fold_scale=case["fold_scale"], hints=case["hints"], no_split=case["no_split"])))
    return out


MIX = HINT_MIX
WIDE = dict(K=8, Kq=4, q_frame0=2, runs=[(2, 4), (0, 2), (6, 2)])      # four query frames: grids of >= 256 eight-wave workgroups
WIDE16 = dict(K=10, Kq=8, q_frame0=1, runs=[(1, 8), (0, 1), (9, 1)])   # with 16 heads: the 8-wave one-tile kernels
CASES = {
    "vt_pack": [R(576, 2, 64)],
    "merge[runs]": [R(576, 2, 64)],
    # ---- Dh = 40, fp32 score scaling
    "il<40,8,ALL,4,2,run>": [R(1024, 8, 40, **WIDE)],
    "il<40,8,ALL,4,3,run>": [R(256, 2, 40, hints=MIX)],
    "il<40,8,DUAL,4,2,run>": [R(1024, 8, 40, inject=True, **WIDE)],
    "il<40,8,SOURCE,4,2>": [R(1024, 8, 40, inject=True, **WIDE)],
    "il<40,8,SOURCE,4,3>": [R(1024, 8, 40, inject=True, hints=MIX)],
    "one<40,1,4,ALL,2,fq0,run>": [R(723, 1, 40), R(200, 2, 40, inject=True)],
    "one<40,1,8,ALL,2,fq0,run>": [R(328, 16, 40, **WIDE16)],
    "one<40,1,4,DUAL,3,fq0,run>": [R(328, 2, 40, inject=True)],
    "one<40,1,4,SOURCE,2,fq0>": [R(723, 1, 40, inject=True)],
    "one<40,1,8,SOURCE,2,fq0>": [R(328, 16, 40, inject=True, **WIDE16)],
    "il<40,4,DUAL,3,0,run>": [R(256, 2, 40, inject=True)],
    # Dh = 40, folded scale (opt-in)
    "one<40,1,4,ALL,2,fq1,run>": [R(200, 2, 40, fold_scale=True)],
    "one<40,1,8,ALL,2,fq1,run>": [R(320, 16, 40, fold_scale=True, **WIDE16)],
    "one<40,1,4,DUAL,3,fq1,run>": [R(576, 2, 40, inject=True, fold_scale=True)],
    "one<40,1,4,SOURCE,2,fq1>": [R(576, 2, 40, inject=True, fold_scale=True)],
    "one<40,1,8,SOURCE,2,fq1>": [R(320, 16, 40, inject=True, fold_scale=True, **WIDE16)],
    # ---- Dh = 64
    "il<64,8,ALL,4,2,run>": [R(576, 2, 64)],
    "il<64,4,DUAL,2,2,run>": [R(576, 2, 64, inject=True)],
    "il<64,8,SOURCE,4,2>": [R(576, 2, 64, inject=True)],
    "pp<64,ALL,run>": [R(515, 1, 64, no_split=True), R(700, 2, 64)],
    "one<64,1,4,ALL,2,fq1,run>": [R(200, 2, 64)],
    "one<64,1,4,DUAL,2,fq1,run>": [R(515, 1, 64, inject=True)],
    "one<64,1,4,SOURCE,2,fq1>": [R(515, 1, 64, inject=True), R(515, 1, 64, no_split=True)],
    # ---- Dh = 80
    "il<80,4,ALL,3,2,run>": [R(256, 2, 80)],
    "il<80,4,DUAL,2,2,run>": [R(256, 2, 80, inject=True)],
    "il<80,4,SOURCE,3,2>": [R(256, 2, 80, inject=True)],
    "one<80,1,4,ALL,2,fq1,run>": [R(181, 2, 80)],
    "one<80,1,4,DUAL,2,fq1,run>": [R(264, 1, 80, inject=True)],
    "one<80,1,4,SOURCE,2,fq1>": [R(264, 1, 80, inject=True)],
    # ---- Dh = 160
    "one<160,1,4,ALL,1,fq1,sb,run>": [R(72, 1, 160), R(72, 1, 160, inject=True)],
}
