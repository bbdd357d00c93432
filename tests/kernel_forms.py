"""The kernel forms the attention and NN-search dispatchers can pick, and the GPU cases that run each of them.

A launch plan (ops.attn_plan / ops.nn_plan, i.e. tf_ext_attn_plan / tf_nn_search_plan) is the list of launches a call
makes, one token per launch, recorded by the library's own launch code.  `form()` reduces a token to what a test must
cover: the kernel and its template parameters, whether the pivot range / bank is split, and (NN) whether the launch
spans several chunks.

CASES maps every form of the default build to the GPU cases that run it (tests/test_kernel_forms_gpu.py); the CPU
test (tests/test_kernel_plan_cpu.py) sweeps the planners over SWEEP_* and checks that every reachable form has a case
and that every case's plan contains its form.
"""
import re

HINT_MIX = 1 << 18   # _lib.TF_ATTN_HINT_MIX (kept literal: this module imports nothing of the package)


def form(token: str) -> str:
    """`rbs<TJ=2>[splits=4,chunks]` -> `rbs<TJ=2>[split,chunks]`, `glds[splits=1]` -> `glds`, `merge[nseg=4]` -> `merge`."""
    if token.startswith("merge["):
        return "merge"
    m = re.fullmatch(r"(.*)\[splits=(\d+)(,chunks)?\]", token)
    if not m:
        return token
    tags = (["split"] if int(m.group(2)) > 1 else []) + (["chunks"] if m.group(3) else [])
    return m.group(1) + ("[" + ",".join(tags) + "]" if tags else "")


# ------------------------------------------------------------------ sweeps (the default build's reachable plans)
SWEEP_ATTN_SHAPES = {
    # Dh: (K, Kq) pairs, S values (ragged and tile multiples), heads
    40: ([(1, 1), (2, 2), (4, 4), (4, 1), (8, 8), (8, 1), (16, 16)], [45, 200, 256, 320, 576, 723, 1024, 2048, 4096],
         [1, 2, 8]),
    64: ([(1, 1), (2, 2), (4, 4), (4, 1), (8, 8), (10, 10), (25, 25)], [45, 256, 515, 576, 1024, 2304, 4096], [1, 5, 10]),
    80: ([(1, 1), (2, 2), (4, 4), (4, 1), (8, 8), (16, 16)], [64, 181, 256, 264, 1024, 1040], [1, 2, 8]),
    160: ([(1, 1), (2, 2), (4, 4), (8, 8), (16, 16)], [16, 45, 64, 72, 256, 320], [1, 8, 20]),
}
PARTS = ("all", "bank", "source")
FUSED = (None, False, True)


def sweep_attn(hinted: bool = False):
    """(key, kwargs of ops.attn_plan) over the sweep grid.  hinted=False: no TF_ATTN_HINT_MIX (the calls whose plans
    the library must keep unchanged); True: the same grid with the hint."""
    for dh, (kk, ss, hh) in SWEEP_ATTN_SHAPES.items():
        for K, Kq in kk:
            for S in ss:
                for H in hh:
                    for inject in (False, True):
                        for part in PARTS:
                            for no_split in (False, True):
                                for fused in FUSED:
                                    for fold in ((False, True) if dh == 40 else (False,)):
                                        for out32 in (False, True):
                                            kw = dict(K=K, Kq=Kq, S=S, heads=H, dh=dh, inject=inject, part=part,
                                                      no_split=no_split, fused=fused, fold_scale=fold,
                                                      out_f32=out32, hints=HINT_MIX if hinted else 0)
                                            yield attn_key(kw), kw


def attn_key(kw) -> str:
    return ("attn K{K} Kq{Kq} S{S} H{heads} d{dh} inj{inject:d} {part} ns{no_split:d} fused{fused} fold{fold_scale:d} "
            "o32{out_f32:d} hints{hints}").format(**kw)


SWEEP_NN = dict(D=[72, 128, 320, 640, 1096, 1280], S=[64, 100, 256, 320, 576, 1024, 1040, 1568, 2304, 4096],
                n=[1, 2, 5, 8, 16, 80], P=[1, 2], C=[1, 8])


def sweep_nn():
    for D in SWEEP_NN["D"]:
        for S in SWEEP_NN["S"]:
            for n in SWEEP_NN["n"]:
                for P in SWEEP_NN["P"]:
                    for C in SWEEP_NN["C"]:
                        if C > 1 and P != 2:
                            continue
                        kw = dict(n_tgt=n * S, S=S, D=D, P=P, C=C)
                        yield nn_key(kw), kw


def nn_key(kw) -> str:
    return "nn n_tgt{n_tgt} S{S} D{D} P{P} C{C}".format(**kw)


def bench_calls():
    """The launches bench.py's cfg2 step makes: per level the attention call (plain and q/k-injected), the per-chunk
    search (one chunk against two keyframes) and the multi-chunk propagation launch (all 8 chunks, first_single)."""
    K, n = 8, 5
    for S, D, H in ((4096, 320, 8), (1024, 640, 8), (256, 1280, 8), (64, 1280, 8)):
        for inject in (False, True):
            kw = dict(K=K, Kq=K, S=S, heads=H, dh=D // H, inject=inject, part="all", no_split=False, fused=None,
                      fold_scale=False, out_f32=False, hints=0)
            yield attn_key(kw), kw
        for P, C in ((2, 1), (2, K)):
            kw = dict(n_tgt=n * S, S=S, D=D, P=P, C=C)
            yield nn_key(kw), kw


def plan(ops, kw):
    """Plan of a sweep / table entry (attn or nn, told apart by its keys)."""
    if "n_tgt" in kw:
        return ops.nn_plan(kw["n_tgt"], kw["S"], kw["D"], kw["P"], kw["C"])
    kw = dict(kw)
    import torch
    out32 = kw.pop("out_f32", False)
    dtype = kw.pop("dtype", torch.bfloat16)
    return ops.attn_plan(kw.pop("K"), kw.pop("Kq"), kw.pop("S"), kw.pop("heads"), kw.pop("dh"), kw.pop("inject"),
                         dtype=dtype, out_dtype=torch.float32 if out32 else None, **kw)


# ------------------------------------------------------------------ the table: form -> GPU cases that run it
def A(K, S, H, dh, inject=False, part="all", no_split=False, fused=False, Kq=None, hints=0, fold_scale=False):
    """An attention case (ops.ext_attn arguments; fused=False: the streaming kernels unless the form is the fused one)."""
    return dict(K=K, Kq=K if Kq is None else Kq, S=S, heads=H, dh=dh, inject=inject, part=part, no_split=no_split,
                fused=fused, fold_scale=fold_scale, out_f32=False, hints=hints)


def N(n, S, D, P=2, C=1):
    """An NN case: n frames of S targets per chunk, C chunks (C > 1: propagate_chunks with first_single)."""
    return dict(n_tgt=n * S, S=S, D=D, P=P, C=C)


MIX = HINT_MIX
CASES = {
    # ---- attention: pre-pass and merge
    "vt_pack": [A(2, 576, 2, 64)],
    "merge": [A(8, 256, 1, 40, inject=True)],
    # ---- Dh = 40, fp32 score scaling
    "il<40,8,ALL,4,2>": [A(4, 1024, 8, 40, no_split=True)],
    "il<40,8,ALL,4,3>": [A(2, 256, 2, 40, hints=MIX), A(4, 1024, 8, 40, hints=MIX, no_split=True)],
    "il<40,8,DUAL,4,2>": [A(4, 1024, 8, 40, inject=True, no_split=True)],
    "il<40,8,SOURCE,4,2>": [A(4, 1024, 8, 40, inject=True, no_split=True, part="source")],
    "il<40,8,SOURCE,4,3>": [A(4, 1024, 8, 40, inject=True, hints=MIX)],
    "one<40,1,4,ALL,2,fq0>": [A(2, 723, 1, 40)],
    "one<40,1,8,ALL,2,fq0>": [A(4, 328, 8, 40)],
    "one<40,1,4,DUAL,3,fq0>": [A(2, 328, 2, 40, inject=True)],
    "one<40,1,4,SOURCE,2,fq0>": [A(2, 723, 1, 40, inject=True)],
    "one<40,1,8,SOURCE,2,fq0>": [A(4, 328, 8, 40, inject=True)],
    "il<40,4,DUAL,3,0>": [A(2, 256, 2, 40, inject=True)],
    # Dh = 40, folded scale (opt-in)
    "one<40,1,4,ALL,2,fq1>": [A(2, 200, 2, 40, fold_scale=True)],
    "one<40,1,8,ALL,2,fq1>": [A(4, 320, 8, 40, fold_scale=True)],
    "one<40,1,4,DUAL,3,fq1>": [A(2, 576, 2, 40, inject=True, fold_scale=True)],
    "one<40,1,4,SOURCE,2,fq1>": [A(2, 576, 2, 40, inject=True, fold_scale=True, part="source")],
    "one<40,1,8,SOURCE,2,fq1>": [A(4, 320, 8, 40, inject=True, fold_scale=True)],
    # ---- Dh = 64
    "il<64,8,ALL,4,2>": [A(2, 576, 2, 64)],
    "il<64,4,DUAL,2,2>": [A(2, 576, 2, 64, inject=True)],
    "il<64,8,SOURCE,4,2>": [A(2, 576, 2, 64, inject=True, part="source")],
    "pp<64,ALL>": [A(2, 515, 1, 64, no_split=True)],
    "one<64,1,4,ALL,2,fq1>": [A(2, 200, 2, 64)],
    "one<64,1,4,DUAL,2,fq1>": [A(2, 515, 1, 64, inject=True)],
    "one<64,1,4,SOURCE,2,fq1>": [A(2, 515, 1, 64, inject=True, part="source")],
    # ---- Dh = 80
    "il<80,4,ALL,3,2>": [A(2, 256, 2, 80)],
    "il<80,4,DUAL,2,2>": [A(2, 256, 2, 80, inject=True)],
    "il<80,4,SOURCE,3,2>": [A(2, 256, 2, 80, inject=True, part="source")],
    "one<80,1,4,ALL,2,fq1>": [A(3, 181, 2, 80)],
    "one<80,1,4,DUAL,2,fq1>": [A(2, 264, 1, 80, inject=True)],
    "one<80,1,4,SOURCE,2,fq1>": [A(3, 181, 2, 80, part="source")],
    # ---- Dh = 160
    "one<160,1,4,ALL,1,fq1,sb>": [A(2, 72, 1, 160)],
    "one<160,1,4,SOURCE,1,fq1,sb>": [A(2, 72, 1, 160, inject=True, part="source")],
    # ---- the fused small-problem kernel
    "fused[qw=1,kw=4,qb=1,prec=1]": [A(2, 200, 2, 40, fused=None)],
    "fused[qw=1,kw=4,qb=1,prec=0]": [A(2, 576, 2, 64, fused=None, no_split=False)],
    "fused[qw=4,kw=1,qb=1,prec=1]": [A(8, 256, 8, 40, fused=None)],
    "fused[qw=2,kw=4,qb=1,prec=1]": [A(8, 200, 8, 40, fused=None, no_split=True)],
    "fused[qw=2,kw=4,qb=1,prec=0]": [A(4, 328, 8, 40, fused=True, no_split=True)],
    # ---- NN search (every target against the oracle; the rbs<TJ=4> launches on sampled targets)
    "rb": [N(80, 1040, 320)],
    "rb[split]": [N(1, 100, 320, P=1)],
    "rb[chunks]": [N(1, 100, 320, C=8)],
    "rb[split,chunks]": [N(1, 1040, 320, C=8)],
    "rbs<TJ=2>[split]": [N(1, 64, 320, P=1)],
    "rbs<TJ=2>[chunks]": [N(1, 64, 320, C=8)],
    "rbs<TJ=2>[split,chunks]": [N(1, 256, 320, C=8)],
    "rbs<TJ=4>": [N(80, 2304, 320)],
    "rbs<TJ=4>[split]": [N(42, 1568, 320)],
    "rbs<TJ=4>[chunks]": [N(16, 4096, 320, C=8)],
    "rbs<TJ=4>[split,chunks]": [N(16, 2304, 320, C=8)],
    "glds": [N(80, 256, 320)],
    "glds[split]": [N(16, 1024, 640)],
    "glds[chunks]": [N(80, 64, 320, C=8)],
    "glds[split,chunks]": [N(5, 320, 320, C=8)],
    "wide": [N(80, 100, 72)],
    "wide[split]": [N(16, 256, 72)],
    "wide[chunks]": [N(8, 64, 72, C=8)],
    "wide[split,chunks]": [N(2, 256, 72, C=8)],
    "bk64": [N(1, 64, 72, P=1)],
    "bk64[chunks]": [N(1, 64, 72, C=8)],
    "bk64[split]": [N(1, 256, 72, P=1)],
    "bk64[split,chunks]": [N(1, 256, 72, C=8)],
    "bk128": [N(1, 64, 640, P=1)],
    "bk128[chunks]": [N(1, 64, 640, C=8)],
    "bk128[split]": [N(1, 256, 640, P=1)],
    "bk128[split,chunks]": [N(1, 256, 640, C=8)],
    "deep": [N(1, 64, 1096, P=1)],
    "deep[chunks]": [N(1, 64, 1096, C=8)],
    "deep[split]": [N(1, 100, 1096, P=1), N(2, 256, 1280)],
    "deep[split,chunks]": [N(1, 256, 1096, C=8)],
    "finalize": [N(1, 64, 320, P=1)],
}
