#!/usr/bin/env python3
"""Compare the per-kernel resource usage of two builds of one HIP source (no GPU needed).

  hipcc <the Makefile's flags> -Rpass-analysis=kernel-resource-usage -c X.hip -o /dev/null 2> before.txt   (parent tree)
  hipcc ...                                                                         2> after.txt    (this tree)
  tools/kernel_resource_table.py before.txt after.txt [--drop-arg NAME ...]

Kernels are matched by their demangled name.  A template parameter added with a default (the chunk-descriptor type of the
ragged forms) changes the mangled name of every existing instantiation: --drop-arg removes that trailing template argument
before matching, so `kernel<.., NnChunks>` of the new build meets `kernel<..>` of the old one, and instantiations on another
descriptor are listed as NEW beside the sibling that differs from them in that argument only.
"""
import argparse
import re
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "TotalSGPRs"]
SHORT = ["vgpr", "agpr", "scratch", "occ", "lds", "sgpr"]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = m.group(2)
    return out


def demangle(names):
    names = list(names)
    if not names:
        return {}
    # binutils' c++filt does not know the _Float16 / __bf16 manglings (DF16_, DF16b): two other builtin codes stand in for
    # them (builtin types are never substitution candidates, so the back references keep their numbers)
    fed = [n.replace("DF16_", "Dh").replace("DF16b", "Dd") for n in names]
    for tool in ("llvm-cxxfilt", "c++filt"):
        try:
            res = subprocess.run([tool], input="\n".join(fed), capture_output=True, text=True, check=True)
        except (OSError, subprocess.CalledProcessError):
            continue
        lines = [re.sub(r"\bhalf\b", "_Float16", x).replace("decimal64", "__bf16") for x in res.stdout.splitlines()]
        return dict(zip(names, lines))
    return {n: n for n in names}


def short(name):
    """`void (anonymous namespace)::kernel<args>(params)` -> `kernel<args>`"""
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, c in enumerate(name):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            return name[:i]
    return name


def row(vals):
    return " ".join(f"{vals.get(f, '?'):>7}" for f in FIELDS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--drop-arg", action="append", default=[], help="trailing template argument that is the new default")
    ap.add_argument("--new-arg", action="append", default=[], help="trailing template argument of the new instantiations")
    a = ap.parse_args()
    before, after = parse(a.before), parse(a.after)
    dm_b, dm_a = demangle(before), demangle(after)
    old = {short(dm_b[k]): v for k, v in before.items()}
    new = {}
    for k, v in after.items():
        s = short(dm_a[k])
        for d in a.drop_arg:
            s = s.replace(f", {d}>", ">")
        new[s] = v
    head = f"{'':8}" + " ".join(f"{s:>7}" for s in SHORT)
    changed = 0
    print(f"# existing instantiations: {len(old)} before, matched by name in the new build")
    for name in sorted(old):
        if name not in new:
            print(f"MISSING  {name}")
            changed += 1
            continue
        same = all(old[name].get(f) == new[name].get(f) for f in FIELDS[:5])
        if not same:
            changed += 1
            print(f"CHANGED  {name}\n{head}\n  before {row(old[name])}\n  after  {row(new[name])}")
    print(f"# {len(old) - changed} of {len(old)} existing instantiations: equal VGPRs, AGPRs, scratch, occupancy and LDS"
          f" ({changed} differ)")
    fresh = sorted(n for n in new if n not in old)
    print(f"# new instantiations: {len(fresh)}")
    worse = 0
    for name in fresh:
        sib = None
        for d in a.new_arg:
            if name.endswith(f", {d}>"):
                sib = name[:-len(f", {d}>")] + ">"
        sv = new.get(sib) or old.get(sib)
        print(f"NEW      {name}\n{head}\n  new    {row(new[name])}")
        if sv:
            print(f"  uniform{row(sv)}")
            if int(new[name][FIELDS[3]]) < int(sv[FIELDS[3]]):
                worse += 1
                print("  ^ occupancy BELOW the uniform sibling")
        if new[name][FIELDS[2]] != "0":
            worse += 1
            print("  ^ SCRATCH in use")
    print(f"# new instantiations with scratch or an occupancy below their sibling's: {worse}")
    return 1 if changed or worse else 0


if __name__ == "__main__":
    sys.exit(main())
