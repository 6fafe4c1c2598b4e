#!/usr/bin/env python3
"""Two-column table of per-kernel code-generation figures from two sets of `hipcc --save-temps` device listings.

    python tools/kernel_meta.py BEFORE AFTER      # each a *-hip-amdgcn-*.s listing or a directory of them

For every __global__ function found on either side: .vgpr_count, .agpr_count, .sgpr_count, .vgpr_spill_count,
.private_segment_fixed_size (scratch bytes), .group_segment_fixed_size (static LDS bytes) from the listing's amdhsa.kernels
metadata, the instruction count of the function body, and the waves per SIMD the register count allows (512 over the allocated
VGPRs + AGPRs, allocated in blocks of 8, at most 8; not capped by the launch bound, which is a minimum: where LDS leaves room a
kernel runs as many workgroups as its registers allow).  A row
whose spills or scratch grew, whose static LDS differs or whose waves fell is marked with `<<`.
"""
import glob
import os
import re
import shutil
import subprocess
import sys

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
HEAD = ("vgpr", "agpr", "sgpr", "spill", "scratch", "lds", "insts", "waves")


def listings(path):
    if os.path.isdir(path):
        return sorted(glob.glob(os.path.join(path, "*-hip-amdgcn-*.s")))
    return [path]


def waves(vgpr, agpr):
    alloc = -(-((vgpr + 3) // 4 * 4 + agpr) // 8) * 8
    return min(8, 512 // alloc) if alloc else 8


def read(path):
    """{(translation unit, kernel symbol): figures}"""
    out = {}
    for f in listings(path):
        unit = os.path.basename(f).split("-hip-")[0]
        text = open(f).read()
        meta = {}
        for block in re.split(r"\n  - \.agpr_count:", text.split("amdhsa.kernels:")[-1])[1:]:
            block = ".agpr_count:" + block
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1)) for k in FIELDS}
        for name, m in meta.items():
            body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M)
            insts = sum(1 for ln in body.group(0).splitlines() if re.match(r"\s+[a-z]\w*(\s|$)", ln)) if body else -1
            v = [m[k] for k in FIELDS]
            out[(unit, name)] = v + [insts, waves(m["vgpr_count"], m["agpr_count"])]
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return names
    r = subprocess.run([tool], input="\n".join(names), stdout=subprocess.PIPE, text=True)
    return r.stdout.splitlines() if r.returncode == 0 else names


def main():
    before, after = read(sys.argv[1]), read(sys.argv[2])
    keys = sorted(set(before) | set(after))
    short = [re.sub(r"\(.*", "", re.sub(r"^void ", "", d.replace("(anonymous namespace)::", "").replace("sgx::", "")))
             for d in demangle([k[1] for k in keys])]
    print("%-14s %-52s | %s" % ("unit", "kernel", "  ".join("%11s" % h for h in HEAD)))
    bad = 0
    for key, nm in zip(keys, short):
        b, a = before.get(key), after.get(key)
        cells = ["%5s>%-5s" % ("-" if b is None else b[i], "-" if a is None else a[i]) for i in range(len(HEAD))]
        flag = ""
        if b and a and (a[3] > b[3] or a[4] > b[4] or a[5] != b[5] or a[7] < b[7]):
            flag, bad = "  <<", bad + 1
        print("%-14s %-52s | %s%s" % (key[0], nm[:52], "  ".join(cells), flag))
    print("%d kernels, %d marked" % (len(keys), bad))


if __name__ == "__main__":
    main()
