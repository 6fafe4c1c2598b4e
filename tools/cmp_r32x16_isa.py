"""Compares the gfx950 assembly of every k_r32x16<...> instance between two `--save-temps` builds of kernels_r32x16.hip (no GPU needed):
instances present in both must be identical once comments and local label / block numbers are stripped.  Exit status 1 if any differ.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Iinclude -Ispectrograms_amd/csrc --save-temps -c spectrograms_amd/csrc/kernels_r32x16.hip
    (once at each commit, in separate directories), then
    python tools/cmp_r32x16_isa.py OLD/kernels_r32x16-hip-amdgcn-amd-amdhsa-gfx950.s NEW/kernels_r32x16-hip-amdgcn-amd-amdhsa-gfx950.s
"""
import re
import sys


def funcs(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'^(_ZN3sgx12_GLOBAL__N_18k_r32x16I[^:\s]*):[^\n]*\n(.*?)^\.Lfunc_end', s, re.M | re.S):
        body = re.sub(r';.*', '', m.group(2))  # comments
        body = re.sub(r'\.L\w+|BB\d+_\d+', 'L', body)  # local label numbering
        out[m.group(1)] = '\n'.join(l.rstrip() for l in body.splitlines() if l.strip())
    return out


def main():
    a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
    diff = [k for k in a if k in b and a[k] != b[k]]
    missing = [k for k in a if k not in b]
    print(f"old instances {len(a)}: identical {len(a) - len(diff) - len(missing)}, differing {len(diff)}, missing {len(missing)}; "
          f"new instances {len([k for k in b if k not in a])}")
    for k in diff + missing:
        print("DIFF" if k in diff else "MISSING", k)
    sys.exit(1 if diff or missing else 0)


if __name__ == "__main__":
    main()
