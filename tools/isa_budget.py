#!/usr/bin/env python3
"""Per-tile instruction budget of one k_r32x16 instance's main loop, from a `hipcc --save-temps` listing (no GPU needed):

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Iinclude -Ispectrograms_amd/csrc --save-temps -c spectrograms_amd/csrc/kernels_r32x16.hip
    python tools/isa_budget.py kernels_r32x16-hip-amdgcn-amd-amdhsa-gfx950.s k_r32x16ILi0ELi0ELi5ELb1ELb1ELb0ELi0ELb0ELi0E

The main loop (the outermost loop with the most instructions) is cut into phases at its s_barrier instructions; a block that
only some waves enter (`s_cbranch_execz` over it: job 0's rearrangement) is reported on its own.  Per phase: VALU split into
packed (v_pk_*), v_cndmask, v_mov, address math (integer adds / shifts / mads / ands / ors) and other plain VALU; LDS
instructions and bytes per lane; SALU; VMEM.  Cost model (per lane and tile, at two lockstep waves per SIMD): 5 cycles per
packed instruction, 2.7 per plain VALU, LDS bytes / 128 B per clock x 64 lanes."""
import re
import sys

LDS_BYTES = {"b32": 4, "b64": 8, "b96": 12, "b128": 16, "u8": 1, "u16": 2, "i8": 1, "i16": 2, "2_b32": 8, "2_b64": 16,
             "2st64_b32": 8, "2st64_b64": 16, "addtid_b32": 4}


def classify(op):
    if op.startswith("v_pk_"):
        return "pk"
    if op.startswith("v_cndmask"):
        return "cnd"
    if op.startswith("v_mov") or op.startswith("v_accvgpr"):
        return "mov"
    if op.startswith("v_"):
        if re.match(r"^v_(add|sub|subrev)_(co_)?(ci_)?u32|^v_(add|sub|subrev)_(nc_)?[ui]32|^v_lsh|^v_ash|^v_and|^v_or|^v_xor|^v_mad_u|^v_mul_(lo|hi)_u|^v_mul_u32|^v_add3|^v_bfe|^v_bfi|^v_mbcnt|^v_readfirstlane|^v_(min|max)_u32|^v_cmp|^v_mad_i32|^v_mul_lo_i|^v_perm", op):
            return "addr"
        return "plain"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("buffer_") or op.startswith("global_"):
        return "vmem"
    return None


def lds_bytes(op):
    m = re.match(r"ds_(read|write|load|store)(\w+)", op)
    if not m:
        return 0
    return LDS_BYTES.get(m.group(2).lstrip("_"), 0)


def main():
    lst, key = sys.argv[1], sys.argv[2]
    lines = open(lst).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(key) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    # basic blocks: (label line, instruction lines); the main loop = its header block and every block tagged "in Loop: Header=<it> Depth=1"
    blocks, cur = [], None
    for i, l in enumerate(body):
        if re.match(r"^(\.LBB\w+:|; %bb\.\d+:)", l):
            cur = [l + " " + (body[i + 1] if i + 1 < len(body) else ""), []]
            blocks.append(cur)
        elif cur is not None:
            cur[1].append(l.strip())
    heads = [b for b in blocks if "Loop Header: Depth=1" in b[0]]
    def members(h):
        tag = "Header=" + h[0].split(":")[0].replace(".L", "", 1) + " "
        return [b for b in blocks if b is h or (tag in b[0] and "Depth=1" in b[0])]
    head = max(heads, key=lambda h: sum(len(b[1]) for b in members(h)))
    mem = members(head)
    k = mem.index(head)
    mem = mem[k:] + mem[:k]  # from the header in program order; latch blocks above the header count as loop control at the end
    # a block entered through s_cbranch_execz (only some waves run it) is reported on its own
    phase, rows, order = 0, {}, []
    def acc(name, op):
        r = rows.setdefault(name, {"pk": 0, "plain": 0, "cnd": 0, "mov": 0, "addr": 0, "lds": 0, "ldsB": 0, "salu": 0, "vmem": 0})
        if name not in order:
            order.append(name)
        c = classify(op)
        if c is None:
            return
        r[c] += 1
        if c == "lds":
            r["ldsB"] += lds_bytes(op)
    prev_execz = False
    for lab, ins in mem:
        cond = prev_execz
        prev_execz = False
        for l in ins:
            if not l or l.startswith((";", ".")):
                continue
            op = l.split()[0]
            acc(f"cond{phase}" if cond else f"phase{phase}", op)
            if op == "s_barrier":
                phase += 1
            if op == "s_cbranch_execz":
                prev_execz = True
    hdr = f"{'phase':8s} {'pk':>5s} {'plain':>5s} {'cnd':>4s} {'mov':>4s} {'addr':>4s} {'VALU':>5s} {'LDS':>4s} {'LDS B':>6s} {'SALU':>5s} {'VMEM':>4s} {'cycles':>7s}"
    print(hdr)
    tot = {}
    for n in order:
        r = rows[n]
        valu = r["pk"] + r["plain"] + r["cnd"] + r["mov"] + r["addr"]
        cyc = 5 * r["pk"] + 2.7 * (valu - r["pk"]) + r["ldsB"] * 64 / 128
        print(f"{n:8s} {r['pk']:5d} {r['plain']:5d} {r['cnd']:4d} {r['mov']:4d} {r['addr']:4d} {valu:5d} {r['lds']:4d} {r['ldsB']:6d} {r['salu']:5d} {r['vmem']:4d} {cyc:7.0f}")
        if not n.startswith("cond"):
            for k, v in r.items():
                tot[k] = tot.get(k, 0) + v
    r = tot
    valu = r["pk"] + r["plain"] + r["cnd"] + r["mov"] + r["addr"]
    cyc = 5 * r["pk"] + 2.7 * (valu - r["pk"]) + r["ldsB"] * 64 / 128
    print(f"{'total':8s} {r['pk']:5d} {r['plain']:5d} {r['cnd']:4d} {r['mov']:4d} {r['addr']:4d} {valu:5d} {r['lds']:4d} {r['ldsB']:6d} {r['salu']:5d} {r['vmem']:4d} {cyc:7.0f}")
    print(f"(VALU cycles {5 * r['pk'] + 2.7 * (valu - r['pk']):.0f}, LDS cycles {r['ldsB'] * 64 / 128:.0f}; cond* blocks excluded from the total)")


if __name__ == "__main__":
    main()
