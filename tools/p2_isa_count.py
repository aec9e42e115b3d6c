#!/usr/bin/env python3
"""Static instruction counts of kernels in a gfx950 assembly listing, basic block by basic block: how DESIGN.md section 3 counts the
VALU instructions of a permutation (block count x trip count, the trip counts read off the branches printed here).

    hipcc -S --offload-arch=gfx950 --cuda-device-only -O3 -std=c++17 lmcs.hip -o lmcs.s
    python tools/p2_isa_count.py lmcs.s k_leaf_absorb k_compress k_perm_rate

Per kernel: every basic block with its VALU count, lane moves between register files (v_readlane / v_writelane: SGPR spills), s_nop,
and the label its last branch goes to (a backward target closes a loop); then the kernel's totals.  --min N hides blocks with fewer
than N VALU instructions."""
import re, sys


def kernels(text):
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        out.setdefault(m.group(1), m.group(2))
    return out


def blocks(body):
    cur, res = ("entry", []), []
    for line in body.splitlines():
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            res.append(cur)
            cur = (m.group(1), [])
        else:
            ins = line.split(";")[0].strip()
            if ins and not ins.startswith("."):
                cur[1].append(ins)
                if ins.startswith(("s_cbranch", "s_branch")):  # the code behind a branch is a block of its own (no label: fall-through)
                    res.append(cur)
                    cur = (cur[0].rstrip("+") + "+", [])
    res.append(cur)
    return [b for b in res if b[1]]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    min_valu = int(sys.argv[sys.argv.index("--min") + 1]) if "--min" in sys.argv else 0
    if "--min" in sys.argv:
        args.remove(str(min_valu))
    text = open(args[0]).read()
    ks = kernels(text)
    for want in args[1:]:
        names = [k for k in ks if re.match(r"_Z\d+%s(?![a-z_])" % re.escape(want), k)]
        for name in names:
            bl = blocks(ks[name])
            order = {b[0]: i for i, b in enumerate(bl)}
            print(f"== {want} ({name})")
            tot = dict(valu=0, lane=0, nop=0, salu=0, smem=0, vmem=0)
            for i, (label, ins) in enumerate(bl):
                valu = sum(1 for x in ins if x.startswith("v_"))
                lane = sum(1 for x in ins if x.startswith(("v_readlane", "v_writelane")))
                nop = sum(1 for x in ins if x.startswith("s_nop"))
                smem = sum(1 for x in ins if x.startswith("s_load"))
                vmem = sum(1 for x in ins if x.startswith(("global_", "flat_", "scratch_", "buffer_")))
                salu = sum(1 for x in ins if x.startswith("s_")) - nop - smem
                for k, v in dict(valu=valu, lane=lane, nop=nop, salu=salu, smem=smem, vmem=vmem).items():
                    tot[k] += v
                br = [x.split()[-1] for x in ins if x.startswith(("s_cbranch", "s_branch"))]
                back = [t for t in br if t in order and order[t] <= i]
                if valu >= min_valu:
                    print(f"  {label:<12} VALU {valu:5d}  lane {lane:3d}  s_nop {nop:4d}  SALU {salu:4d}  s_load {smem:3d}  vmem {vmem:3d}"
                          f"  -> {' '.join(br) or '-'}{'   LOOP back to ' + ' '.join(back) if back else ''}")
            print("  total        " + "  ".join(f"{k} {v}" for k, v in tot.items()))


if __name__ == "__main__":
    main()
