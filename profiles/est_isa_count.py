"""Counts what a wave of k_estimate_prod executes, from the listing of `make -C hmmufotu_amd/csrc asm` (hipcc -S, device only).  Nothing runs
on a GPU.

  python3 profiles/est_isa_count.py hu_engine.s [--kernel '<6,4,4,false>'] [--uniform TNN...] [--idle 3,7]

1. Barriers.  Over the kernel's control-flow graph, with every conditional branch taken both ways, the set of s_barrier counts a wave can
   have passed when it reaches s_endpgm, and every edge into s_endpgm with its set.  The kernel is right only if the set is {0, N}: 0 for
   the workgroup-uniform early return, which leaves ahead of the first barrier, N for every other path, whatever the wave's role.
   One refinement: a branch on exec whose basic block does not write exec in front of it (the compiler's `s_cbranch_execnz A; s_branch B`
   behind a uniform branch) goes the way of "exec is not zero": a wave does not run with an empty mask, every masked region of the listing
   is entered through a branch that skips it.
2. One path.  The walk follows the listing; a branch on exec (s_cbranch_execz / execnz) is decided as "some lane is active" unless its
   ordinal on the path is named in --idle, a branch on scc / vcc (uniform: the early return, builder or not, weighted or not, wnr == 0) by
   the next letter of --uniform (T = taken, N = not taken; asked for one by one: the script prints every decision with the branch's line,
   and stops with the line of the first branch it has no letter for).  It prints the vector instructions (VALU; LDS; vector memory) and the
   scalar ones between the markers of the path: the first message load (global_load_dword of the exponents), every s_barrier, s_endpgm;
   and any global_load behind the first barrier (every message load stands in front of it), which is what the table build must not have."""
import argparse
import re
import sys

NAMES = {  # template arguments -> mangled prefix
    "<2,4>": "ILi2ELi4ELi1ELb0EE", "<4,4>": "ILi4ELi4ELi1ELb0EE", "<6,4,4,false>": "ILi6ELi4ELi4ELb0EE", "<6,4,4,true>": "ILi6ELi4ELi4ELb1EE",
    "<6,4,1>": "ILi6ELi4ELi1ELb0EE", "<8,4>": "ILi8ELi4ELi1ELb0EE", "<12,4>": "ILi12ELi4ELi1ELb0EE", "<12,2>": "ILi12ELi2ELi1ELb0EE",
    "<6,8,2>": "ILi6ELi8ELi2ELb0EE",
}


def kernel_lines(path, inst):
    txt = open(path).read().split("\n")
    pref = "_Z15k_estimate_prod" + NAMES[inst]
    a = next(i for i, l in enumerate(txt) if l.startswith(pref) and l.split(";")[0].rstrip().endswith(":"))
    b = next(i for i in range(a, len(txt)) if txt[i].startswith(".Lfunc_end"))
    out = []
    for i in range(a + 1, b):
        l = txt[i].split(";")[0].strip()
        if l and not l.startswith(".") or re.match(r"\.LBB\d+_\d+:", l):
            out.append((i + 1, l))
    return out


def kind(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "scratch_", "buffer_", "flat_")):
        return "vmem"
    if op.startswith("s_"):
        return "salu"
    return None


def exec_written(L, i):
    """is exec written between the start of the branch's basic block and the branch at index i"""
    j = i - 1
    while j >= 0 and not L[j][1].endswith(":") and not L[j][1].startswith(("s_cbranch", "s_branch")):
        if re.search(r"saveexec|\bexec\b", L[j][1].split(",")[0]):
            return True
        j -= 1
    return False


def barrier_sets(L):
    """per listing index: the set of barrier counts on arrival, all branches both ways"""
    lab = {l[:-1]: i for i, (_, l) in enumerate(L) if l.endswith(":")}
    arrive = [set() for _ in L]
    arrive[0].add(0)
    ends = {}
    work = [0]
    while work:
        i = work.pop()
        _, l = L[i]
        op = l.split()[0]
        cnt = {c + (op == "s_barrier") for c in arrive[i]}
        nxt = []
        if op == "s_endpgm":
            continue
        if op == "s_branch":
            nxt = [lab[l.split()[1]]]
        elif op.startswith("s_cbranch_exec") and not exec_written(L, i):
            nxt = [lab[l.split()[1]] if op == "s_cbranch_execnz" else i + 1]
        elif op.startswith("s_cbranch"):
            nxt = [lab[l.split()[1]], i + 1]
        else:
            nxt = [i + 1]
        for j in nxt:
            if L[j][1].split()[0] == "s_endpgm" or (L[j][1].endswith(":") and L[j + 1][1] == "s_endpgm"):
                ends.setdefault(L[i][0], set()).update(cnt)
            if not cnt <= arrive[j]:
                arrive[j] |= cnt
                work.append(j)
    return ends


def walk(L, uniform, idle):
    lab = {l[:-1]: i for i, (_, l) in enumerate(L) if l.endswith(":")}
    seg = dict(valu=0, lds=0, vmem=0, salu=0)
    segs, marks, notes = [], ["entry"], []
    i, nu, ne, seen_load, nbar = 0, 0, 0, False, 0

    def close(mark):
        nonlocal seg
        segs.append(seg)
        marks.append(mark)
        seg = dict(valu=0, lds=0, vmem=0, salu=0)

    while True:
        ln, l = L[i]
        if l.endswith(":"):
            i += 1
            continue
        op = l.split()[0]
        if op == "global_load_dword" and not seen_load:
            seen_load = True
            close("first message load (line %d)" % ln)
        if op.startswith("global_load") and nbar >= 1:
            notes.append("line %d: %s behind barrier %d" % (ln, l, nbar))
        k = kind(op)
        if k:
            seg[k] += 1
        if op == "s_barrier":
            nbar += 1
            close("barrier %d (line %d)" % (nbar, ln))
        if op == "s_endpgm":
            close("s_endpgm (line %d)" % ln)
            return segs, marks, notes, nbar
        if op == "s_branch":
            i = lab[l.split()[1]]
            continue
        if op.startswith("s_cbranch_exec"):
            active = ne not in idle
            taken = (op == "s_cbranch_execnz") == active
            print("  exec branch %2d, line %d: %-34s lanes %s" % (ne, ln, l, "active" if active else "idle"))
            ne += 1
            i = lab[l.split()[1]] if taken else i + 1
            continue
        if op.startswith("s_cbranch"):
            if nu >= len(uniform):
                sys.exit("uniform branch %d at line %d (%s): no letter left in --uniform" % (nu, ln, l))
            taken = uniform[nu] == "T"
            print("  uniform branch %2d, line %d: %-31s %s" % (nu, ln, l, "taken" if taken else "not taken"))
            nu += 1
            i = lab[l.split()[1]] if taken else i + 1
            continue
        i += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("--kernel", default="<6,4,4,false>", choices=sorted(NAMES))
    ap.add_argument("--uniform", default="")
    ap.add_argument("--idle", default="")
    a = ap.parse_args()
    L = kernel_lines(a.listing, a.kernel)
    ends = barrier_sets(L)
    allc = set().union(*ends.values())
    print("k_estimate_prod%s: barrier counts at s_endpgm over all paths: %s" % (a.kernel, sorted(allc)))
    for ln, c in sorted(ends.items()):
        print("  edge into s_endpgm from line %d: %s" % (ln, sorted(c)))
    if a.uniform or a.idle:
        idle = {int(x) for x in a.idle.split(",") if x}
        segs, marks, notes, nbar = walk(L, a.uniform, idle)
        tot = dict(valu=0, lds=0, vmem=0, salu=0)
        for s, m0, m1 in zip(segs, marks, marks[1:]):
            print("%-36s -> %-36s VALU %4d  LDS %3d  VMEM %3d  scalar %4d" % (m0, m1, s["valu"], s["lds"], s["vmem"], s["salu"]))
            for k in tot:
                tot[k] += s[k]
        print("path: %d barriers, vector instructions %d (VALU %d, LDS %d, VMEM %d), scalar %d" %
              (nbar, tot["valu"] + tot["lds"] + tot["vmem"], tot["valu"], tot["lds"], tot["vmem"], tot["salu"]))
        for n in notes:
            print("  NOTE", n)


if __name__ == "__main__":
    main()
