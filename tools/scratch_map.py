#!/usr/bin/env python3
"""Static map of the register spills of rppk2t::rrt_star_kernel_v2 (the one-wave RRT* kernel), from device assembly kept by
    KEEP_ASM=a.s tools/loop_spill_check.sh [csrc directory]
    KEEP_ASM=g.s tools/loop_spill_check.sh [csrc directory] -gline-tables-only      (optional: the per-file table)
Usage: tools/scratch_map.py a.s [g.s]

Prints, per spill slot (the scratch offset): static spills, static reloads and the opcodes that read a reloaded register
before it is written again; per code region delimited by the six streaming loops (the loop finder of
loop_spill_check.sh): scratch instructions and reloads; with g.s the same counts per source file of the .loc lines.
Spill code is recognised as loop_spill_check.sh does: a `scratch_` instruction carrying the compiler's `Folded Spill` /
`Folded Reload` comment.  Everything is static (instructions in the binary, not instructions executed): a map for
choosing what to take out of scratch, and the gate of DESIGN.md 6.0h.  CPU only."""
import re
import sys
from collections import Counter, defaultdict

KERNEL = "_ZN6rppk2t18rrt_star_kernel_v2EN4rppk3CtxEi:"
WINDOW = 400   # instructions searched for the consumers of a reload
# instructions without a destination in their first operand
NO_DEST = re.compile(r"^(scratch_store|global_store|flat_store|buffer_store|ds_write|v_cmp|v_cmpx|s_cmp|s_waitcnt|s_nop|s_cbranch|s_branch|s_barrier)")
REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def kernel_lines(path):
    L = open(path).read().split("\n")
    try:
        a = next(i for i, l in enumerate(L) if l.startswith(KERNEL))
    except StopIteration:
        sys.exit("%s: no %s" % (path, KERNEL))
    b = next(i for i in range(a, len(L)) if "s_endpgm" in L[i])
    return L[a:b + 1]


def regs(text):
    s = set()
    for m in REG.finditer(text):
        if m.group(1) is not None:
            s.add(int(m.group(1)))
        else:
            s.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return s


def split_ins(line):
    """(opcode, [operands]) of an instruction line, or None for labels, directives and comments"""
    t = line.split(";")[0].strip()
    if not t or t.startswith(".") or t.endswith(":"):
        return None
    p = t.split(None, 1)
    return p[0], ([o.strip() for o in p[1].split(",")] if len(p) > 1 else [])


def is_spill(l):
    return "scratch_" in l and "Folded Spill" in l


def is_reload(l):
    return "scratch_" in l and "Folded Reload" in l


def slot_of(l):
    m = re.search(r"offset:(\d+)", l)
    return int(m.group(1)) if m else 0


def consumers(L, i):
    """opcodes reading the registers that the reload at line i defines, until each is written again"""
    op, ops = split_ins(L[i])
    live = regs(ops[0])
    out = []
    seen = 0
    for l in L[i + 1:]:
        ins = split_ins(l)
        if ins is None:
            continue
        seen += 1
        if seen > WINDOW or not live:
            break
        o, a = ins
        nodest = NO_DEST.match(o) is not None
        for k, text in enumerate(a):
            if k == 0 and not nodest:
                continue
            if regs(text) & live:
                tag = o
                if o.startswith("ds_bpermute") or o.startswith("ds_permute"):
                    tag = o + (":addr" if k == 1 else ":data")
                out.append(tag)
                break
        if a and not nodest:
            live -= regs(a[0])
    return out


def loops(L):
    """[first, last] line of every streaming loop, as loop_spill_check.sh finds them"""
    loads = [i for i, l in enumerate(L) if "global_load_dwordx4" in l and " nt" in l]
    if not loads:
        return []
    groups, cur = [], [loads[0]]
    for a, b in zip(loads, loads[1:]):
        if b - a < 60:
            cur.append(b)
        else:
            groups.append(cur)
            cur = [b]
    groups.append(cur)
    res, i = [], 0
    while i < len(groups):
        g = groups[i]
        if len(g) >= 2:
            j, last = i + 1, g[-1]
            while j < len(groups) and len(groups[j]) == 1:
                last = groups[j][0]
                j += 1
            if j > i + 1:
                res.append((g[-1], last))
            i = j
        else:
            i += 1
    return res


def slot_table(L):
    spills, reloads, cons = Counter(), Counter(), defaultdict(Counter)
    bperm = qd = 0
    for i, l in enumerate(L):
        if is_spill(l):
            spills[slot_of(l)] += 1
        elif is_reload(l):
            s = slot_of(l)
            reloads[s] += 1
            c = consumers(L, i)
            for o in set(c):
                cons[s][o] += 1
            bperm += any(o.endswith(":addr") for o in c)
            qd += any(o.startswith("v_pk_sub_i16") or o.startswith("v_dot2_i32_i16") for o in c)
    print("spill slots of rppk2t::rrt_star_kernel_v2: %d slots, %d static spills, %d static reloads, %d scratch instructions"
          % (len(set(spills) | set(reloads)), sum(spills.values()), sum(reloads.values()), sum("scratch_" in l for l in L)))
    print("reloads whose consumer is a ds_bpermute / ds_permute address: %d" % bperm)
    print("reloads that feed v_pk_sub_i16 / v_dot2_i32_i16 (qdist): %d" % qd)
    print("%6s %7s %8s  consumers (reloads that reach the opcode)" % ("slot", "spills", "reloads"))
    for s in sorted(set(spills) | set(reloads), key=lambda s: (-reloads[s], s)):
        print("%6d %7d %8d  %s" % (s, spills[s], reloads[s], " ".join("%s:%d" % kv for kv in cons[s].most_common(6))))


def region_table(L):
    lp = loops(L)
    edges = [0]
    for a, b in lp:
        edges += [a, b + 1]
    edges.append(len(L))
    names = []
    for k in range(len(lp)):
        names += ["before loop %d" % (k + 1) if k == 0 else "between loops %d and %d" % (k, k + 1), "loop %d" % (k + 1)]
    names.append("after loop %d" % len(lp) if lp else "whole kernel")
    print("\n%d streaming loops; regions of the kernel (asm lines from the kernel's label):" % len(lp))
    print("%-26s %15s %9s %8s" % ("region", "lines", "scratch", "reloads"))
    for k, name in enumerate(names):
        a, b = edges[k], edges[k + 1]
        seg = L[a:b]
        print("%-26s %7d-%-7d %9d %8d" % (name, a, b - 1, sum("scratch_" in l for l in seg), sum(is_reload(l) for l in seg)))


def file_table(L, whole):
    files = {}
    for l in whole:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            files[int(m.group(1))] = (m.group(3) or m.group(2)).split("/")[-1]
    cur = "?"
    sp, rl = Counter(), Counter()
    for l in L:
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
        if m:
            cur = "%s" % files.get(int(m.group(1)), m.group(1))
        elif is_spill(l):
            sp[cur] += 1
        elif is_reload(l):
            rl[cur] += 1
    print("\nper source file (-gline-tables-only build; that flag shifts the allocation a little: a map, not a gate):")
    print("%-34s %7s %8s" % ("file", "spills", "reloads"))
    for f in sorted(set(sp) | set(rl), key=lambda f: -rl[f]):
        print("%-34s %7d %8d" % (f, sp[f], rl[f]))
    print("%-34s %7d %8d" % ("total", sum(sp.values()), sum(rl.values())))


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    L = kernel_lines(sys.argv[1])
    slot_table(L)
    region_table(L)
    if len(sys.argv) > 2:
        file_table(kernel_lines(sys.argv[2]), open(sys.argv[2]).read().split("\n"))


if __name__ == "__main__":
    main()
