#!/usr/bin/env python3
"""Did a change of the source leave the generated kernels alone?  Two builds of the same kernels from the compiler's assembly
(`hipcc <the Makefile's flags> --cuda-device-only -S`), compared kernel symbol by kernel symbol:

  - VGPR / SGPR / static LDS / scratch from the kernel descriptor, the occupancy the compiler states
  - instruction counts
  - lines that differ once branch labels are numbered in their order of appearance and comments are dropped
  - the difference of the two opcode multisets, as a whole and for the vector-ALU and the memory opcodes alone

python tools/investigations/isa_same_kernels.py <parent.s>[,<parent2.s>...] <branch.s>[,<branch2.s>...] [symbol-substring]
(a side may be several files: kernels that moved to another translation unit are found by their symbol).  Exit status 1 when a kernel
is missing on one side or a descriptor figure differs; differences of the text are reported, not judged."""
import collections
import difflib
import re
import sys

FIGURES = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size"))
MEMORY = ("global_", "buffer_", "ds_", "flat_", "scratch_")


def kernels(paths):
    """symbol -> {"ins": [normalised instruction lines], "fig": {...}}"""
    out = {}
    for path in paths.split(","):
        lines = open(path).read().split("\n")
        descr = {}
        for i, l in enumerate(lines):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
            if not m:
                continue
            fig = {}
            for k in range(i + 1, len(lines)):
                if ".end_amdhsa_kernel" in lines[k]:
                    break
                d = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", lines[k])
                if d:
                    fig[d.group(1)] = d.group(2)
            for k in range(i + 1, len(lines)):          # (the compiler's summary comment behind the descriptor)
                o = re.match(r";\s*Occupancy:\s*(\d+)", lines[k])
                if o or ".amdhsa_kernel " in lines[k]:
                    fig["occupancy"] = o.group(1) if o else "?"
                    break
            descr[m.group(1)] = fig
        for sym, fig in descr.items():
            start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
            end = next(i for i in range(start, len(lines)) if re.match(r"\s*\.section|\s*\.amdhsa_kernel", lines[i]))
            labels, ins = {}, []
            for l in lines[start + 1:end]:
                l = l.split(";")[0].rstrip()
                if not l.startswith("\t") or l.strip().startswith("."):
                    continue
                l = re.sub(r"\.LBB\d+_\d+", lambda m: "L%d" % labels.setdefault(m.group(0), len(labels)), " ".join(l.split()))
                ins.append(l)
            out[sym] = {"ins": ins, "fig": fig}
    return out


def multiset_diff(a, b, keep=lambda op: True):
    ca = collections.Counter(l.split()[0] for l in a if keep(l.split()[0]))
    cb = collections.Counter(l.split()[0] for l in b if keep(l.split()[0]))
    return {op: cb[op] - ca[op] for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]}


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    parent, branch = kernels(sys.argv[1]), kernels(sys.argv[2])
    only = sys.argv[3] if len(sys.argv) > 3 else ""
    bad = 0
    print("| kernel | VGPR | SGPR | LDS | scratch | occupancy | instructions | differing lines | opcodes | VALU opcodes | memory opcodes |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for sym in sorted(set(parent) | set(branch)):
        if only not in sym:
            continue
        if sym not in parent or sym not in branch:
            print(f"| {sym} | only in the {'parent' if sym in parent else 'branch'} |")
            bad = 1
            continue
        p, b = parent[sym], branch[sym]
        cells = []
        for _, key in FIGURES + (("occupancy", "occupancy"),):
            x, y = p["fig"].get(key, "?"), b["fig"].get(key, "?")
            cells.append(x if x == y else f"**{x} -> {y}**")
            bad |= x != y
        n0, n1 = len(p["ins"]), len(b["ins"])
        cells.append(str(n0) if n0 == n1 else f"{n0} -> {n1} ({100.0 * (n1 - n0) / n0:+.2f} %)")
        sm = difflib.SequenceMatcher(None, p["ins"], b["ins"], autojunk=False)
        cells.append(str(sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")))
        for keep in (lambda op: True, lambda op: op.startswith("v_"), lambda op: op.startswith(MEMORY)):
            d = multiset_diff(p["ins"], b["ins"], keep)
            cells.append("same" if not d else " ".join(f"{op}{n:+d}" for op, n in d.items()))
        print(f"| {sym} | " + " | ".join(cells) + " |")
    sys.exit(bad)


if __name__ == "__main__":
    main()
