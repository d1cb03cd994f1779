#!/usr/bin/env python3
"""Prints the instruction histogram of one kernel of /tmp/qpn_isa/<file>.s OUTSIDE the loop that contains a marker
instruction: the lines before the loop's header and the lines behind its latch, each with its own histogram (developer aid
for counting issue slots; the companion of tools/isa_loop.py, which prints the loop itself).  A listing holds every path, also
those a wavefront does not take: the counters decide what is executed (tools/pivot_cost.sh).

    tools/isa_outside.py <file.s> <kernel symbol prefix> <marker> [-l before|after] [-g <regex>]

-l prints the lines of one side, -g only those of them that match."""
import collections
import re
import sys


def kernel_lines(path, kern):
    L = open(path).read().split("\n")
    st = [i for i, x in enumerate(L) if x.startswith(kern)][0]
    en = [i for i, x in enumerate(L) if x.startswith(".Lfunc_end") and i > st][0]
    return L[st:en]


def loop_bounds(K, marker):
    """(header line, line behind the latch) of the innermost loop around the last line that holds the marker."""
    mk = [i for i, x in enumerate(K) if marker in x]
    hd = [i for i, x in enumerate(K) if "Loop Header" in x]
    a = max(h for h in hd if h <= mk[-1])
    tgt = {K[a].split(":")[0]}
    for i in range(a - 1, max(a - 40, 0), -1):      # flow labels that fall into the header
        if K[i].startswith(".LBB"):
            tgt.add(K[i].split(":")[0])
        elif K[i].strip().startswith(("s_branch", "s_endpgm")):
            break
    b = max(i for i, x in enumerate(K) if "branch" in x and any(x.strip().endswith(" " + t) for t in tgt)) + 1
    return a, b


def code(lines):
    return [x for x in lines if x.strip() and not x.strip().startswith(";") and not x.strip().startswith(".") and not x.rstrip().endswith(":")]


def main():
    path, kern, marker = sys.argv[1:4]
    K = kernel_lines(path, kern)
    a, b = loop_bounds(K, marker)
    sides = {"before": code(K[:a]), "after": code(K[b:])}
    for name, body in sides.items():
        c = collections.Counter(x.split()[0] for x in body)
        kinds = collections.Counter("VALU" if o.startswith("v_") else "SALU" if o.startswith("s_") else "LDS" if o.startswith("ds_")
                                    else "VMEM" if o.startswith(("global_", "buffer_", "flat_", "scratch_")) else "other" for o in c.elements())
        print(f"{name} the loop: {len(body)} instructions", dict(kinds))
        print(sorted(c.items(), key=lambda t: -t[1])[:48])
    if "-l" in sys.argv:
        body = sides[sys.argv[sys.argv.index("-l") + 1]]
        pat = re.compile(sys.argv[sys.argv.index("-g") + 1]) if "-g" in sys.argv else None
        print("\n".join(x for x in body if pat is None or pat.search(x)))


if __name__ == "__main__":
    main()
