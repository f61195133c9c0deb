#!/usr/bin/env python3
"""The launch sequence of a run, one line per kernel dispatch, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o <name> -- <program>
    python tools/launch_list.py <dir or ..._kernel_trace.csv> > launches.txt

Per dispatch, in dispatch-id order (the order the host enqueued them): the kernel's short name (template arguments kept,
`void` and the parameter list dropped), the grid in work-items as the trace gives it, and the workgroup size.  Two builds
that launch the same kernels with the same geometry in the same order give the same text: `diff` is the comparison."""
import csv
import glob
import os
import re
import sys


def short(name):
    name = re.sub(r"\.kd$", "", name.strip())
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, ch in enumerate(name):  # cut at the parameter list: the first "(" outside the template arguments
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    path = sys.argv[1]
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if len(found) != 1:
            sys.exit("%d kernel traces under %s" % (len(found), path))
        path = found[0]
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        print("%s grid %s,%s,%s wg %s,%s,%s" % ((short(r["Kernel_Name"]),) + tuple(r["Grid_Size_" + a] for a in "XYZ") +
                                                tuple(r["Workgroup_Size_" + a] for a in "XYZ")))


if __name__ == "__main__":
    main()
