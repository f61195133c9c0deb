#!/usr/bin/env python3
"""Host time of every ingest route on two builds, route for route: what a change of the host side alone can move.

    python tools/ingest_sources_ab.py --parent <tree of the parent commit, built> [--out profiles/ingest_sources_ab.txt]

Shapes 1 M x 20, 5 M x 14 and 2 M x 40.  Five sources in pageable memory - C float64, C float32, Fortran float32 (a
columns-form view), C-pitched float32 (d of d + 26 columns: a rows-form view), big-endian float32 event records of d + 10
channels - and three operations, each to the moment cc_sync returns: upload, prefetch followed at once by the adopting upload,
assign against a settled table of 5 000 rows.  Per visit: 7 calls after 2 warm-ups.  The two builds run in alternation on one
machine, one child process per visit, each build twice per shape in the order A B B A, the other build first at every other
shape - what a process pays for coming first or last falls on both builds.  Per figure: the median of a build's 14 calls, minimum
and maximum beside it, and the medians of its two visits.  A route is "unchanged" when each build's median lies inside the
other's [min .. max]."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1000000, 20), (5000000, 14), (2000000, 40)]
SOURCES = ("C float64", "C float32", "Fortran float32", "C-pitched float32", "big-endian float32 records")
OPS = ("upload", "prefetch+upload", "assign")
WARM, CALLS = 2, 7


def child(tree, n, d):
    """Runs in a process of its own with `tree` first on the path: prints one JSON object, source -> op -> [ms per call]."""
    sys.path.insert(0, tree)
    import numpy as np
    from chronoclust_amd import _lib
    rng = np.random.default_rng(n + d)
    centres = rng.uniform(0.1, 0.9, (5000, d))
    x64 = np.clip(centres[rng.integers(0, 5000, n)] + rng.normal(0.0, 0.01, (n, d)), 0.0, 1.0)
    x32 = np.ascontiguousarray(x64, dtype=np.float32)
    wide = np.zeros((n, d + 26), dtype=np.float32)
    wide[:, :d] = x32
    rec = np.zeros((n, d + 10), dtype=">f4")
    rec[:, 5:5 + d] = x32
    arrays = {"C float64": x64, "C float32": x32, "Fortran float32": np.asfortranarray(x32), "C-pitched float32": wide[:, :d],
              "big-endian float32 records": _lib.ListMode(rec.tobytes(), n, d + 10, ">f4", columns=np.arange(5, 5 + d))}
    del rec
    h = _lib.Handle(0)
    h.set_params(0.05 ** 2, 0.05 ** 2, 4.0, 0.5, 20.0, 0.0, 6.5 * 0.05, (6.5 * 0.05) ** 2, 0.05, d)
    h.inject_bulk(_lib.PCORE, centres * 50.0, (centres * centres + 1e-4) * 50.0, centres, np.ones((5000, d)), np.full(5000, 50.0),
                  np.arange(5000), np.arange(5000))

    def op(name, x):
        if name == "assign":
            h.assign(x)
        else:
            if name == "prefetch+upload":
                h.points_prefetch(x)
            h.points_upload(x)
        h.sync()

    out = {}
    for source in SOURCES:
        x = arrays[source]
        assert isinstance(x, _lib.ListMode) or _lib.points_source(x)[0] is x
        out[source] = {}
        for name in OPS:
            ms = []
            for _ in range(WARM + CALLS):
                t0 = time.perf_counter()
                op(name, x)
                ms.append((time.perf_counter() - t0) * 1e3)
            out[source][name] = ms[WARM:]
    out["counters"] = {k: h.stats()[k] for k in ("f32_points", "view_points", "list_points")}
    h.close()
    print("RESULT " + json.dumps(out))


def summary(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_sources_ab.txt"))
    ap.add_argument("--child", nargs=3, metavar=("TREE", "N", "D"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]), int(args.child[2]))
        return 0
    if not args.parent:
        ap.error("--parent is required")
    trees = (("parent", os.path.abspath(args.parent)), ("this", ROOT))
    res = {}
    for i, (n, d) in enumerate(SHAPES):
        first, second = trees if i % 2 == 0 else trees[::-1]
        for label, tree in (first, second, second, first):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, str(n), str(d)], capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:  # (nothing more is started on the device after a failure)
                sys.stderr.write(p.stdout + p.stderr)
                return 1
            res.setdefault((n, d, label), []).append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    lines = ["python tools/ingest_sources_ab.py --parent <parent tree>: source (pageable) -> cc_sync, ms; per build two visits (A B B A) "
             "of %d calls after %d warm-ups: median of the %d calls [min .. max] (the medians of the two visits).  unchanged: each "
             "median inside the other build's [min .. max]." % (CALLS, WARM, 2 * CALLS), ""]
    moved = 0
    for n, d in SHAPES:
        lines.append("%d x %d" % (n, d))
        for source in SOURCES:
            for name in OPS:
                fig = {}
                for label in ("parent", "this"):
                    visits = [r[source][name] for r in res[(n, d, label)]]
                    fig[label] = summary(visits[0] + visits[1]) + tuple(summary(v)[0] for v in visits)
                a, b = fig["parent"], fig["this"]
                same = a[1] <= b[0] <= a[2] and b[1] <= a[0] <= b[2]
                moved += not same
                lines.append("  %-27s %-16s parent %8.2f [%8.2f .. %8.2f] (%8.2f, %8.2f)   this %8.2f [%8.2f .. %8.2f] (%8.2f, %8.2f)   %+6.2f ms  %s"
                             % ((source, name) + a + b + (b[0] - a[0], "unchanged" if same else "OUTSIDE")))
        counters = {label: [r["counters"] for r in res[(n, d, label)]] for label in ("parent", "this")}
        same_counters = all(c == counters["this"][0] for c in counters["parent"] + counters["this"])
        lines.append("  counters %s: %s" % ("the same on both builds" if same_counters else "DIFFER", counters["this"][0]))
        lines.append("")
    lines.append("%d of %d routes outside the other build's spread" % (moved, len(SHAPES) * len(SOURCES) * len(OPS)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
