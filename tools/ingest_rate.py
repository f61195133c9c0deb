#!/usr/bin/env python3
"""What a float32 user pays to get points onto the device, before and after the single-precision entry points.

    python tools/ingest_rate.py --parent <tree of the parent commit, built> [--out profiles/ingest_f32.txt]

Shapes 1 M x 20, 5 M x 14 and 2 M x 40.  Three operations, each from a float32 numpy array in pageable memory to the
moment cc_sync returns: upload (to resident points), assign (against a settled table of 5 000 rows), and prefetch followed
at once by the adopting upload (nothing overlaps it here: the whole of the worker's time is exposed).  Three routes:
  (a) np.ascontiguousarray(x32, np.float64) inside the bracket, then the float64 call - what a float32 user pays on the
      parent commit, measured on the parent's build;
  (b) the float64 call on an array that already is float64 - on the parent's build and on this one (its code is untouched);
  (c) the float32 route of this build.
Per figure: the median of 7 calls after 2 warm-ups, minimum and maximum beside it.  The two builds run in alternation on one
machine, one child process per (build, shape) and the other build first at every other shape, so that neither sits on a
warmer or a busier stretch of it.  The verdicts at
the end: (c) below (a) by more than the spread (max - min) of either; (b) of the two builds within that spread."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1000000, 20), (5000000, 14), (2000000, 40)]
OPS = ("upload", "assign", "prefetch+upload")
WARM, CALLS = 2, 7


def child(tree, n, d):
    """Runs in a process of its own with `tree` first on the path: prints one JSON object, op -> route -> [ms per call]."""
    sys.path.insert(0, tree)
    import numpy as np
    from chronoclust_amd import _lib
    has_f32 = hasattr(_lib, "as_points")
    rng = np.random.default_rng(n + d)
    centres = rng.uniform(0.1, 0.9, (5000, d))
    x32 = np.ascontiguousarray(np.clip(centres[rng.integers(0, 5000, n)] + rng.normal(0.0, 0.01, (n, d)), 0.0, 1.0), dtype=np.float32)
    x64 = np.ascontiguousarray(x32, dtype=np.float64)
    h = _lib.Handle(0)
    # a settled table: 5 000 pcore rows, one per centre, each of weight 50 and a little variance
    w = np.full(5000, 50.0)
    cf1 = centres * 50.0
    cf2 = (centres * centres + 1e-4) * 50.0
    h.set_params(0.05 ** 2, 0.05 ** 2, 4.0, 0.5, 20.0, 0.0, 6.5 * 0.05, (6.5 * 0.05) ** 2, 0.05, d)
    h.inject_bulk(_lib.PCORE, cf1, cf2, centres, np.ones((5000, d)), w, np.arange(5000), np.arange(5000))

    def op(name, x):
        if name == "upload":
            h.points_upload(x)
        elif name == "assign":
            h.assign(x)
        else:
            h.points_prefetch(x)
            h.points_upload(x)
        h.sync()

    routes = {"a": lambda name: op(name, np.ascontiguousarray(x32, dtype=np.float64)), "b": lambda name: op(name, x64)}
    if has_f32:
        routes["c"] = lambda name: op(name, x32)
    out = {}
    for name in OPS:
        out[name] = {}
        for route, call in sorted(routes.items()):
            ms = []
            for i in range(WARM + CALLS):
                t0 = time.perf_counter()
                call(name)
                ms.append((time.perf_counter() - t0) * 1e3)
            out[name][route] = ms[WARM:]
    if has_f32:
        out["f32_points"] = h.stats()["f32_points"]
    h.close()
    print("RESULT " + json.dumps(out))


def summary(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_f32.txt"))
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
        for label, tree in (trees if i % 2 == 0 else trees[::-1]):  # (the builds alternate, and so does which of them goes first)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, str(n), str(d)], capture_output=True,
                               text=True, timeout=900)
            if p.returncode != 0:  # (nothing more is started on the device after a failure)
                sys.stderr.write(p.stdout + p.stderr)
                return 1
            res[(n, d, label)] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    lines = ["python tools/ingest_rate.py --parent <parent tree>: float32 numpy array (pageable) -> cc_sync, ms; median of %d calls"
             " after %d warm-ups [min .. max].  (a) widen on the host + float64 call, parent build; (b) float64 call on a float64"
             " array; (c) the float32 route." % (CALLS, WARM), ""]
    ok = True
    for n, d in SHAPES:
        lines.append("%d x %d (%.0f MB as float32, %.0f MB as float64)" % (n, d, n * d * 4 / 1e6, n * d * 8 / 1e6))
        for name in OPS:
            fig = {"a": summary(res[(n, d, "parent")][name]["a"]), "b parent": summary(res[(n, d, "parent")][name]["b"]),
                   "b this": summary(res[(n, d, "this")][name]["b"]), "c": summary(res[(n, d, "this")][name]["c"])}
            for key in ("a", "b parent", "b this", "c"):
                med, lo, hi = fig[key]
                lines.append("  %-16s (%-8s) %9.2f  [%9.2f .. %9.2f]   %7.1f M points/s" % (name, key, med, lo, hi, n / med / 1e3))
            spread_ac = max(fig["a"][2] - fig["a"][1], fig["c"][2] - fig["c"][1])
            spread_b = max(fig["b parent"][2] - fig["b parent"][1], fig["b this"][2] - fig["b this"][1])
            c_below_a = fig["a"][0] - fig["c"][0] > spread_ac
            b_same = abs(fig["b this"][0] - fig["b parent"][0]) <= spread_b
            ok = ok and c_below_a and b_same
            lines.append("  %-16s (c) below (a) by %.2f ms, spread %.2f ms: %s;  (b) this - parent = %+.2f ms, spread %.2f ms: %s;  (c) / (b this) = %.2f"
                         % (name, fig["a"][0] - fig["c"][0], spread_ac, "holds" if c_below_a else "DOES NOT HOLD",
                            fig["b this"][0] - fig["b parent"][0], spread_b, "holds" if b_same else "DOES NOT HOLD",
                            fig["c"][0] / fig["b this"][0]))
        lines.append("")
    lines.append("all verdicts hold" if ok else "a verdict does not hold")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
