#!/usr/bin/env python3
"""What a user whose points are column-major, pitched or narrow-typed pays to get them onto the device, before and after
the `_view` entry points.

    python tools/ingest_layouts.py --parent <tree of the parent commit, built> [--out profiles/ingest_layouts.txt]

Shapes 1 M x 20, 5 M x 14 and 2 M x 40.  One operation, from a numpy array in pageable memory to the moment cc_sync returns:
the upload to resident points.  Four sources - Fortran-order float64 (what pandas hands out for a parsed CSV), Fortran-order
float32, C-pitched float32 (14 of 40 columns; at 5 M x 14 that is the shape itself, at the others the first 14 columns of
40), C-contiguous uint16 - each on two routes:
  (a) as_points(x) inside the bracket, then the upload - what that user pays on the parent commit, on the parent's build;
  (b) points_upload(x) of this build: the array is read where it lies.
And the two routes of old, C-contiguous float64 and float32, on both builds (their code is untouched).
Per figure: the median of 7 calls after 2 warm-ups, minimum and maximum beside it.  The two builds run in alternation on one
machine, one child process per (build, shape) and the other build first at every other shape.  Then, on this build alone, the
Scaler(handle=...) fit plus the first timepoint of an app.run over CSV files (--csv-points rows x 20, three timepoints):
once as the CSVs are parsed, once with the parent's copy to a C-contiguous array put back in.
The verdicts at the end: (b) below (a) by more than the spread (max - min) of either; the old routes of the two builds within
that spread."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1000000, 20), (5000000, 14), (2000000, 40)]
SOURCES = ("Fortran float64", "Fortran float32", "C-pitched float32", "C uint16")
OLD = ("C float64", "C float32")
WARM, CALLS = 2, 7


def child(tree, n, d):
    """Runs in a process of its own with `tree` first on the path: prints one JSON object, source -> [ms per call]."""
    sys.path.insert(0, tree)
    import numpy as np
    from chronoclust_amd import _lib
    has_views = hasattr(_lib, "points_source")
    rng = np.random.default_rng(n + d)
    x64 = rng.uniform(0.0, 1.0, (n, d))
    pitched_d = min(d, 14)
    big32 = np.ascontiguousarray(rng.uniform(0.0, 1.0, (n, 40)), dtype=np.float32)
    arrays = {"Fortran float64": np.asfortranarray(x64), "Fortran float32": np.asfortranarray(x64.astype(np.float32)),
              "C-pitched float32": big32[:, :pitched_d], "C uint16": np.ascontiguousarray(x64 * 60000.0).astype(np.uint16),
              "C float64": x64, "C float32": np.ascontiguousarray(x64.astype(np.float32))}
    h = _lib.Handle(0)
    out = {}
    for name, x in arrays.items():
        if has_views:
            assert _lib.points_source(x)[0] is x
            call = lambda: h.points_upload(x)
        else:
            call = lambda: h.points_upload(_lib.as_points(x))
        ms = []
        for _ in range(WARM + CALLS):
            t0 = time.perf_counter()
            call()
            h.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = ms[WARM:]
    if has_views:
        out["view_points"] = h.stats()["view_points"]
    h.close()
    print("RESULT " + json.dumps(out))


def csv_child(points, workdir):
    """Scaler fit + first timepoint of app.run over CSVs, as parsed and with the copy to C order put back: seconds."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import pandas as pd
    import scenarios
    from chronoclust_amd import app
    from chronoclust_amd.scaling import scaler as S
    files = []
    for t in range(3):
        x = scenarios.make_blobs(50 + t, points, 20, 200)
        fn = os.path.join(workdir, "tp%d.csv" % t)
        pd.DataFrame(x, columns=["m%d" % i for i in range(20)]).to_csv(fn, index=False)
        files.append(fn)
    keep = S.points_source
    res = {}
    for label, source in (("as parsed", keep), ("copied to C order", lambda a: (np.ascontiguousarray(a, dtype=np.float64), None)),
                          ("as parsed again", keep)):
        S.points_source = source
        out = os.path.join(workdir, "out_" + label.replace(" ", "_"))
        os.makedirs(out)
        parse = []
        real = S.read_timepoint

        def timed(fn):
            t0 = time.perf_counter()
            x = real(fn)
            parse.append(time.perf_counter() - t0)
            return x

        S.read_timepoint = timed
        t0 = time.perf_counter()
        app.run(data=files, output_directory=out, **scenarios.blob_params(points))
        total = time.perf_counter() - t0
        S.read_timepoint = real
        first = app.LAST_RUN_TIMINGS[0]
        res[label] = dict(total_s=total, parse_s=sum(parse), first_read_s=first["read"], first_clustering_s=first["clustering"])
    S.points_source = keep
    print("RESULT " + json.dumps(res))


def summary(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_layouts.txt"))
    ap.add_argument("--csv-points", type=int, default=1000000)
    ap.add_argument("--child", nargs=3, metavar=("TREE", "N", "D"), help=argparse.SUPPRESS)
    ap.add_argument("--csv-child", nargs=2, metavar=("POINTS", "DIR"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]), int(args.child[2]))
        return 0
    if args.csv_child:
        csv_child(int(args.csv_child[0]), args.csv_child[1])
        return 0
    if not args.parent:
        ap.error("--parent is required")
    trees = (("parent", os.path.abspath(args.parent)), ("this", ROOT))
    res = {}

    def run(argv, timeout):
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:  # (nothing more is started on the device after a failure)
            sys.stderr.write(p.stdout + p.stderr)
            return None
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])

    for i, (n, d) in enumerate(SHAPES):
        for label, tree in (trees if i % 2 == 0 else trees[::-1]):  # (the builds alternate, and so does which of them goes first)
            res[(n, d, label)] = run(["--child", tree, str(n), str(d)], 600)
            if res[(n, d, label)] is None:
                return 1
    lines = ["python tools/ingest_layouts.py --parent <parent tree>: numpy array (pageable) -> resident points -> cc_sync, ms; median "
             "of %d calls after %d warm-ups [min .. max].  (a) as_points + upload, parent build; (b) points_upload of the array where "
             "it lies, this build." % (CALLS, WARM), ""]
    ok = True
    for n, d in SHAPES:
        lines.append("%d x %d" % (n, d))
        for name in SOURCES:
            a, b = summary(res[(n, d, "parent")][name]), summary(res[(n, d, "this")][name])
            spread = max(a[2] - a[1], b[2] - b[1])
            holds = a[0] - b[0] > spread
            ok = ok and holds
            for key, fig in (("a", a), ("b", b)):
                lines.append("  %-18s (%s) %9.2f  [%9.2f .. %9.2f]   %7.1f M points/s" % (name, key, fig[0], fig[1], fig[2], n / fig[0] / 1e3))
            lines.append("  %-18s (b) below (a) by %.2f ms, spread %.2f ms: %s;  (a) / (b) = %.1f"
                         % (name, a[0] - b[0], spread, "holds" if holds else "DOES NOT HOLD", a[0] / b[0]))
        for name in OLD:
            a, b = summary(res[(n, d, "parent")][name]), summary(res[(n, d, "this")][name])
            spread = max(a[2] - a[1], b[2] - b[1])
            same = abs(b[0] - a[0]) <= spread
            ok = ok and same
            for key, fig in (("parent", a), ("this", b)):
                lines.append("  %-18s (%-6s) %6.2f  [%9.2f .. %9.2f]   %7.1f M points/s" % (name, key, fig[0], fig[1], fig[2], n / fig[0] / 1e3))
            lines.append("  %-18s this - parent = %+.2f ms, spread %.2f ms: %s" % (name, b[0] - a[0], spread, "holds" if same else "DOES NOT HOLD"))
        lines.append("")
    import tempfile
    with tempfile.TemporaryDirectory() as work:
        csv = run(["--csv-child", str(args.csv_points), work], 900)
    if csv is None:
        return 1
    lines.append("app.run over three CSV timepoints of %d x 20 (this build; seconds): the whole run, of it pandas parsing, and the first "
                 "timepoint's read and clustering steps" % args.csv_points)
    for label, r in csv.items():
        lines.append("  %-18s total %7.2f   parse %7.2f   total - parse %6.2f   first read %.4f   first clustering %.4f"
                     % (label, r["total_s"], r["parse_s"], r["total_s"] - r["parse_s"], r["first_read_s"], r["first_clustering_s"]))
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
