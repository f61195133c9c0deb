#!/usr/bin/env python3
"""What a user whose timepoints are list-mode FCS data pays to get them onto the device, with and without the `_list` entry
points.

    python tools/ingest_fcs.py [--out profiles/ingest_fcs.txt] [--app-points 1000000]

Shapes 1 M x 20 of 30 channels, 5 M x 14 of 20 and 2 M x 40 of 50 (unclustered channels interleaved with the clustered ones),
as big-endian float32 and as big-endian uint16 event records in pageable memory.  One operation, from the record buffer to the
moment cc_sync returns: the upload to resident points, on two routes
  (a) np.asarray(list_mode) - the byte swap, the gather of the channels and the widening on the host - then the float32 /
      float64 upload that has always existed;
  (b) points_upload(list_mode): the records cross the bus as they are and k_ingest_list decodes them.
Per figure: the median of 7 calls after 2 warm-ups, minimum and maximum beside it; (a) and (b) alternate call by call in ONE
process (one per shape).  Then app.run over three timepoints of --app-points x 20 of 30 channels as big-endian float64 FCS
files against CSV files of the same values: what the text parse costs.
The verdict at the end: (b) below (a) at every shape by more than the spread (max - min) of either."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1000000, 20, 30), (5000000, 14, 20), (2000000, 40, 50)]
SOURCES = (("big-endian float32", ">f4"), ("big-endian uint16", ">u2"))
WARM, CALLS = 2, 7


def selected(d, src_cols):
    """d of src_cols channels in file order: all but the first src_cols - d of the channels 0, 3, 6, ..."""
    skipped = set(range(0, 3 * (src_cols - d), 3))
    cols = [c for c in range(src_cols) if c not in skipped]
    assert len(cols) == d
    return cols


def child(n, d, src_cols):
    """One process per shape: prints one JSON object, source -> {"a": [ms per call], "b": [...]}."""
    sys.path.insert(0, ROOT)
    import numpy as np
    from chronoclust_amd import _lib
    rng = np.random.default_rng(n + d)
    cols = selected(d, src_cols)
    h = _lib.Handle(0)
    out = {}
    for name, code in SOURCES:
        dt = np.dtype(code)
        if dt.kind == "f":
            rec = rng.uniform(0.0, 1.0, (n, src_cols)).astype(dt)
        else:
            rec = rng.integers(0, 60000, (n, src_cols)).astype(dt)
        lm = _lib.ListMode(rec.tobytes(), n, src_cols, dt, columns=cols)
        del rec
        routes = {"a": lambda: h.points_upload(np.asarray(lm)), "b": lambda: h.points_upload(lm)}
        ms = {"a": [], "b": []}
        for _ in range(WARM + CALLS):
            for key in ("a", "b"):
                t0 = time.perf_counter()
                routes[key]()
                h.sync()
                ms[key].append((time.perf_counter() - t0) * 1e3)
        out[name] = {key: v[WARM:] for key, v in ms.items()}
    out["list_points"] = h.stats()["list_points"]
    h.close()
    print("RESULT " + json.dumps(out))


def write_fcs(path, rec, names):
    """A minimal FCS 3.1 file around big-endian float64 records."""
    par = rec.shape[1]
    kw = [("$MODE", "L"), ("$DATATYPE", "D"), ("$PAR", str(par)), ("$BYTEORD", "4,3,2,1"), ("$TOT", str(len(rec))), ("$NEXTDATA", "0")]
    for i, name in enumerate(names):
        kw += [("$P%dB" % (i + 1), "64"), ("$P%dR" % (i + 1), "262144"), ("$P%dN" % (i + 1), name), ("$P%dE" % (i + 1), "0,0")]
    data = rec.astype(">f8").tobytes()
    text = ("/" + "".join("%s/%s/" % kv for kv in kw)).encode()
    lo = 58 + len(text)
    hi = lo + len(data) - 1
    fits = hi <= 99999999
    if not fits:  # (the header's fields are eight digits: the offsets go into TEXT, at a fixed width)
        for _ in range(2):
            text = ("/$BEGINDATA/%020d/$ENDDATA/%020d/" % (lo, hi) + "".join("%s/%s/" % kv for kv in kw)).encode()
            lo = 58 + len(text)
            hi = lo + len(data) - 1
    head = b"FCS3.1    " + b"".join(b"%8d" % v for v in (58, 58 + len(text) - 1, lo if fits else 0, hi if fits else 0, 0, 0))
    with open(path, "wb") as f:
        f.write(head + text + data)


def app_child(points, workdir):
    """app.run over FCS and over CSV timepoints of the same values: seconds."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import pandas as pd
    import scenarios
    from chronoclust_amd import app
    cols = selected(20, 30)
    markers = ["m%d" % i for i in range(20)]
    names = ["x%d" % c for c in range(30)]
    for i, c in enumerate(cols):
        names[c] = markers[i]
    files = {"fcs": [], "csv": []}
    for t in range(3):
        x = scenarios.make_blobs(50 + t, points, 20, 200)
        fn = os.path.join(workdir, "tp%d.csv" % t)
        pd.DataFrame(x, columns=markers).to_csv(fn, index=False)
        x = pd.read_csv(fn).to_numpy()  # (the values the CSV holds)
        rec = np.full((points, 30), np.nan)
        rec[:, cols] = x
        write_fcs(fn[:-4] + ".fcs", rec, names)
        with open(fn[:-4] + ".fcs.columns", "w") as f:
            f.write("\n".join(markers) + "\n")
        files["csv"].append(fn)
        files["fcs"].append(fn[:-4] + ".fcs")
    res = {}
    for label in ("fcs", "csv", "fcs again"):
        out = os.path.join(workdir, "out_" + label.replace(" ", "_"))
        os.makedirs(out)
        t0 = time.perf_counter()
        app.run(data=files[label.split()[0]], output_directory=out, **scenarios.blob_params(points))
        total = time.perf_counter() - t0
        tm = app.LAST_RUN_TIMINGS
        res[label] = dict(total_s=total, read_s=sum(t["read"] for t in tm), clustering_s=sum(t["clustering"] for t in tm),
                          point_details_s=sum(t["point_details"] for t in tm))
    same = all(open(os.path.join(workdir, "out_fcs", fn), "rb").read() == open(os.path.join(workdir, "out_csv", fn), "rb").read()
               for fn in ["result.csv"] + ["cluster_points_D%d.csv" % t for t in range(3)])
    res["same_files"] = same
    print("RESULT " + json.dumps(res))


def summary(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_fcs.txt"))
    ap.add_argument("--app-points", type=int, default=1000000)
    ap.add_argument("--child", nargs=3, metavar=("N", "D", "SRC_COLS"), help=argparse.SUPPRESS)
    ap.add_argument("--app-child", nargs=2, metavar=("POINTS", "DIR"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(*[int(v) for v in args.child])
        return 0
    if args.app_child:
        app_child(int(args.app_child[0]), args.app_child[1])
        return 0

    def run(argv, timeout):
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:  # (nothing more is started on the device after a failure)
            sys.stderr.write(p.stdout + p.stderr)
            return None
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])

    lines = ["python tools/ingest_fcs.py: list-mode event records (pageable) -> resident points -> cc_sync, ms; median of %d calls "
             "after %d warm-ups [min .. max], (a) and (b) alternating in one process per shape.  (a) np.asarray(list_mode) + the "
             "upload of old; (b) points_upload(list_mode)." % (CALLS, WARM), ""]
    ok = True
    for n, d, src_cols in SHAPES:
        res = run(["--child", str(n), str(d), str(src_cols)], 600)
        if res is None:
            return 1
        lines.append("%d x %d of %d channels" % (n, d, src_cols))
        for name, _ in SOURCES:
            a, b = summary(res[name]["a"]), summary(res[name]["b"])
            spread = max(a[2] - a[1], b[2] - b[1])
            holds = a[0] - b[0] > spread
            ok = ok and holds
            for key, fig in (("a", a), ("b", b)):
                lines.append("  %-18s (%s) %9.2f  [%9.2f .. %9.2f]   %7.1f M points/s" % (name, key, fig[0], fig[1], fig[2], n / fig[0] / 1e3))
            lines.append("  %-18s (b) below (a) by %.2f ms, spread %.2f ms: %s;  (a) / (b) = %.1f"
                         % (name, a[0] - b[0], spread, "holds" if holds else "DOES NOT HOLD", a[0] / b[0]))
        lines.append("")
    import tempfile
    with tempfile.TemporaryDirectory() as work:
        res = run(["--app-child", str(args.app_points), work], 1100)
    if res is None:
        return 1
    lines.append("app.run over three timepoints of %d x 20 of 30 channels (seconds): the whole run, of it reading the files (the scaler's "
                 "fit reads them first: 'read' is what the run's loop still spends), the clustering step (upload included) and the "
                 "per-point file" % args.app_points)
    for label in ("fcs", "csv", "fcs again"):
        r = res[label]
        lines.append("  %-10s total %7.2f   read %7.3f   clustering %7.3f   point details %7.2f"
                     % (label, r["total_s"], r["read_s"], r["clustering_s"], r["point_details_s"]))
    lines.append("  the FCS run's files %s the CSV run's, byte for byte" % ("are" if res["same_files"] else "ARE NOT"))
    lines.append("")
    lines.append("all verdicts hold" if ok and res["same_files"] else "a verdict does not hold")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
