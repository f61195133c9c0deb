#!/usr/bin/env python3
"""What compensation and arcsinh cost where the events land, and what they cost on the host.

    python tools/ingest_transform.py [--out profiles/ingest_transform.txt]

The shapes of tools/ingest_fcs.py - 1 M x 20 of 30 channels, 5 M x 14 of 20 and 2 M x 40 of 50, as big-endian float32 and as
big-endian uint16 event records in pageable memory - with a 9-channel spillover matrix over the first nine selected channels
and cofactor 5 on every selected channel.  One operation, from the record buffer to the moment cc_sync returns: the upload to
resident points, on three routes
  (x) points_upload(list_mode with the transform): k_ingest_list_xf compensates and transforms as it decodes;
  (a) points_upload(the same records without a transform): k_ingest_list, which this change leaves as it was - the floor;
      (x) - (a) is what the transform costs;
  (b) the route (x) replaces: np.asarray(list_mode with the transform) - the decode, the compensation in numpy and np.arcsinh
      on the host - then the float64 upload.
Per figure the median with minimum and maximum beside it: (x) and (a) 7 calls after 2 warm-ups, alternating call by call; (b),
seconds per call, 3 calls after 1 warm-up, in the same process (one per shape).
Then the distance of the device's asinh from an extended-precision reference, in units in the last place, over |q| from 1e-9
to 1e6, both signs and 0 (the sweep of tests/test_fcs_transform.py).
The verdict at the end: (x) below (b) at every shape by more than the spread (max - min) of either."""
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
HOST_WARM, HOST_CALLS = 1, 3
M, COFACTOR = 9, 5.0


def selected(d, src_cols):
    """d of src_cols channels in file order: all but the first src_cols - d of the channels 0, 3, 6, ..."""
    skipped = set(range(0, 3 * (src_cols - d), 3))
    cols = [c for c in range(src_cols) if c not in skipped]
    assert len(cols) == d
    return cols


def inverse_spillover(np, m):
    rng = np.random.default_rng(m)
    s = np.eye(m) + rng.uniform(0.0, 0.15, (m, m)) * (1.0 - np.eye(m))
    return np.ascontiguousarray(np.linalg.inv(s))


def child(n, d, src_cols):
    """One process per shape: prints one JSON object, source -> {"x": [ms per call], "a": [...], "b": [...]}."""
    sys.path.insert(0, ROOT)
    import numpy as np
    from chronoclust_amd import _lib
    rng = np.random.default_rng(n + d)
    cols = selected(d, src_cols)
    tr = _lib.ListTransform(cols[:M], inverse_spillover(np, M), COFACTOR)
    h = _lib.Handle(0)
    out = {}
    for name, code in SOURCES:
        dt = np.dtype(code)
        if dt.kind == "f":
            rec = (rng.uniform(0.0, 1.0, (n, src_cols)) ** 3 * 20000.0).astype(dt)
        else:
            rec = rng.integers(0, 60000, (n, src_cols)).astype(dt)
        blob = rec.tobytes()
        del rec
        lm_x = _lib.ListMode(blob, n, src_cols, dt, columns=cols, transform=tr)
        lm_a = _lib.ListMode(blob, n, src_cols, dt, columns=cols)
        routes = {"x": lambda: h.points_upload(lm_x), "a": lambda: h.points_upload(lm_a),
                  "b": lambda: h.points_upload(np.asarray(lm_x))}
        ms = {"x": [], "a": [], "b": []}
        for _ in range(WARM + CALLS):
            for key in ("x", "a"):
                t0 = time.perf_counter()
                routes[key]()
                h.sync()
                ms[key].append((time.perf_counter() - t0) * 1e3)
        for _ in range(HOST_WARM + HOST_CALLS):
            t0 = time.perf_counter()
            routes["b"]()
            h.sync()
            ms["b"].append((time.perf_counter() - t0) * 1e3)
        out[name] = {"x": ms["x"][WARM:], "a": ms["a"][WARM:], "b": ms["b"][HOST_WARM:]}
    h.close()
    print("RESULT " + json.dumps(out))


def asinh_child():
    """The sweep: largest distance of the device's asinh from the reference, per band of |q|."""
    sys.path.insert(0, ROOT)
    import numpy as np
    from chronoclust_amd import _lib
    rng = np.random.default_rng(3)
    q = np.concatenate([10.0 ** rng.uniform(lo, lo + 3, 40000) for lo in (-9, -6, -3, 0, 3)])
    q = np.concatenate([q, -q, [0.0, -0.0, 1e-9, -1e-9, 1e6, -1e6, 1.0, -1.0]])
    v = np.ascontiguousarray((q * COFACTOR).reshape(-1, 4))
    h = _lib.Handle(0)
    h.points_upload(_lib.ListMode(v.tobytes(), v.shape[0], 4, np.dtype("<f8"), transform=_lib.ListTransform(cofactor=COFACTOR)))
    got = h.points_download(4)
    h.close()
    q = v / COFACTOR
    extended = np.finfo(np.longdouble).nmant >= 63
    ref = np.arcsinh(q.astype(np.longdouble)).astype(np.float64) if extended else np.arcsinh(q)

    def ordered(x):
        i = np.ascontiguousarray(x).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)

    dist = np.abs(ordered(got) - ordered(ref))
    own = np.abs(ordered(np.arcsinh(q)) - ordered(ref))
    bands = []
    for lo in (-9, -6, -3, 0, 3):
        band = (np.abs(q) >= 10.0 ** lo) & (np.abs(q) < 10.0 ** (lo + 3))
        bands.append([lo, int(band.sum()), int(dist[band].max()), float((dist[band] > 0).mean()), int(own[band].max()),
                      float((own[band] > 0).mean())])
    print("RESULT " + json.dumps(dict(values=int(dist.size), max_ulp=int(dist.max()), extended=bool(extended), bands=bands,
                                      zeros=bool((got[q == 0] == 0).all()))))


def summary(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_transform.txt"))
    ap.add_argument("--child", nargs=3, metavar=("N", "D", "SRC_COLS"), help=argparse.SUPPRESS)
    ap.add_argument("--asinh-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(*[int(v) for v in args.child])
        return 0
    if args.asinh_child:
        asinh_child()
        return 0

    def run(argv, timeout):
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:  # (nothing more is started on the device after a failure)
            sys.stderr.write(p.stdout + p.stderr)
            return None
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])

    lines = ["python tools/ingest_transform.py: list-mode event records (pageable) -> resident points -> cc_sync, ms; median [min .. "
             "max].  A %d-channel spillover over the first %d selected channels, cofactor %g on every selected channel.  (x) "
             "points_upload(list_mode with the transform); (a) the same records without a transform (k_ingest_list, untouched by "
             "the transform: the floor); (x) and (a) %d calls after %d warm-ups, alternating.  (b) np.asarray(list_mode with the "
             "transform) - decode, compensation and arcsinh in numpy - + the float64 upload: %d calls after %d warm-up."
             % (M, M, COFACTOR, CALLS, WARM, HOST_CALLS, HOST_WARM), ""]
    ok = True
    for n, d, src_cols in SHAPES:
        res = run(["--child", str(n), str(d), str(src_cols)], 900)
        if res is None:
            return 1
        lines.append("%d x %d of %d channels" % (n, d, src_cols))
        for name, _ in SOURCES:
            x, a, b = (summary(res[name][k]) for k in ("x", "a", "b"))
            spread = max(x[2] - x[1], b[2] - b[1])
            holds = b[0] - x[0] > spread
            ok = ok and holds
            for key, fig in (("x", x), ("a", a), ("b", b)):
                lines.append("  %-18s (%s) %9.2f  [%9.2f .. %9.2f]   %7.1f M points/s" % (name, key, fig[0], fig[1], fig[2], n / fig[0] / 1e3))
            lines.append("  %-18s the transform costs (x) - (a) = %.2f ms, (x) / (a) = %.2f;  (x) below (b) by %.2f ms, spread %.2f ms: "
                         "%s;  (b) / (x) = %.1f" % (name, x[0] - a[0], x[0] / a[0], b[0] - x[0], spread,
                                                    "holds" if holds else "DOES NOT HOLD", b[0] / x[0]))
        lines.append("")
    res = run(["--asinh-child"], 300)
    if res is None:
        return 1
    lines.append("asinh on the device against %s, units in the last place, %d values, |q| from 1e-9 to 1e6, both signs, and 0"
                 % ("np.arcsinh in extended precision rounded to double" if res["extended"] else "np.arcsinh in double", res["values"]))
    for lo, count, worst, share, own_worst, own_share in res["bands"]:
        lines.append("  |q| in [1e%+d, 1e%+d)  %6d values   device: largest %d ulp, %.2f %% off by one or more   numpy's own float64 arcsinh: "
                     "largest %d ulp, %.2f %%" % (lo, lo + 3, count, worst, 100 * share, own_worst, 100 * own_share))
    lines.append("  largest distance: %d ulp; asinh(+-0) == 0: %s" % (res["max_ulp"], "yes" if res["zeros"] else "NO"))
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
