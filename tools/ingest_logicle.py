#!/usr/bin/env python3
"""What the logicle scale costs where the events land, what it costs on the host, and how far the device's solve lies from the
true root.

    python tools/ingest_logicle.py [--out profiles/ingest_logicle.txt]

The accuracy sweep of tests/test_fcs_logicle.py first: per parameter set of tests/logicle_util.py one upload of float64 records,
|v| log-uniform per three decades from 1e-6 to 2 T, 20 000 values per band, both signs, +-0, +-T, the smallest subnormal and
1e300; the distance of what the device holds from the referee (the root in extended precision, derived from T, W, M, A alone,
rounded once) in units of np.spacing(max(|y_ref|, 0.5)), per band of |v|, and the host fallback's beside it.
Then the shapes of tools/ingest_transform.py - 1 M x 20 of 30 channels, 5 M x 14 of 20 and 2 M x 40 of 50, as big-endian float32
and as big-endian uint16 event records in pageable memory - with a 9-channel spillover matrix over the first nine selected
channels.  One operation, from the record buffer to the moment cc_sync returns: the upload to resident points, on three routes
  (x) points_upload(list_mode with compensation and the logicle scale (T 262144, W 0.5, M 4.5, A 0) on every selected channel):
      the logicle instance of k_ingest_list_xf;
  (a) the same records with cofactor 5 on every channel instead: the kernel as it was, the floor measured beside it;
      (x) - (a) is what the solve costs over asinh;
  (b) the host route (x) replaces: np.asarray(list_mode of (x)) - decode, compensation and the logicle solve in numpy - then the
      float64 upload.
(x), (a) and (b) alternate call by call in one process (one per shape) on one machine; per figure the median with minimum and
maximum beside it, 7 calls after 2 warm-ups.  No rate is promised: the figures are what was measured."""
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
M, COFACTOR = 9, 5.0
LOGICLE = (262144.0, 0.5, 4.5, 0.0)


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
    inv = inverse_spillover(np, M)
    tr_x = _lib.ListTransform(cols[:M], inv, None, LOGICLE)
    tr_a = _lib.ListTransform(cols[:M], inv, COFACTOR)
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
        lm_x = _lib.ListMode(blob, n, src_cols, dt, columns=cols, transform=tr_x)
        lm_a = _lib.ListMode(blob, n, src_cols, dt, columns=cols, transform=tr_a)
        routes = {"x": lambda: h.points_upload(lm_x), "a": lambda: h.points_upload(lm_a),
                  "b": lambda: h.points_upload(np.asarray(lm_x))}
        ms = {"x": [], "a": [], "b": []}
        for call in range(WARM + CALLS):
            for key in ("x", "a", "b"):
                t0 = time.perf_counter()
                routes[key]()
                h.sync()
                ms[key].append((time.perf_counter() - t0) * 1e3)
            print("PROGRESS %d x %d of %d, %s: call %d of %d" % (n, d, src_cols, name, call + 1, WARM + CALLS), flush=True)
        out[name] = {key: ms[key][WARM:] for key in ms}
    h.close()
    print("RESULT " + json.dumps(out), flush=True)


def sweep_child():
    """The accuracy sweep: per parameter set and band of |v| the largest distance from the referee, device and host."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import logicle_util as L
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    sets = []
    for p in L.P:
        v = L.sweep(p[0]).reshape(-1, 4)
        lm = _lib.ListMode(v.tobytes(), v.shape[0], 4, np.dtype("<f8"), transform=_lib.ListTransform(logicle=p))
        h.points_upload(lm)
        got = h.points_download(4)
        ref = L.logicle(v, *p)
        dev, host = L.units(got, ref), L.units(np.asarray(lm), ref)
        bands = []
        for lo, hi in L.sweep_bands(p[0]):
            band = (np.abs(v) >= lo) & (np.abs(v) <= hi)
            bands.append([lo, hi, int(band.sum()), float(dev[band].max()), float((dev[band] >= 1).mean()), float(host[band].max()),
                          float((host[band] >= 1).mean())])
        special = [[what, float(dev[sel].max()), float(host[sel].max())]
                   for what, sel in (("+-0", v == 0), ("+-T", np.abs(v) == p[0]), ("5e-324", v == 5e-324), ("1e300", v == 1e300))]
        x1 = _lib.logicle_coefficients(p)[0]
        sets.append(dict(p=list(p), values=int(dev.size), dev_max=float(dev.max()), host_max=float(host.max()), bands=bands,
                         special=special, finite=bool(np.isfinite(got).all()),
                         zeros=bool((got[v == 0].view(np.int64) == np.float64(x1).view(np.int64)).all())))
        print("PROGRESS sweep %r" % (p,), flush=True)
    h.close()
    print("RESULT " + json.dumps(dict(extended=bool(L.EXTENDED), sets=sets)), flush=True)


def summary(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_logicle.txt"))
    ap.add_argument("--child", nargs=3, metavar=("N", "D", "SRC_COLS"), help=argparse.SUPPRESS)
    ap.add_argument("--sweep-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(*[int(v) for v in args.child])
        return 0
    if args.sweep_child:
        sweep_child()
        return 0

    def run(argv, timeout):
        """The child's RESULT, its progress lines passed on as they come; None after a failure (nothing more is started on the
        device then)."""
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True)
        result, deadline = None, time.time() + timeout
        for line in p.stdout:
            if line.startswith("RESULT "):
                result = json.loads(line[7:])
            else:
                sys.stdout.write(line)
                sys.stdout.flush()
            if time.time() > deadline:
                p.kill()
                return None
        return result if p.wait() == 0 else None

    lines = ["python tools/ingest_logicle.py"]
    res = run(["--sweep-child"], 600)
    if res is None:
        return 1
    lines += ["", "the logicle solve against %s, in units of np.spacing(max(|y_ref|, 0.5)); device: what points_download returns "
              "after the upload, host: np.asarray(list_mode)"
              % ("the referee (extended precision, rounded once)" if res["extended"] else "A REFEREE NO WIDER THAN float64")]
    for s in res["sets"]:
        lines.append("  (T, W, M, A) = (%g, %g, %g, %g), %d values: device largest %.3f, host largest %.3f; every result finite: %s; "
                     "logicle(+-0) has the bits of x1: %s" % (tuple(s["p"]) + (s["values"], s["dev_max"], s["host_max"],
                                                                               "yes" if s["finite"] else "NO",
                                                                               "yes" if s["zeros"] else "NO")))
        for lo, hi, count, dmax, dshare, hmax, hshare in s["bands"]:
            lines.append("    |v| in [%g, %g]  %6d values   device: largest %.3f, %5.2f %% at one unit or more   host: largest %.3f, "
                         "%5.2f %%" % (lo, hi, count, dmax, 100 * dshare, hmax, 100 * hshare))
        lines.append("    " + ";  ".join("%s: device %.3f, host %.3f" % tuple(x) for x in s["special"]))
    lines.append("  largest distance over every set: device %.3f, host %.3f"
                 % (max(s["dev_max"] for s in res["sets"]), max(s["host_max"] for s in res["sets"])))
    lines += ["", "list-mode event records (pageable) -> resident points -> cc_sync, ms; median [min .. max] of %d calls after %d "
              "warm-ups, (x), (a) and (b) alternating call by call.  A %d-channel spillover over the first %d selected channels.  (x) "
              "compensation + logicle %r on every selected channel; (a) the same records, compensation + cofactor %g (the kernel as "
              "it was: the floor); (b) np.asarray(list_mode of (x)) + the float64 upload." % (CALLS, WARM, M, M, LOGICLE, COFACTOR), ""]
    for n, d, src_cols in SHAPES:
        res = run(["--child", str(n), str(d), str(src_cols)], 1100)
        if res is None:
            return 1
        lines.append("%d x %d of %d channels" % (n, d, src_cols))
        for name, _ in SOURCES:
            x, a, b = (summary(res[name][k]) for k in ("x", "a", "b"))
            for key, fig in (("x", x), ("a", a), ("b", b)):
                lines.append("  %-18s (%s) %9.2f  [%9.2f .. %9.2f]   %7.1f M points/s" % (name, key, fig[0], fig[1], fig[2], n / fig[0] / 1e3))
            lines.append("  %-18s the solve costs (x) - (a) = %.2f ms over asinh, (x) / (a) = %.2f;  (b) / (x) = %.1f"
                         % (name, x[0] - a[0], x[0] / a[0], b[0] / x[0]))
        lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
