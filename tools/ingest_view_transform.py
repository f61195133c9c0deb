#!/usr/bin/env python3
"""What compensation, arcsinh and the logicle scale cost where a CSV's or an array's points land, and what they cost on the host.

    python tools/ingest_view_transform.py [--out profiles/ingest_view_transform.txt]

1 M x 20 points in pageable memory as a Fortran-order float64 array (what pd.read_csv(...).to_numpy() hands over), as a
C-contiguous float32 array and as uint16 columns (Fortran order), each with a 9-channel spillover matrix over the first nine
columns and cofactor 5 on every column, and the logicle variant: the same compensation and the logicle scale (T = 262144,
W = 0.5, M = 4.5, A = 0) on every column.  One operation, from the array to the moment cc_sync returns: the upload to resident
points, on four routes timed beside each other in one process
  (x) points_upload(TransformedPoints(array, transform)): the `_view_xl` route - k_ingest_xf for the columns forms,
      k_ingest_list_xf over rows for the C-contiguous one;
  (v) the plain `_view` upload of the same array (TransformedPoints without a transform IS that sibling): the floor,
      (x) - (v) is what the transform costs;
  (l) the `_list_xf` / `_list_xl` upload of the same values and element type laid out as event records of 20 channels, with the
      same transform: the route the transform was first built on;
  (b) the host route (x) replaces: np.asarray(TransformedPoints) - the compensation in numpy, np.arcsinh or logicle_host -
      then the float64 upload.
Per figure the median with minimum and maximum beside it: (x), (v) and (l) 7 calls after 2 warm-ups, alternating call by
call; (b) 2 calls after 1 warm-up.  Per case the verdicts: (x) below (b) by more than the spread (max - min) of either, and
whether (x) exceeds (l) by more than the spread of either - and where it does, how much of the gap the plain upload (v) of the
same array already has: what bounds it."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, M, COFACTOR = 1000000, 20, 9, 5.0
LOGICLE = (262144.0, 0.5, 4.5, 0.0)
WARM, CALLS = 2, 7
HOST_WARM, HOST_CALLS = 1, 2
CASES = (("float64, Fortran order (a parsed CSV)", "f8", "F"), ("float32, C-contiguous", "f4", "C"), ("uint16 columns (Fortran order)", "u2", "F"))


def inverse_spillover(np, m):
    rng = np.random.default_rng(m)
    s = np.eye(m) + rng.uniform(0.0, 0.15, (m, m)) * (1.0 - np.eye(m))
    return np.ascontiguousarray(np.linalg.inv(s))


def summary(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def bound_note(x, v, l):
    """What bounds (x) where it exceeds (l): how much of the gap the plain upload of the same array - no transform - already has."""
    return ("  what bounds it: of these %.2f ms, (v) - (l) = %+.2f ms is there without any transform - the plain upload of the same "
            "array against the list route WITH one: a slab of the columns form is staged as d strip copies, event records as one "
            "copy -; the rest is the transform's own share, (x) - (v) = %.2f ms (the logicle instances of k_ingest_xf spill 26 to 35 "
            "scalar registers to vector lanes, profiles/view_transform_device_code.txt; not separated further here)"
            % (x[0] - l[0], v[0] - l[0], x[0] - v[0]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_view_transform.txt"))
    ap.add_argument("--points", type=int, default=N, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from chronoclust_amd import _lib
    n = args.points
    rng = np.random.default_rng(n + D)
    inv = inverse_spillover(np, M)
    variants = (("spillover of %d channels, cofactor %g" % (M, COFACTOR), _lib.ListTransform(np.arange(M), inv, COFACTOR)),
                ("spillover of %d channels, logicle %r" % (M, LOGICLE), _lib.ListTransform(np.arange(M), inv, None, LOGICLE)))
    lines = ["python tools/ingest_view_transform.py: %d x %d points (pageable) -> resident points -> cc_sync, ms; median [min .. max].  "
             "(x) points_upload(TransformedPoints(array, transform)), the `_view_xl` route; (v) the plain `_view` upload of the same "
             "array; (l) the `_list_xf` / `_list_xl` upload of the same values and type as event records with the same transform; "
             "(x), (v), (l) %d calls after %d warm-ups, alternating.  (b) np.asarray(TransformedPoints) - compensation and arcsinh / "
             "logicle in numpy - + the float64 upload: %d calls after %d warm-up." % (n, D, CALLS, WARM, HOST_CALLS, HOST_WARM), ""]
    ok = True
    h = _lib.Handle(0)
    for name, code, order in CASES:
        dt = np.dtype(code)
        if dt.kind == "f":
            vals = (rng.uniform(-0.02, 1.0, (n, D)) ** 3 * 20000.0).astype(dt)
        else:
            vals = rng.integers(0, 60000, (n, D)).astype(dt)
        a = np.asfortranarray(vals) if order == "F" else np.ascontiguousarray(vals)
        blob = np.ascontiguousarray(vals).tobytes()
        del vals
        plain = _lib.TransformedPoints(a, None)
        for what, tr in variants:
            tp = _lib.TransformedPoints(a, tr)
            lm = _lib.ListMode(blob, n, D, dt, transform=tr)
            routes = {"x": lambda: h.points_upload(tp), "v": lambda: h.points_upload(plain), "l": lambda: h.points_upload(lm),
                      "b": lambda: h.points_upload(np.asarray(tp))}
            ms = {k: [] for k in routes}
            for _ in range(WARM + CALLS):
                for key in ("x", "v", "l"):
                    t0 = time.perf_counter()
                    routes[key]()
                    h.sync()
                    ms[key].append((time.perf_counter() - t0) * 1e3)
            for _ in range(HOST_WARM + HOST_CALLS):
                t0 = time.perf_counter()
                routes["b"]()
                h.sync()
                ms["b"].append((time.perf_counter() - t0) * 1e3)
            x, v, l, b = (summary(ms[k][(HOST_WARM if k == "b" else WARM):]) for k in ("x", "v", "l", "b"))
            lines.append("%s; %s" % (name, what))
            for key, fig in (("x", x), ("v", v), ("l", l), ("b", b)):
                lines.append("  (%s) %9.2f  [%9.2f .. %9.2f]   %7.1f M points/s" % (key, fig[0], fig[1], fig[2], n / fig[0] / 1e3))
            spread_b = max(x[2] - x[1], b[2] - b[1])
            spread_l = max(x[2] - x[1], l[2] - l[1])
            holds = b[0] - x[0] > spread_b
            ok = ok and holds
            lines.append("  the transform costs (x) - (v) = %.2f ms, (x) / (v) = %.2f;  (x) below (b) by %.2f ms, spread %.2f ms: %s, "
                         "(b) / (x) = %.1f;  (x) - (l) = %+.2f ms, spread %.2f ms: (x) %s (l) by more than the spread"
                         % (x[0] - v[0], x[0] / v[0], b[0] - x[0], spread_b, "holds" if holds else "DOES NOT HOLD", b[0] / x[0],
                            x[0] - l[0], spread_l, "exceeds" if x[0] - l[0] > spread_l else "does not exceed"))
            if x[0] - l[0] > spread_l:
                lines.append(bound_note(x, v, l))
            lines.append("")
    h.close()
    lines.append("all verdicts against the host route hold" if ok else "a verdict against the host route does not hold")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
