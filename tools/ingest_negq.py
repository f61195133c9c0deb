#!/usr/bin/env python3
"""What the estimate of the logicle width costs where the events land, and what it costs on the host.

    python tools/ingest_negq.py [--out profiles/ingest_negq.txt]

The shapes of tools/ingest_logicle.py - 1 M x 20 of 30 channels, 5 M x 14 of 20 and 2 M x 40 of 50, as big-endian float32 and as
big-endian uint16 event records in pageable memory - with a 9-channel spillover matrix over the first nine selected channels.
One operation, from the record buffer to the answer on the host, on three routes
  (x) Handle.negative_quantiles of the one source at q = 0.05, every selected channel wanted: cc_negq_begin (the scratch is
      allocated), cc_negq_add_list (the copy, k_negq_stage), cc_negq_select (eight digit passes, the successor), cc_negq_end;
  (a) Handle.col_minmax of the same source: the same copy and the same value function - the floor;
  (b) the host route (x) replaces: np.asarray(list_mode) - decode and compensation in numpy - and np.quantile of the negative
      values per channel.
(x), (a) and (b) alternate call by call in one process (one per shape) on one machine; per figure the median with minimum and
maximum beside it, 7 calls after 2 warm-ups.  (x) and (b) are checked to agree bit for bit on the first call.  No rate is
promised: the figures are what was measured."""
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
M, Q = 9, 0.05


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
    """One process per shape: prints one JSON object, source -> {"x": [ms per call], "a": [...], "b": [...], "negative": share}."""
    sys.path.insert(0, ROOT)
    import numpy as np
    from chronoclust_amd import _lib
    rng = np.random.default_rng(n + d)
    cols = selected(d, src_cols)
    tr = _lib.ListTransform(cols[:M], inverse_spillover(np, M))
    h = _lib.Handle(0)
    out = {}
    for name, code in SOURCES:
        dt = np.dtype(code)
        if dt.kind == "f":
            rec = (rng.uniform(0.0, 1.0, (n, src_cols)) ** 3 * 20000.0 - 50.0).astype(dt)  # (dim channels dip below zero)
        else:
            rec = rng.integers(0, 60000, (n, src_cols)).astype(dt)  # (negative through the compensation alone)
        blob = rec.tobytes()
        del rec
        lm = _lib.ListMode(blob, n, src_cols, dt, columns=cols, transform=tr)
        got = {}

        def host():
            v = np.asarray(lm)
            got["b"] = [np.quantile(v[:, c][v[:, c] < 0], Q) if (v[:, c] < 0).any() else np.nan for c in range(d)]
            got["share"] = float((v < 0).mean())

        def device():
            got["x"] = h.negative_quantiles([lm], Q)

        routes = {"x": device, "a": lambda: h.col_minmax(lm), "b": host}
        ms = {"x": [], "a": [], "b": []}
        for call in range(WARM + CALLS):
            for key in ("x", "a", "b"):
                t0 = time.perf_counter()
                routes[key]()
                h.sync()
                ms[key].append((time.perf_counter() - t0) * 1e3)
            if call == 0:
                count, lo, hi, frac = got["x"]
                mine = np.array([np.quantile(np.array([lo[c], hi[c]]), frac[c]) if count[c] else np.nan for c in range(d)])
                assert np.array_equal(mine.view(np.int64), np.array(got["b"]).view(np.int64)), "device and host disagree"
            print("PROGRESS %d x %d of %d, %s: call %d of %d" % (n, d, src_cols, name, call + 1, WARM + CALLS), flush=True)
        out[name] = {key: ms[key][WARM:] for key in ms}
        out[name]["negative"] = got["share"]
    h.close()
    print("RESULT " + json.dumps(out), flush=True)


def summary(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_negq.txt"))
    ap.add_argument("--child", nargs=3, metavar=("N", "D", "SRC_COLS"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(*[int(v) for v in args.child])
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

    lines = ["python tools/ingest_negq.py", "",
             "list-mode event records (pageable) -> the answer on the host, ms; median [min .. max] of %d calls after %d warm-ups, (x), "
             "(a) and (b) alternating call by call.  A %d-channel spillover over the first %d selected channels.  (x) "
             "Handle.negative_quantiles at q = %g, every selected channel wanted (begin, add, select, end); (a) Handle.col_minmax of "
             "the same source: the floor; (b) np.asarray(list_mode) + np.quantile of the negative values per channel.  (x) and (b) "
             "agreed bit for bit on the first call of every row." % (CALLS, WARM, M, M, Q), ""]
    for n, d, src_cols in SHAPES:
        res = run(["--child", str(n), str(d), str(src_cols)], 500)
        if res is None:
            return 1
        lines.append("%d x %d of %d channels" % (n, d, src_cols))
        for name, _ in SOURCES:
            x, a, b = (summary(res[name][k]) for k in ("x", "a", "b"))
            for key, fig in (("x", x), ("a", a), ("b", b)):
                lines.append("  %-18s (%s) %9.2f  [%9.2f .. %9.2f]   %7.1f M events/s" % (name, key, fig[0], fig[1], fig[2], n / fig[0] / 1e3))
            lines.append("  %-18s %.1f %% of the values negative;  (x) - (a) = %.2f ms, (x) / (a) = %.2f;  (b) / (x) = %.1f;  (x) below (b) "
                         "by more than the spread: %s" % (name, 100 * res[name]["negative"], x[0] - a[0], x[0] / a[0], b[0] / x[0],
                                                          "yes" if x[2] < b[1] else "NO"))
        lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
