"""Points per second of cc_assign (Handle.assign: transfers inside the call) against a settled table, beside the plain
snapshot scan of the same handle in the same process - k_scan_u does the same arithmetic per (point, row) and is the
yardstick, not the assign call itself.

Shapes: C2 (1 M x 20 against the 5 000 rows its own stream settles at) and C5h (2 M x 40 against 50 000 rows).  Per shape:
one online run builds the table, a second one over the same points (no reset: every point joins a microcluster) runs with
pruning off and time_kernels on and gives k_scan_u's launches and their HIP-event time; then the same points are assigned
REPS times from pageable memory and from a page-locked copy (torch's pinned allocator, if torch is there).
Usage: python tools/assign_rate.py [C2] [C5h] [--out profiles/assign.txt]; environment: REPS (3)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SHAPES = {"C2": (1_000_000, 20, 5000), "C5h": (2_000_000, 40, 50_000)}


def pinned_copy(X):
    """X in page-locked host memory, or None where no allocator for it can be had."""
    try:
        import torch
        t = torch.empty(X.shape, dtype=torch.float64, pin_memory=True)
        a = t.numpy()
        a[...] = X
        return a, t  # (the tensor keeps the allocation alive)
    except Exception as e:  # noqa: BLE001 - reported, the pageable figure stands alone
        print("no page-locked copy (%s)" % e, flush=True)
        return None, None


def measure(name, reps, lines):
    from chronoclust_amd import _lib
    n, d, g = SHAPES[name]
    X = bench.make_blobs(42, n, d, g)
    os.environ["CHRONOCLUST_HIP_PRUNE"] = "0"   # the plain scan on every window
    h = _lib.Handle(0)
    h.set_tuning(time_kernels=1, sequential=1)
    bench.set_params(h, bench.blob_config(n), n, d)
    h.points_upload(X)
    h.online_run()
    rows = h.count(_lib.PCORE) + h.count(_lib.OUTLIER)
    h.online_run()
    s = h.stats()
    scan_points = s["scan_pair_dims"] / max(1.0, float(rows) * d)
    scan_rate = scan_points / max(1e-9, s["scan_ms"]) * 1e3
    lines.append("%s: %d x %d against %d rows (%d pcore)" % (name, n, d, rows, h.count(_lib.PCORE)))
    lines.append("  plain snapshot scan (k_scan_u: %d of %d windows): %d launches, %.1f us each, %.1f M points/s" % (
        s["scan_u_launches"], s["windows"], s["scan_launches"], 1e3 * s["scan_ms"] / max(1, s["scan_launches"]),
        scan_rate / 1e6))
    Xp, keep = pinned_copy(X)
    for what, arr in (("pageable", X), ("page-locked", Xp)):
        if arr is None:
            continue
        h.assign(arr[:4096])   # buffers allocated, code loaded
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            uid, path, _ = h.assign(arr)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        st = h.stats()
        lines.append("  cc_assign, %s input, transfers inside: %.2f ms = %.1f M points/s = %.2f x the plain scan "
                     "(%d chunks; paths %s)" % (what, 1e3 * best, n / best / 1e6, n / best / scan_rate, st["assign_launches"],
                                                dict(zip(*[x.tolist() for x in np.unique(path, return_counts=True)]))))
    h.close()
    del keep
    print("\n".join(lines[-4:]), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        out = args[args.index("--out") + 1]
        del args[args.index("--out"):args.index("--out") + 2]
    lines = []
    for name in args or ["C2", "C5h"]:
        measure(name, int(os.environ.get("REPS", "3")), lines)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
