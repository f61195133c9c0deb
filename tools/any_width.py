"""A C2-shaped stream (1 M points, 5 000 populations, default tuning) at widths off the ladder of compiled scan widths and
at their ladder neighbours: per width the whole-call rate (empty table: start-up and steady state together) and the
steady-state rate (the same points again without a reset, as tools/steady.py), every repetition printed so that the
run-to-run spread stands beside the figures; beside each padded width the ratio to its neighbour.

    python3 tools/any_width.py                      # every width, the table of profiles/any_width.txt
    python3 tools/any_width.py --dims 18,20 --reps 5
    python3 tools/any_width.py --pad-time 18,37     # k_pad_rows per launch: one child per width under rocprofv3 --kernel-trace

The script uses nothing the library did not have before the padded scans, so a copy of it runs in a checkout of an older
commit: that is how a build is compared with its parent on one machine (alternate the two)."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PADDED = {13: 14, 18: 20, 25: 32, 30: 32, 37: 40, 50: 64}
LADDER = (14, 20, 32, 40, 64)


def measure(d, n, g, reps):
    import bench
    from chronoclust_amd import _lib
    X = bench.make_blobs(42, n, d, g)
    cfg = bench.blob_config(n)
    h = _lib.Handle(0)
    bench.set_params(h, cfg, n, d)
    h.points_upload(X)
    whole, steady, s = [], [], {}
    for _ in range(reps):
        h.reset()
        h.online_run()
        whole.append(n / h.stats()["run_ms"] / 1e3)
        h.online_run()  # (same daystamp: no decay, every point joins an existing microcluster)
        s = h.stats()
        steady.append(n / s["run_ms"] / 1e3)
    h.close()
    return whole, steady, s


def pad_time(d, n, g):
    """k_pad_rows (and the scans behind it) per launch at width d: a fresh child under rocprofv3 --kernel-trace, one repetition."""
    out = tempfile.mkdtemp(prefix="any_width_trace_")
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable,
                    os.path.abspath(__file__), "--dims", str(d), "--reps", "1", "--n", str(n), "--g", str(g)],
                   check=True, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    per = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"].replace("void ", "").split("(")[0]
        if name.startswith(("k_pad_rows", "k_scan_u", "k_scan_p3", "k_seed16", "k_prefix16", "k_seed_merge")):
            per.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for name in sorted(per):
        v = sorted(per[name])
        print("d %2d  %-28s %5d launches, median %8.1f us, mean %8.1f us, max %8.1f us" % (
            d, name[:28], len(v), v[len(v) // 2], sum(v) / len(v), v[-1]), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default=",".join(str(x) for x in sorted(set(PADDED) | set(LADDER))))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--g", type=int, default=5000)
    ap.add_argument("--pad-time", default="")
    a = ap.parse_args()
    if a.pad_time:
        for d in (int(x) for x in a.pad_time.split(",")):
            pad_time(d, a.n, a.g)
        sys.exit(0)
    fmt = lambda v: " ".join("%6.2f" % x for x in v)  # noqa: E731
    best = {}
    for d in (int(x) for x in a.dims.split(",")):
        whole, steady, s = measure(d, a.n, a.g, a.reps)
        best[d] = (max(whole), max(steady))
        print("d %2d  whole call %s  steady %s  M points/s | last run: windows %d, scans %d of them pruned %d, pad passes %d" % (
            d, fmt(whole), fmt(steady), s["windows"], s["scan_u_launches"], s["scan_p_launches"], s.get("pad_rows_launches", 0)),
            flush=True)
    for d, nb in sorted(PADDED.items()):
        if d in best and nb in best:
            print("d %2d / d %2d (best of %d): whole call %.3f, steady %.3f" % (
                d, nb, a.reps, best[d][0] / best[nb][0], best[d][1] / best[nb][1]), flush=True)
