"""Wide-dimension timings (d = 128 / 256 / 512 / 1 024): one fixed stream shape - 20 000 points of
300 anisotropic blobs, which settle on a few hundred microclusters - with the pdim filter off (pi = 0 -> d) and on
(pi = d - 3), k = 4.  Beyond 64 dimensions every point runs on k_seq_g (the wide form beyond 128).  Per width and filter:

  online   host time of one synchronised HDDStream.online_microcluster_maintenance call (upload, online phase, labels,
           offline phase) per point, and the online phase alone (cc_stats.run_ms) per point;
  kernel   k_seq_g's own time per point, from a separate `rocprofv3 --kernel-trace --stats` run of this tool
           (--online-only D, one child process per width);
  offline  one more offline phase on the table the stream left (cc_offline + export);
  assoc    one assoc_argmin of 2 000 x 2 000 random pcores (median of three, host copies included);
  oracle   the single-thread C oracle (oracle/chrono_oracle.c) on the same stream, its online phase alone (offline=False):
           points per second, against the GPU's online phase alone (cc_stats.run_ms).

Then the two expectations: online time per point at most 1.3 x (d / 128) x the d = 128 figure, and the GPU ahead of the
oracle at every width.  Usage:

    python tools/wide_dims.py [--out FILE] [--no-kernels] [--dims 128,256,512,1024]
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, G, SIGMA, WIDE_DIMS, WIDE_SIGMA, K = 20000, 300, 0.01, 8, 0.08, 4.0


def stream(d):
    rng = np.random.default_rng(4000 + d)
    centres = rng.uniform(0.1, 0.9, (G, d))
    sig = np.full((G, d), SIGMA)
    for i in range(G):
        sig[i, rng.choice(d, WIDE_DIMS, replace=False)] = WIDE_SIGMA
    lab = rng.integers(0, G, N)
    return np.ascontiguousarray(np.clip(centres[lab] + rng.normal(0.0, 1.0, (N, d)) * sig[lab], 0.0, 1.0))


def config(d, filt):
    import scenarios
    eps = float(np.sqrt(2.0 * (d * SIGMA * SIGMA / K + WIDE_DIMS * WIDE_SIGMA * WIDE_SIGMA)))
    return scenarios.params_to_config(scenarios.blob_params(N, param_epsilon=eps, param_k=K,
                                                            param_pi=(d - 3) if filt else 0))


def run_gpu(d, filt, X):
    from chronoclust_amd.clustering.hddstream import HDDStream
    h = HDDStream(config(d, filt))
    t0 = time.perf_counter()
    h.online_microcluster_maintenance(X, 0)  # (returns once labels and clusters are on the host: synchronised)
    host_ms = (time.perf_counter() - t0) * 1e3
    s = h.stats()
    t0 = time.perf_counter()
    h._h.offline_arrays()
    off_ms = (time.perf_counter() - t0) * 1e3
    return dict(host_us=host_ms * 1e3 / N, online_us=s["run_ms"] * 1e3 / N, seq_g=s["seq_g_points"], windows=s["windows"],
                rows=s["rows"], pcores=len(h.table(0)["id"]), clusters=len(h.final_clusters), offline_ms=off_ms)


def run_assoc(d):
    from chronoclust_amd import _lib
    rng = np.random.default_rng(d)
    hd = _lib.Handle(0)
    hd.set_params(0.01, 0.01, K, 0.5, 1.0, 0.0, 0.1, 0.01, 0.1, d)
    cur, prev = rng.random((2000, d)), rng.random((2000, d))
    pref = np.where(rng.random((2000, d)) < 0.5, K, 1.0)
    hd.assoc_argmin(cur, pref, prev)  # (warm-up: buffers, code object)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        hd.assoc_argmin(cur, pref, prev)
        ts.append((time.perf_counter() - t0) * 1e3)
    hd.close()
    return float(np.median(ts))


def run_oracle(d, filt, X):
    from oracle import oracle as O
    o = O.OracleHDDStream(config(d, filt))
    t0 = time.perf_counter()
    o.online_microcluster_maintenance(X, 0, offline=False)  # (like for like with cc_stats.run_ms: the online phase alone)
    return N / (time.perf_counter() - t0)


def kernel_times(dims, timeout):
    """k_seq_g's own time per point from one rocprofv3 child per width: {(d, filter): us per point}."""
    out = {}
    for d in dims:
        tmp = tempfile.mkdtemp(prefix="wide_dims_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "wd", "--",
               sys.executable, os.path.abspath(__file__), "--online-only", str(d)]
        subprocess.run(cmd, check=True, timeout=timeout, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel trace under %s" % tmp)
        tot = {False: 0.0, True: 0.0}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                if "k_seq_g" in name:
                    # the first template argument, demangled (k_seq_g<true, ...) or not (_Z7k_seq_gILb1E...)
                    if "k_seq_g<" in name:
                        filt = name.split("k_seq_g<", 1)[1].startswith("true")
                    elif "k_seq_gILb" in name:
                        filt = name.split("k_seq_gILb", 1)[1].startswith("1")
                    else:
                        raise RuntimeError("cannot tell the filter form of %r" % name)
                    tot[filt] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
        for filt in (False, True):
            out[(d, filt)] = tot[filt] / N
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="128,256,512,1024")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--online-only", type=int, default=0, help="(the profiled child: both streams of one width, nothing else)")
    ap.add_argument("--kernel-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.online_only:
        from chronoclust_amd.clustering.hddstream import HDDStream
        X = stream(a.online_only)
        for filt in (False, True):
            HDDStream(config(a.online_only, filt)).online_microcluster_maintenance(X, 0)
        return
    dims = [int(x) for x in a.dims.split(",")]
    rows = []
    from chronoclust_amd.clustering.hddstream import HDDStream
    for d in dims:
        X = stream(d)
        for filt in (False, True):
            HDDStream(config(d, filt)).online_microcluster_maintenance(X[:500], 0)  # (warm-up: code objects, buffers)
            r = dict(d=d, filt=filt, **run_gpu(d, filt, X))
            r["oracle_pps"] = run_oracle(d, filt, X) if not a.no_oracle else float("nan")
            rows.append(r)
            print("d %4d filter %-3s: online %.2f us/pt (host %.2f), rows %d, pcores %d, clusters %d, seq_g %d, windows %d, "
                  "offline %.1f ms, oracle %.0f pts/s" % (d, "on" if filt else "off", r["online_us"], r["host_us"], r["rows"],
                                                          r["pcores"], r["clusters"], r["seq_g"], r["windows"], r["offline_ms"],
                                                          r["oracle_pps"]), flush=True)
    assoc = {d: run_assoc(d) for d in dims}
    kern = kernel_times(dims, a.kernel_timeout) if not a.no_kernels else {}
    lines = ["# tools/wide_dims.py: %d points, %d blobs (sigma %g, %d dimensions of each at %g), k = %g; filter off: pi = 0 "
             "(-> d), on: pi = d - 3" % (N, G, SIGMA, WIDE_DIMS, WIDE_SIGMA, K),
             "# us/pt: online = cc_stats.run_ms / n, host = the whole synchronised online_microcluster_maintenance call / n "
             "(offline phase included), kernel = k_seq_g's own time / n (rocprofv3 --kernel-trace); offline = one more "
             "offline phase (ms); assoc = assoc_argmin 2 000 x 2 000 (ms, median of 3); oracle = single-thread C oracle, "
             "online phase alone, points/s; gpu = 1e6 / online",
             "%5s %6s %6s %6s %9s %9s %9s %10s %9s %11s %11s %9s" % ("d", "filter", "rows", "pcores", "online", "host",
                                                                   "kernel", "offline_ms", "assoc_ms", "oracle_pps",
                                                                   "gpu_pps", "gpu/orc")]
    for r in rows:
        k = kern.get((r["d"], r["filt"]), float("nan"))
        gpu_pps = 1e6 / r["online_us"]
        lines.append("%5d %6s %6d %6d %9.2f %9.2f %9.2f %10.2f %9.2f %11.0f %11.0f %9.1f" % (
            r["d"], "on" if r["filt"] else "off", r["rows"], r["pcores"], r["online_us"], r["host_us"], k, r["offline_ms"],
            assoc[r["d"]], r["oracle_pps"], gpu_pps, gpu_pps / r["oracle_pps"]))
    lines.append("# expectation 1: online us/pt at d <= 1.3 x (d / 128) x the d = 128 figure")
    for filt in (False, True):
        base = [r for r in rows if r["d"] == 128 and r["filt"] == filt]
        if not base:
            continue
        b = base[0]["online_us"]
        for r in rows:
            if r["filt"] == filt and r["d"] != 128:
                lim = 1.3 * (r["d"] / 128.0) * b
                lines.append("#   filter %-3s d %4d: %.2f us/pt, limit %.2f -> %s (%.2f x the d = 128 figure for %.0f x the "
                             "dimensions)" % ("on" if filt else "off", r["d"], r["online_us"], lim,
                                              "met" if r["online_us"] <= lim else "MISSED", r["online_us"] / b, r["d"] / 128.0))
    lines.append("# expectation 2: the GPU ahead of the single-thread oracle at every width")
    for r in rows:
        ok = 1e6 / r["online_us"] > r["oracle_pps"]
        lines.append("#   filter %-3s d %4d: %s" % ("on" if r["filt"] else "off", r["d"], "met" if ok else "MISSED"))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
