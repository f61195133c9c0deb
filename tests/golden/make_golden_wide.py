#!/usr/bin/env python3
"""Generates tests/golden/blob_d160.npz (TEST INFRASTRUCTURE): a d = 160 blob scenario run through the reference's
app.run, recorded like make_golden.py's blob_*.npz (per-timepoint state dumps, result.csv, per-point cluster ids).

Runs ONLY where the upstream Python reference can be imported (oracle/ref_harness/refenv.py); the GPU test
(tests/test_any_dims.py) reads the committed .npz alone.  The scenario lives here and in that test, not in
tests/scenarios.py: a new entry of scenarios.BLOB_SCENARIOS would grow the existing parametrized tests.

    python tests/golden/make_golden_wide.py
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_harness"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import refenv  # noqa: E402
import scenarios  # noqa: E402
from make_golden import Recorder, read_labels, reset_logging, save_calls  # noqa: E402

# beyond 128 dimensions (k_seq_g's wide form online, the dimension-blocked K6 offline): ~1 500 points per timepoint, the
# pdim filter on (pi < d: every blob is wide in 12-20 dimensions, so that its microclusters prefer at most pi of them),
# decay and outlier deletion (lambda, omicron > 0); epsilon lets the blobs' microclusters grow and get promoted, and an
# upsilon * epsilon wider than the distance between blobs gives the offline phase neighbourhoods of several of them
D160 = dict(seed=160, n=1500, d=160, g=10, sigma=0.01, wide_dims=(12, 20), wide_sigma=0.08, timepoints=3, drift=0.01,
            churn=0.2, params=scenarios.blob_params(1500, param_epsilon=0.4, param_pi=150, param_upsilon=10.0,
                                                    param_omicron=0.0002, param_lambda=1.5))


def gen_d160(path=os.path.join(HERE, "blob_d160.npz")):
    from chronoclust import app
    import pandas as pd
    sc = D160
    Xs = scenarios.make_blob_timepoints(sc, raw=True)
    tmp = tempfile.mkdtemp()
    files = []
    cols = ["m%d" % i for i in range(sc["d"])]
    for t, X in enumerate(Xs):
        fn = os.path.join(tmp, "tp%d.csv" % t)
        pd.DataFrame(X, columns=cols).to_csv(fn, index=False)  # repr floats: exact round trip
        assert (pd.read_csv(fn).to_numpy() == scenarios.through_csv(X)).all()
        files.append(fn)
    out = os.path.join(tmp, "out")
    os.makedirs(out)
    rec = Recorder()
    rec.install()
    try:
        app.run(data=files, output_directory=out, normalise_data=False, **sc["params"])
    finally:
        rec.uninstall()
        reset_logging()
    extra = {"result_csv": np.frombuffer(open(os.path.join(out, "result.csv"), "rb").read(), dtype=np.uint8)}
    for t in range(len(Xs)):
        ids, cl = read_labels(os.path.join(out, "cluster_points_D%d.csv" % t))
        assert (ids == np.arange(len(ids))).all()
        extra["t%d_cluster_id" % t] = cl
    save_calls(path, rec.calls, extra, keep_x=False)
    shutil.rmtree(tmp)
    print("blob d160: pcore/outlier/clusters per tp %s, %s s, %d bytes" % (
        [(len(c["pcore_id"]), len(c["outlier_id"]), int(c["n_clusters"][0])) for c in rec.calls],
        [round(c["seconds"], 1) for c in rec.calls], os.path.getsize(path)))


if __name__ == "__main__":
    refenv.load()
    gen_d160(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "blob_d160.npz"))
