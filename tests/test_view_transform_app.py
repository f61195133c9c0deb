"""app.run on CSV timepoints with `.transform` sidecars (read_timepoint -> _lib.TransformedPoints -> the `_view_xl` route) against
the same events as `.fcs` timepoints (ListMode -> the `_list_xl` route): one run each, result.csv and every per-point file equal
byte for byte.  The events are float32 multiples of 1 / 64 below 2^18, written to the CSV with repr: at most twelve significant
digits, which pandas' default parser - the one app.run documents - reads exactly (asserted), so both files hold the same values;
the CSV sidecar carries under "spillover" the matrix the `.fcs` files hold in $SPILLOVER.  A CSV run without a sidecar still
writes its golden: the guard that the plain route is where it was."""
import json
import os

import numpy as np
import pytest

import fcs_util as F
import logicle_util as L
import scenarios
import transform_util as U
from golden_util import GOLDEN
from test_app_end_to_end import _reset_logging

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

N, D, TIMEPOINTS = 2000, 5, 3
MARKERS = ["CD%d" % i for i in range(D)]
COMP = [MARKERS[3], MARKERS[0], MARKERS[4]]
LOGICLE = dict(T=262144, W=0.5, M=4.5, A=0)


def events(t, logicle):
    """float32 [N, D] whose transform gives (about) the blobs of scenarios.make_blobs, three channels spilled into each other"""
    X = scenarios.make_blobs(900 + t, N, D, 8, 0.01)
    truth = L.inverse(X, 262144.0, 0.5, 4.5, 0.0) if logicle else np.sinh(X) * 5.0
    idx = [MARKERS.index(c) for c in COMP]
    truth[:, idx] = truth[:, idx] @ U.spillover(3, 8)[0]  # (building an input: any rounding will do)
    rec = (np.round(truth * 64.0) / 64.0).astype(np.float32)
    assert np.abs(rec).max() < 2.0 ** 18 and np.array_equal(rec.astype(np.float64) * 64.0, np.round(rec.astype(np.float64) * 64.0))
    return rec


@pytest.mark.parametrize("logicle,normalise", [(False, True), (True, False)], ids=["cofactor-scaled", "logicle-unscaled"])
def test_csv_timepoints_with_sidecars_write_what_fcs_timepoints_write(tmp_path, monkeypatch, logicle, normalise):
    from chronoclust_amd import _lib, app
    from chronoclust_amd.scaling.scaler import read_timepoint
    spill = U.spillover(3, 8)[0]
    ask = {"compensate": True, "logicle": LOGICLE} if logicle else {"compensate": True, "cofactor": 5}
    params = scenarios.blob_params(N)
    fcs_files, csv_files = [], []
    for t in range(TIMEPOINTS):
        rec = events(t, logicle)
        fn = os.path.join(str(tmp_path), "tp%d.fcs" % t)
        F.write_fcs(fn, F.fast_records(rec, U.BIG), D, "F", U.BIG, 32, names=MARKERS, tot=N,
                    extra={"$SPILLOVER": U.spillover_text(COMP, spill)})
        with open(fn + ".transform", "w") as f:
            json.dump(ask, f)
        fcs_files.append(fn)
        fn = os.path.join(str(tmp_path), "tp%d.csv" % t)
        with open(fn, "w") as f:
            f.write(",".join(MARKERS) + "\n")
            f.writelines(",".join(repr(float(v)) for v in row) + "\n" for row in rec)
        with open(fn + ".transform", "w") as f:
            json.dump(dict(ask, spillover={"channels": COMP, "matrix": spill.tolist()}), f)
        csv_files.append(fn)
        tp = read_timepoint(fn)
        assert isinstance(tp, _lib.TransformedPoints) and tp.points.flags["F_CONTIGUOUS"] and tp.transform.m == 3
        assert np.array_equal(tp.array, rec.astype(np.float64)), "the CSV parse is not exact"
    seen, made = [], []

    class Recording(app.HDDStream):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

        def online_microcluster_maintenance(self, input_dataset, *a, **kw):
            seen.append(input_dataset)
            return super().online_microcluster_maintenance(input_dataset, *a, **kw)

    # neither run transforms on the host
    monkeypatch.setattr(app, "HDDStream", Recording)
    monkeypatch.setattr(_lib.ListMode, "__array__", lambda *a, **kw: pytest.fail("the events were decoded on the host"))
    monkeypatch.setattr(_lib.TransformedPoints, "__array__", lambda *a, **kw: pytest.fail("the array was transformed on the host"))
    outs = []
    try:
        for name, files in (("out_fcs", fcs_files), ("out_csv", csv_files)):
            out = os.path.join(str(tmp_path), name)
            os.makedirs(out)
            app.run(data=files, output_directory=out, normalise_data=normalise, **params)
            outs.append(out)
            _reset_logging()
    finally:
        _reset_logging()
    assert len(seen) == 2 * TIMEPOINTS
    assert all(isinstance(x, _lib.ListMode) for x in seen[:TIMEPOINTS]) and all(isinstance(x, _lib.TransformedPoints) for x in seen[TIMEPOINTS:])
    stats = made[1].stats()
    assert stats["view_points"] >= TIMEPOINTS * N and stats["list_points"] == 0 and stats["f32_points"] == 0
    for fn in ["result.csv"] + ["cluster_points_D%d.csv" % t for t in range(TIMEPOINTS)]:
        a, b = (open(os.path.join(o, fn), "rb").read() for o in outs)
        assert a == b and len(a) > 0, fn
    assert len(open(os.path.join(outs[1], "result.csv")).read().splitlines()) > 3, "no cluster was written: nothing was compared"


def test_a_csv_run_without_a_sidecar_still_writes_its_golden(tmp_path):
    """The guard: the no-cluster integration run of test_app_end_to_end.py, whose CSV timepoints have no sidecar."""
    from chronoclust_amd import app
    nc = os.path.join(GOLDEN, "nocluster")
    try:
        app.run(data=[os.path.join(nc, "synthetic_d%d.csv.gz" % t) for t in range(5)], output_directory=str(tmp_path),
                **scenarios.NOCLUSTER_PARAMS)
    finally:
        _reset_logging()
    assert open(os.path.join(str(tmp_path), "result.csv"), "rb").read() == open(os.path.join(nc, "expected_result.csv"), "rb").read()
    for t in range(5):
        assert open(os.path.join(str(tmp_path), "cluster_points_D%d.csv" % t), "rb").read() == \
            open(os.path.join(nc, "expected_cluster_points_D%d.csv" % t), "rb").read()
