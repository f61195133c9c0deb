"""FCS timepoints through app.run: the bundled d0-d4 timepoints written as FCS files - $DATATYPE D, big-endian, extra Time /
FSC / SSC channels interleaved and holding NaN patterns, a `.columns` sidecar naming the markers in the CSV's order - give
result.csv and every cluster_points_D{t}.csv byte for byte what the CSV run writes (the committed goldens); the same with
normalise_data=False, for a float32 little-endian file against the float32 `.npy` run of the same values, and for a
stop-and-resume run."""
import gzip
import os

import numpy as np
import pandas as pd
import pytest

import fcs_util as F
import scenarios
from golden_util import GOLDEN
from test_app_end_to_end import _reset_logging

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

C1 = os.path.join(GOLDEN, "c1")
GATING = os.path.join(C1, "gating_centroids.csv")
LITTLE, BIG = (1, 2, 3, 4), (4, 3, 2, 1)
EXTRA = ["Time", "FSC-A", "SSC-A"]
NAN_BITS = {8: (0x7FF8000000000000, 0xFFF0000000000001, 0x7FF0000000000000), 4: (0x7FC00000, 0xFF800001, 0x7F800000)}

_frames = []


def frames():
    if not _frames:
        _frames.extend(pd.read_csv(os.path.join(C1, "synthetic_d%d.csv.gz" % t)) for t in range(5))
    return _frames


def write_timepoints(folder, dtype, order):
    """The five timepoints as FCS files of `dtype`: channels Time, marker 0, FSC-A, marker 1, SSC-A, marker 2, ...; the
    sidecar names the markers in the CSV's order.  Returns (files, the marker values as stored)."""
    files, stored = [], []
    for t, frame in enumerate(frames()):
        markers = list(frame.columns)
        x = frame.to_numpy().astype(dtype)
        names = []
        for i, m in enumerate(markers):
            if i < len(EXTRA):
                names.append(EXTRA[i])
            names.append(m)
        rec = np.zeros((len(x), len(names)), dtype=dtype)
        image = rec.view("u%d" % rec.dtype.itemsize)
        for c, name in enumerate(names):
            if name in markers:
                rec[:, c] = x[:, markers.index(name)]
            else:
                image[:, c] = NAN_BITS[rec.dtype.itemsize][EXTRA.index(name)]
        fn = os.path.join(str(folder), "tp%d.fcs" % t)
        bits = 8 * rec.dtype.itemsize
        F.write_fcs(fn, F.fast_records(rec, order), len(names), "D" if bits == 64 else "F", order, bits, names=names, tot=len(rec),
                    pad_before_data=t % 2)  # (every other file's DATA segment starts at another parity)
        with open(fn + ".columns", "w") as f:
            f.write("\n".join(markers) + "\n")
        files.append(fn)
        stored.append(x)
    return files, stored


def run(files, out, **kw):
    from chronoclust_amd import app
    os.makedirs(out, exist_ok=True)
    try:
        app.run(data=files, output_directory=out, **dict(scenarios.C1_PARAMS, **kw))
    finally:
        _reset_logging()
    return out


def same_as_golden(out):
    with open(os.path.join(C1, "expected_result.csv"), newline="") as f:
        exp = f.read()
    with open(os.path.join(out, "result.csv"), newline="") as f:
        got = f.read()
    assert got.replace("\r\n", "\n") == exp.replace("\r\n", "\n")
    rec = np.load(os.path.join(C1, "hdd_state.npz"))
    for t in range(5):
        exp_text = gzip.decompress(rec["t%d_points_csv" % t].tobytes())
        assert open(os.path.join(out, "cluster_points_D%d.csv" % t), "rb").read() == exp_text, t


def same_files(a, b):
    for fn in ["result.csv"] + ["cluster_points_D%d.csv" % t for t in range(5)]:
        x, y = (open(os.path.join(o, fn), "rb").read() for o in (a, b))
        assert x == y and len(x) > 0, fn


def test_fcs_timepoints_give_the_csv_runs_files(tmp_path, monkeypatch):
    from chronoclust_amd import _lib, app
    seen, made = [], []

    class Recording(app.HDDStream):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

        def online_microcluster_maintenance(self, input_dataset, *a, **kw):
            seen.append(input_dataset)
            return super().online_microcluster_maintenance(input_dataset, *a, **kw)

    monkeypatch.setattr(app, "HDDStream", Recording)
    files, stored = write_timepoints(tmp_path, np.float64, BIG)
    out = run(files, os.path.join(str(tmp_path), "out"), gating_centroid_file=GATING)
    same_as_golden(out)
    # the device decoded them: every timepoint reached the HDDStream as the file's own bytes
    assert len(seen) == 5 and all(isinstance(x, _lib.ListMode) and x.swapped for x in seen)
    assert [x.shape for x in seen] == [s.shape for s in stored]
    assert made[0].stats()["list_points"] == sum(len(s) for s in stored) and made[0].stats()["view_points"] == 0


def test_fcs_timepoints_without_normalisation(tmp_path):
    files, _ = write_timepoints(tmp_path, np.float64, BIG)
    csvs = [os.path.join(C1, "synthetic_d%d.csv.gz" % t) for t in range(5)]
    a = run(files, os.path.join(str(tmp_path), "out_fcs"), normalise_data=False)
    b = run(csvs, os.path.join(str(tmp_path), "out_csv"), normalise_data=False)
    same_files(a, b)


def test_float32_little_endian_against_the_float32_npy_run(tmp_path):
    files, stored = write_timepoints(tmp_path, np.float32, LITTLE)
    npys = []
    for t, x in enumerate(stored):
        fn = os.path.join(str(tmp_path), "tp%d.npy" % t)
        np.save(fn, x)
        with open(fn + ".columns", "w") as f:
            f.write("\n".join(frames()[t].columns) + "\n")
        npys.append(fn)
    for kw in (dict(gating_centroid_file=GATING), dict(normalise_data=False)):
        tag = "_".join(sorted(kw))
        a = run(files, os.path.join(str(tmp_path), "out_fcs_" + tag), **kw)
        b = run(npys, os.path.join(str(tmp_path), "out_npy_" + tag), **kw)
        same_files(a, b)


def test_stop_and_resume_on_fcs_timepoints(tmp_path):
    import chronoclust_amd.app as A
    files, _ = write_timepoints(tmp_path, np.float64, BIG)
    out = os.path.join(str(tmp_path), "out")

    class Stop(Exception):
        pass

    orig = A.save_program_state

    def save_and_maybe_stop(h, o, ta, tl):
        orig(h, o, ta, tl)
        if h.last_data_timestamp == 2:
            raise Stop()
    A.save_program_state = save_and_maybe_stop
    try:
        with pytest.raises(Stop):
            run(files, out, gating_centroid_file=GATING)
    finally:
        A.save_program_state = orig
    assert open(os.path.join(out, "result.csv")).read().count("\n") < 24
    run(files, out, gating_centroid_file=GATING, restore_program=True)
    same_as_golden(out)
