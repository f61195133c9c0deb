"""MinMax [0, 1] scaling fitted on all timepoints: the interface of chronoclust/scaling/scaler.py:11-54.

The reference delegates to scikit-learn's MinMaxScaler; the arithmetic feeds the hot path, so it is restated
here operation by operation (sklearn/preprocessing/_data.py, MinMaxScaler.partial_fit / transform /
inverse_transform): scale_ = 1 / range (range < 10 eps -> 1), min_ = 0 - data_min * scale_,
transform = X * scale_ + min_ (two roundings), inverse = (X - min_) / scale_.
tests/test_host_logic.py checks bit equality against scikit-learn."""
import numpy as np
import pandas as pd

from .._lib import SOURCE_OBJECTS, TransformedPoints, points_source


def read_timepoint(filename, logicle=None):
    """One timepoint as float64 [N, d].  CSV with a header row as in the reference (app.py:170, scaler.py:31);
    `.npy` files (binary side input: no text parse) are taken as they are - a float32 file stays float32 (cytometry events are
    single precision at the source; the device widens them), anything else becomes float64.  `.fcs` files (fcs.read_fcs) come
    back as a `_lib.ListMode` over the memory-mapped DATA segment - the device decodes it - or, for the layouts that route
    does not take, as a float64 array decoded on the host; `<file>.columns` (one name per line, matched against $PnN, then
    $PnS) selects and orders the channels, without it all channels are taken in file order; `<file>.transform` (JSON:
    {"compensate": bool, "cofactor": number | {name: number}, "logicle": {T, W, M, A} | {name: {T, W, M, A}}},
    fcs.sidecar_transform) asks for the file's own spillover compensation and arcsinh(x / cofactor) or the logicle scale,
    applied on the device as the events land (read_fcs).  Beside a `.csv` or `.npy` timepoint `<file>.transform` takes the same
    keys and "spillover": {"channels": [names], "matrix": [[...]]} in the place of the file's own keyword (fcs.array_transform;
    names: the CSV header, `<file>.columns` for a `.npy`); the timepoint then comes back as a `_lib.TransformedPoints`, which
    the device compensates and transforms as it takes the array in.  logicle: {path: logicle rows by channel name} - the rows that take
    the place of the sidecar's for that file: what fcs.estimate_sidecars resolved where a sidecar holds "W": "estimate"."""
    if str(filename).lower().endswith(".fcs"):
        from ..fcs import read_fcs, sidecar_columns, sidecar_transform
        kw = sidecar_transform(filename) or {}
        if logicle and filename in logicle:
            kw = dict(kw, logicle=logicle[filename])
        return read_fcs(filename, columns=sidecar_columns(filename), **kw)[0]
    from ..fcs import array_transform, sidecar_columns, sidecar_transform
    kw = sidecar_transform(filename)
    if str(filename).endswith(".npy"):
        X = np.load(filename)
        X = np.ascontiguousarray(X, dtype=np.float32 if X.dtype == np.float32 else np.float64)
        names = sidecar_columns(filename) if kw else None
        if kw and (names is None or len(names) != X.shape[1]):
            raise ValueError("%s.transform needs %s.columns with one name per column (%d)" % (filename, filename, X.shape[1]))
    else:
        frame = pd.read_csv(filename, header=0, sep=',')
        X, names = frame.to_numpy(), [str(c) for c in frame.columns]
    # (`<file>.transform` beside a CSV or .npy: the transform rides with the array and the device applies it - _view_xl)
    transform = array_transform(filename, names, **kw) if kw else None
    return X if transform is None else TransformedPoints(X, transform)


class Scaler(object):
    def __init__(self, data_files=None, handle=None, logicle=None):
        """handle: a chronoclust_amd._lib.Handle.  With it the fit reduces every file's columns on the device
        (cc_col_minmax) and the parsed files are kept for the run, so that no file is parsed twice.
        logicle: read_timepoint's {path: resolved logicle rows}, handed on to it."""
        self.scale_ = None
        self.min_ = None
        self.input_data = []
        self._handle = handle
        self.parsed = {}
        if data_files is not None and handle is not None:
            lo = hi = None
            for filename in data_files:
                # (kept as parsed where the library reads it where it lies - pandas hands a CSV out column-major -, else as
                # a C-contiguous float64 copy)
                X = read_timepoint(filename, logicle)
                if not isinstance(X, SOURCE_OBJECTS):  # (event records, an array with its transform: read where they lie)
                    X = points_source(X)[0]
                self.parsed[filename] = X
                if X.shape[0] == 0:
                    continue
                mn, mx = handle.col_minmax(X)
                lo = mn if lo is None else np.fmin(lo, mn)
                hi = mx if hi is None else np.fmax(hi, mx)
            self._finish_fit(lo, hi)
        elif data_files is not None:
            rows = []
            for filename in data_files:
                rows.append(np.asarray(read_timepoint(filename, logicle)))
            self.fit_scaler(np.concatenate(rows, axis=0) if rows else np.empty((0, 0)))

    def _finish_fit(self, data_min, data_max):
        data_range = data_max - data_min
        safe = data_range.copy()
        safe[safe < 10 * np.finfo(np.float64).eps] = 1.0
        self.scale_ = (1.0 - 0.0) / safe
        self.min_ = 0.0 - data_min * self.scale_
        self.data_min_, self.data_max_, self.data_range_ = data_min, data_max, data_range

    def fit_scaler(self, data):
        X = np.asarray(data, dtype=np.float64)
        self._finish_fit(np.nanmin(X, axis=0), np.nanmax(X, axis=0))
        self.set_input_data(data)

    def scale_data(self, data):
        X = np.array(data, dtype=np.float64)  # copy
        X *= self.scale_
        X += self.min_
        return X

    def reverse_scaling(self, data):
        X = np.array(data, dtype=np.float64)
        X -= self.min_
        X /= self.scale_
        return X

    def set_input_data(self, data):
        self.input_data = data

    def get_input_data(self):
        return self.input_data
