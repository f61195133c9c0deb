"""The `_view_xl` route without a GPU: _lib.TransformedPoints' host transform against ListMode's over the same values, the
`.transform` sidecar of a `.csv` / `.npy` timepoint ("spillover" and every refusal with its message), what read_timepoint hands
out, how Handle._source routes a TransformedPoints (which layouts are read where they lie, which are copied), and the five new
symbols in the header and in the binding."""
import ctypes
import json
import os

import numpy as np
import pytest

import transform_util as U
import view_transform_util as V
from chronoclust_amd import _lib, fcs
from chronoclust_amd.scaling.scaler import read_timepoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["FSC-A", "CD3", "CD4", "CD8", "CD19"]
NEW_SYMBOLS = ("cc_points_upload_view_xl", "cc_points_prefetch_view_xl", "cc_col_minmax_view_xl", "cc_online_view_xl",
               "cc_assign_view_xl")


# ---- the host transform -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", V.TYPES, ids=lambda t: np.dtype(t).name)
def test_the_host_transform_is_list_modes_bit_for_bit(dtype):
    n, d = 130, 13
    for li, layout in enumerate(V.LAYOUTS):
        a = V.laid_out(V.values(dtype, n, d, 3 + li), layout)
        for cof, lg in (("none", "none"), ("scalar", "none"), ("per dimension", "some"), ("none", "all")):
            cofactor = V.cofactors(cof, d)
            tr = V.transform(d, 9, li, cofactor, V.logicle_rows(lg, d, cofactor))[0]
            got = np.asarray(_lib.TransformedPoints(a, tr))
            exp = np.asarray(V.referee_source(a, tr))
            assert got.dtype == np.float64 and got.shape == (n, d)
            U.same_bits(got, exp, "%s %s cofactors %s logicle %s" % (np.dtype(dtype).name, layout, cof, lg))
    # the compensation itself is the explicit loop
    tr, cc, inv = V.transform(d, 9, 1)
    x = V.widened(a)
    U.same_bits(np.asarray(_lib.TransformedPoints(a, tr)), U.compensated(x, np.ascontiguousarray(x[:, cc]), np.arange(d), cc, inv), "loop")


def test_transformed_points_is_an_n_by_d_source():
    a = np.asfortranarray(np.arange(12.0).reshape(4, 3))
    tp = _lib.TransformedPoints(a, _lib.ListTransform(cofactor=5.0))
    assert tp.shape == (4, 3) and tp.ndim == 2 and len(tp) == 4
    assert isinstance(tp, _lib.SOURCE_OBJECTS)
    assert np.asarray(tp, dtype=np.float32).dtype == np.float32
    U.same_bits(np.asarray(_lib.TransformedPoints(a, None)), a, "no transform: the values")
    with pytest.raises(ValueError, match="2-d"):
        _lib.TransformedPoints(np.zeros(3), None)
    with pytest.raises(ValueError, match="must be a ListTransform"):
        _lib.TransformedPoints(a, dict(cofactor=5))
    with pytest.raises(ValueError, match="TransformedPoints: dimension 1 has a cofactor and a logicle scale"):
        _lib.TransformedPoints(a, _lib.ListTransform(cofactor=[0.0, 5.0, 0.0], logicle=V.LOGICLE))
    with pytest.raises(ValueError, match="3 selected dimensions"):
        _lib.TransformedPoints(a, _lib.ListTransform(cofactor=[5.0, 5.0]))
    with pytest.raises(ValueError, match="outside 0..2"):
        np.asarray(_lib.TransformedPoints(a, _lib.ListTransform([0, 3], np.eye(2))))
    # rows that are all off are no logicle rows
    assert _lib.TransformedPoints(a, _lib.ListTransform(logicle=np.zeros((3, 4)))).logicle_descriptor() is None


# ---- routing ------------------------------------------------------------------------------------------------------------------------

class StubHandle(_lib.Handle):
    def __init__(self):  # (no library, no device: _source needs neither)
        self._h = None


def deref(arg, typ):
    return ctypes.cast(arg, ctypes.POINTER(typ)).contents


def test_source_routes_transformed_points_to_view_xl_without_a_copy():
    h = StubHandle()
    n, d = 70, 5
    cof = np.full(d, 5.0)
    tr = V.transform(d, 3, 1, cof)[0]
    base = V.values(np.float64, n, d, 1)
    accepted = [V.laid_out(V.values(t, n, d, 2), lay) for t in V.TYPES for lay in V.LAYOUTS]
    assert any(a.flags["C_CONTIGUOUS"] and a.dtype == np.float64 for a in accepted)  # (the plain route's own layouts included)
    assert any(a.flags["C_CONTIGUOUS"] and a.dtype == np.float32 for a in accepted)
    for a in accepted:
        tp = _lib.TransformedPoints(a, tr)
        kind, src, args, n_, d_ = h._source(tp)
        assert (kind, n_, d_) == ("view_xl", n, d) and src is tp and len(args) == 3
        assert tp.points is a, "an accepted layout was copied"
        view = deref(args[0], _lib.CcPointsView)
        assert view.data == a.ctypes.data and view.dtype == _lib.VIEW_DTYPES[a.dtype]
        assert (view.row_stride, view.col_stride) == (a.strides[0] // a.itemsize, a.strides[1] // a.itemsize)
        xf = deref(args[1], _lib.CcListTransform)
        assert xf.m == 3 and args[2] is None
    # the fallbacks: a C-contiguous float64 copy, made once and kept
    fallbacks = [base[:, ::2], np.asfortranarray(base)[::2], base[::-1], base.astype(np.int64), base.astype(">f8"), np.asfortranarray(base)[:, ::-1]]
    for a in fallbacks:
        tp = _lib.TransformedPoints(a, _lib.ListTransform(cofactor=5.0))
        assert _lib.points_view(a) is None
        p = tp.points
        assert p is not a and p.flags["C_CONTIGUOUS"] and p.dtype == np.float64 and np.array_equal(p, a)
        args = h._source(tp)[2]  # (kept: the descriptor lives as long as its reference)
        view = deref(args[0], _lib.CcPointsView)
        assert view.data == p.ctypes.data and view.dtype == _lib.DT_F64 and (view.row_stride, view.col_stride) == (a.shape[1], 1)
        assert h._source(tp)[1] is tp and tp.points is p
    # logicle rows that are on ride as the third argument; no transform: two nulls, the `_view` sibling
    rows = _lib.ListTransform(logicle=V.LOGICLE)
    args = h._source(_lib.TransformedPoints(accepted[0], rows))[2]
    assert args[1] is not None and deref(args[2], _lib.CcListLogicle).d == d
    assert h._source(_lib.TransformedPoints(accepted[0], None))[2][1:] == (None, None)
    # plain arrays keep their routes
    assert h._source(np.asfortranarray(base))[0] == "view" and h._source(base)[0] == "f64"
    assert h._source(base.astype(np.float32))[0] == "f32"


def test_the_new_symbols_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "chronoclust_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(cc_handle* h, const cc_points_view* view, const cc_list_transform* xf, const cc_list_logicle* lg," % name in text
        assert name in _lib.SYMBOLS
    for op, name in zip(("upload", "prefetch", "col_minmax", "assign"), (NEW_SYMBOLS[0], NEW_SYMBOLS[1], NEW_SYMBOLS[2], NEW_SYMBOLS[4])):
        assert _lib._INGEST[op]["view_xl"] == name
    assert _lib._INGEST["upload_scaled"]["view_xl"] == NEW_SYMBOLS[0] and "view_xl" in _lib._DESCRIBED
    from chronoclust_amd import build
    lib = ctypes.CDLL(build.build())
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS)


# ---- sidecars ------------------------------------------------------------------------------------------------------------------------

def write_csv(path, X, names=NAMES):
    """Values with repr: exact for what `dyadic` hands out (pandas' default parser is exact up to 15 significant digits)."""
    with open(path, "w") as f:
        f.write(",".join(names) + "\n")
        for row in X:
            f.write(",".join(repr(float(v)) for v in row) + "\n")


def sidecar(path, spec):
    with open(str(path) + ".transform", "w") as f:
        json.dump(spec, f)


def dyadic(n, d, seed):
    """float64 [n, d] of multiples of 1 / 64 below 2^19: at most 12 significant decimal digits each"""
    return np.round(V.values(np.float64, n, d, seed) * 64.0) / 64.0


SPILL = U.spillover(3, 4)[0]
SPILLOVER = {"channels": ["CD4", "CD3", "CD19"], "matrix": SPILL.tolist()}


def test_read_timepoint_without_and_with_a_sidecar(tmp_path):
    X = dyadic(50, 5, 1)
    fn = str(tmp_path / "t0.csv")
    write_csv(fn, X)
    plain = read_timepoint(fn)
    assert isinstance(plain, np.ndarray) and plain.flags["F_CONTIGUOUS"] and np.array_equal(plain, X)
    sidecar(fn, {"compensate": False})  # (asks for nothing)
    assert isinstance(read_timepoint(fn), np.ndarray)
    sidecar(fn, {"compensate": True, "spillover": SPILLOVER, "cofactor": {"CD3": 5, "CD8": 150},
                 "logicle": {"CD19": {"T": 262144, "W": 0.5}}})
    tp = read_timepoint(fn)
    assert isinstance(tp, _lib.TransformedPoints) and tp.shape == (50, 5)
    assert tp.points is tp.array and tp.array.flags["F_CONTIGUOUS"], "the parsed CSV is read where it lies"
    t = tp.transform
    assert t.comp_cols.tolist() == [2, 1, 4]
    U.same_bits(t.comp, np.ascontiguousarray(np.linalg.inv(SPILL)), "the inverse read_fcs would take")
    assert t.cofactor.tolist() == [0.0, 5.0, 0.0, 150.0, 0.0]
    assert t.logicle.tolist() == [[0.0] * 4] * 4 + [[262144.0, 0.5, 4.5, 0.0]]
    exp = np.asarray(_lib.ListMode(np.ascontiguousarray(X), 50, 5, np.float64, transform=t))
    U.same_bits(np.asarray(tp), exp, "the host transform of a CSV timepoint")
    # a .npy timepoint takes its names from <file>.columns
    npy = str(tmp_path / "t0.npy")
    np.save(npy, X.astype(np.float32))
    assert read_timepoint(npy).dtype == np.float32
    sidecar(npy, {"cofactor": 5})
    with pytest.raises(ValueError, match=r"\.columns"):
        read_timepoint(npy)
    with open(npy + ".columns", "w") as f:
        f.write("\n".join(NAMES) + "\n")
    tq = read_timepoint(npy)
    assert isinstance(tq, _lib.TransformedPoints) and tq.points.dtype == np.float32 and tq.transform.m == 0
    sidecar(npy, {"compensate": True, "spillover": SPILLOVER})
    assert read_timepoint(npy).transform.comp_cols.tolist() == [2, 1, 4]


@pytest.mark.parametrize("spec,message", [
    ({"compensate": True}, '"compensate" needs "spillover"'),
    ({"compensate": True, "spillover": {"channels": ["CD3", "CD4"], "matrix": [[1, 0.1], [0.1]]}}, "not square"),
    ({"compensate": True, "spillover": {"channels": ["CD3", "CD4"], "matrix": [[1, 0.1, 0], [0.1, 1, 0]]}}, "not square"),
    ({"compensate": True, "spillover": {"channels": ["CD3", "CD4"], "matrix": [[1, 0.1]]}}, "not square"),
    ({"compensate": True, "spillover": {"channels": ["CD3", "CD4"], "matrix": [[1, float("nan")], [0.1, 1]]}}, "not finite"),
    ({"compensate": True, "spillover": {"channels": ["CD3", "CD4"], "matrix": [[1, float("inf")], [0.1, 1]]}}, "not finite"),
    ({"compensate": True, "spillover": {"channels": ["CD3", "CD4"], "matrix": [[1, "x"], [0.1, 1]]}}, "no number"),
    ({"compensate": True, "spillover": {"channels": ["CD3", "CD3"], "matrix": [[1, 0], [0, 1]]}}, "twice"),
    ({"compensate": True, "spillover": {"channels": ["CD3", "CD4"], "matrix": [[1, 1], [1, 1]]}}, "singular"),
    ({"compensate": True, "spillover": {"channels": ["CD3", "CD5"], "matrix": [[1, 0], [0, 1]]}}, "names channel 'CD5', which is no column"),
    ({"compensate": True, "spillover": {"names": ["CD3"], "matrix": [[1]]}}, '"spillover" must be'),
    ({"cofactor": {"CD5": 5}}, "cofactor names 'CD5'"),
    ({"logicle": {"CD5": {"T": 1000}}}, "logicle names 'CD5'"),
    ({"logicle": {"CD3": {"W": 0.5}}}, 'channel CD3 needs "T"'),
    ({"logicle": {"W": 0.5}}, 'channel FSC-A needs "T"'),
    ({"logicle": {"CD3": {"T": 1000, "W": "estimate"}}}, r'channel CD3 has "W": "estimate".*not for \.csv or \.npy'),
    ({"cofactor": {"CD3": 5}, "logicle": {"CD3": {"T": 1000}}}, "CD3 has a cofactor and a logicle scale"),
    ({"spill": True}, "expected"),
])
def test_sidecar_refusals_beside_a_csv(tmp_path, spec, message):
    fn = str(tmp_path / "t0.csv")
    write_csv(fn, dyadic(4, 5, 1))
    sidecar(fn, spec)
    with pytest.raises(ValueError, match=message):
        read_timepoint(fn)


def test_spillover_beside_an_fcs_file_is_refused(tmp_path):
    import fcs_util as F
    rec = U.records(np.float32, 10, 5, 1)
    fn = str(tmp_path / "t0.fcs")
    F.write_fcs(fn, F.fast_records(rec, U.LITTLE), 5, "F", U.LITTLE, 32, names=NAMES, tot=10)
    sidecar(fn, {"compensate": True, "spillover": SPILLOVER})
    for call in (lambda: fcs.sidecar_transform(fn), lambda: read_timepoint(fn)):
        with pytest.raises(ValueError, match='"spillover" is for .csv and .npy timepoints'):
            call()
    # and an .fcs sidecar without the key reads as ever
    sidecar(fn, {"cofactor": 5})
    assert fcs.sidecar_transform(fn) == dict(compensate=False, cofactor=5)
    lm = read_timepoint(fn)
    assert isinstance(lm, _lib.ListMode) and lm.transform is not None
