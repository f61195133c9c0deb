"""Point views without a GPU: the header declares cc_points_view and its six entry points and the ctypes mirror matches it;
_lib.points_source sorts arrays into the three ways the library takes points; a parsed CSV is accepted in the columns form
and Scaler(handle=...) keeps that very array."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from chronoclust_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chronoclust_hip.h")
VIEW_SYMBOLS = ("cc_points_upload_view", "cc_points_prefetch_view", "cc_col_minmax_view", "cc_online_view", "cc_assign_view",
                "cc_view_points")


# ---- header and bindings --------------------------------------------------------------------------------------------------

def test_the_header_declares_the_view_and_its_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+cc_points_view\s*\{", text)
    for name in VIEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.SYMBOLS, name
    assert "view_points" not in [f for f, _ in _lib.CcStats._fields_]  # (cc_stats keeps its layout: a counter of its own)


def test_the_ctypes_view_matches_the_header_layout(tmp_path):
    fields = [f for f, _ in _lib.CcPointsView._fields_]
    assert fields == ["data", "n", "d", "dtype", "row_stride", "col_stride"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "chronoclust_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(cc_points_view));']
    for f in fields:
        lines.append('printf("%s %%zu\\n", offsetof(cc_points_view, %s));' % (f, f))
    for name in ("F64", "F32", "F16", "I8", "U8", "I16", "U16", "I32", "U32"):
        lines.append('printf("DT_%s %%d\\n", (int)CC_DT_%s);' % (name, name))
    lines += ['return 0;', '}']
    src, exe = tmp_path / "view.c", tmp_path / "view"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_lib.CcPointsView)
    for f in fields:
        assert int(out[f]) == getattr(_lib.CcPointsView, f).offset, f
    for name in ("F64", "F32", "F16", "I8", "U8", "I16", "U16", "I32", "U32"):
        assert int(out["DT_" + name]) == getattr(_lib, "DT_" + name), name


# ---- points_source ----------------------------------------------------------------------------------------------------------

A = np.arange(60 * 9, dtype=np.float64).reshape(60, 9) / 7.0
AF = np.asfortranarray(A)
B = np.ascontiguousarray(A.T)  # [d, N]
DTYPES = {np.float64: _lib.DT_F64, np.float32: _lib.DT_F32, np.float16: _lib.DT_F16, np.int8: _lib.DT_I8, np.uint8: _lib.DT_U8,
          np.int16: _lib.DT_I16, np.uint16: _lib.DT_U16, np.int32: _lib.DT_I32, np.uint32: _lib.DT_U32}

# (name, array, expectation): "plain" the array itself for the entry points of old; (dtype code, row stride, column stride)
# the array itself and its descriptor; "copy" the float64 fallback
TABLE = [
    ("C float64", A, "plain"),
    ("C float32", A.astype(np.float32), "plain"),
    ("Fortran float64", AF, (_lib.DT_F64, 1, 60)),
    ("Fortran float32", np.asfortranarray(A.astype(np.float32)), (_lib.DT_F32, 1, 60)),
    ("columns 2:7", A[:, 2:7], (_lib.DT_F64, 9, 1)),
    ("every other row", A[::2], (_lib.DT_F64, 18, 1)),
    ("rows 5:40 of Fortran", AF[5:40], (_lib.DT_F64, 1, 60)),
    ("transpose of [d, N]", B.T, (_lib.DT_F64, 1, 60)),
    ("every other column", A[:, ::2], "copy"),
    ("rows reversed", A[::-1], "copy"),
    ("broadcast row", np.broadcast_to(A[0], (60, 9)), "copy"),
    ("int64", (A * 7).astype(np.int64), "copy"),
    ("bool", A > 3, "copy"),
    ("big-endian float32", A.astype(">f4"), "copy"),
    ("a list", A[:3].tolist(), "copy"),
    ("no points", np.empty((0, 9)), "plain"),
    ("no points, uint16", np.empty((0, 9), np.uint16), "copy"),
    ("one point", A[:1], "plain"),
    ("one point of a Fortran array", AF[:1], (_lib.DT_F64, 1, 60)),
    ("one point, uint16", A[:1].astype(np.uint16), (_lib.DT_U16, 9, 1)),
    ("one dimension", A[:, :1].copy(), "plain"),
    ("one dimension of a C array", A[:, 3:4], (_lib.DT_F64, 9, 1)),
    ("one dimension of a Fortran array", AF[:, 3:4], "plain"),  # (one strip: C-contiguous too)
    ("one dimension of a Fortran uint8 array", np.asfortranarray(A.astype(np.uint8))[:, 3:4], (_lib.DT_U8, 1, 1)),
] + [("C %s" % np.dtype(t).name, (A * 3).astype(t), (code, 9, 1)) for t, code in DTYPES.items() if t not in (np.float64, np.float32)] \
  + [("Fortran %s" % np.dtype(t).name, np.asfortranarray((A * 3).astype(t)), (code, 1, 60)) for t, code in DTYPES.items()
     if t not in (np.float64, np.float32)]


@pytest.mark.parametrize("name,a,exp", TABLE, ids=[t[0] for t in TABLE])
def test_points_source(name, a, exp):
    got, view = _lib.points_source(a)
    if exp == "plain":
        assert got is a and view is None
        assert _lib.as_points(a) is a or a.dtype == np.float64  # (what the entry points of old take as it is)
    elif exp == "copy":
        assert view is None and got is not a
        assert got.dtype == np.float64 and got.flags["C_CONTIGUOUS"]
        wide = np.asarray(a, dtype=np.float64)
        assert got.shape == wide.shape and got.tobytes() == np.ascontiguousarray(wide).tobytes()
    else:
        assert got is a and isinstance(view, _lib.CcPointsView)
        assert (view.dtype, view.row_stride, view.col_stride) == exp
        assert (view.n, view.d) == a.shape and view.data == a.ctypes.data
        # the descriptor addresses the array's own elements
        flat = np.frombuffer((ctypes.c_char * (a.dtype.itemsize * (1 + (view.n - 1) * view.row_stride + (view.d - 1) * view.col_stride)))
                             .from_address(view.data), dtype=a.dtype)
        r, c = view.n - 1, view.d - 1
        assert flat[r * view.row_stride + c * view.col_stride] == a[r, c] and flat[0] == a[0, 0]
        # one of the two accepted layouts
        assert (view.col_stride == 1 and view.row_stride >= view.d) or (view.row_stride == 1 and view.col_stride >= view.n)


def test_as_points_is_what_it_was():
    for _, a, _ in TABLE:
        got = _lib.as_points(a)
        assert got is a or not _lib.is_f32_points(a)
        assert got.flags["C_CONTIGUOUS"] and got.dtype in (np.float32, np.float64)


# ---- CSV through the scaler ----------------------------------------------------------------------------------------------------

class StubHandle(object):
    """Records col_minmax calls and answers them with numpy."""

    def __init__(self):
        self.calls = []

    def col_minmax(self, x):
        self.calls.append(x)
        return np.nanmin(np.asarray(x, np.float64), axis=0), np.nanmax(np.asarray(x, np.float64), axis=0)


def test_a_parsed_csv_reaches_the_handle_as_it_is(tmp_path):
    import pandas as pd
    from chronoclust_amd.scaling.scaler import Scaler, read_timepoint
    rng = np.random.default_rng(3)
    files, arrays = [], []
    for t in range(2):
        x = rng.uniform(-2.0, 5.0, (40 + t, 6))
        fn = str(tmp_path / ("tp%d.csv" % t))
        pd.DataFrame(x, columns=list("abcdef")).to_csv(fn, index=False)
        files.append(fn)
        arrays.append(x)
    parsed = pd.read_csv(files[0]).to_numpy()
    assert parsed.dtype == np.float64 and parsed.flags["F_CONTIGUOUS"] and not parsed.flags["C_CONTIGUOUS"]
    got, view = _lib.points_source(parsed)
    assert got is parsed and (view.dtype, view.row_stride, view.col_stride) == (_lib.DT_F64, 1, 40)
    assert read_timepoint(files[0]).strides == parsed.strides  # (read_timepoint is what it was)

    stub = StubHandle()
    sc = Scaler(files, handle=stub)
    assert len(stub.calls) == 2
    for fn, call in zip(files, stub.calls):
        assert sc.parsed[fn] is call  # the very object the fit reduced is the one kept for the run
        assert not call.flags["C_CONTIGUOUS"] and _lib.points_source(call)[0] is call
    ref = Scaler()
    ref.fit_scaler(np.concatenate([pd.read_csv(fn).to_numpy() for fn in files]))
    assert sc.scale_.tobytes() == ref.scale_.tobytes() and sc.min_.tobytes() == ref.min_.tobytes()

    # what the library does not read where it lies is kept as before: a C-contiguous float64 copy (an integer CSV parses to int64)
    fn = str(tmp_path / "ints.csv")
    pd.DataFrame(np.arange(12).reshape(4, 3), columns=list("abc")).to_csv(fn, index=False)
    sc = Scaler([fn], handle=StubHandle())
    kept = sc.parsed[fn]
    assert kept.dtype == np.float64 and kept.flags["C_CONTIGUOUS"] and np.array_equal(kept, np.arange(12.0).reshape(4, 3))


def test_npy_timepoints_are_kept_as_before(tmp_path):
    from chronoclust_amd.scaling.scaler import Scaler
    x = np.random.default_rng(1).uniform(0, 1, (10, 4))
    files = []
    for kind in (np.float32, np.float64, np.uint16):
        fn = str(tmp_path / ("x_%s.npy" % np.dtype(kind).name))
        np.save(fn, (x * 100).astype(kind))
        files.append(fn)
    sc = Scaler(files, handle=StubHandle())
    assert [sc.parsed[fn].dtype for fn in files] == [np.float32, np.float64, np.float64]
    assert all(sc.parsed[fn].flags["C_CONTIGUOUS"] for fn in files)
