"""Single-precision points, the part that needs no device: the eight entry points are declared, exported and bound; cc_stats
keeps its layout (the counter of single-precision points is cc_f32_points, which Handle.stats() adds); read_timepoint keeps a float32 `.npy` as it is; the dispatch helper of the binding hands a C-contiguous
float32 [n, d] array on as the very object and widens everything else on the host, as ever; the host-side Scaler fits the
same scale_ / min_ on float32 files as on their widened copies."""
import ctypes
import os
import re
import subprocess

import numpy as np

from chronoclust_amd import _lib, build
from chronoclust_amd.scaling.scaler import Scaler, read_timepoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chronoclust_hip.h")
NEW = ("cc_points_upload_f32", "cc_points_upload_scaled_f32", "cc_points_prefetch_f32", "cc_col_minmax_f32", "cc_online_f32",
       "cc_assign_f32", "cc_points_download_xt", "cc_f32_points")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_the_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), "the header does not declare %s" % name
        assert hasattr(lib, name), "the library does not export %s" % name
        assert name in _lib.SYMBOLS, "_lib.SYMBOLS does not bind %s" % name
    # the points of every `_f32` taker are const float*, everything else is what the float64 sibling takes
    for name in NEW[:-2]:
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, text)
        sib = re.search(r"\bint %s\s*\(([^)]*)\)" % name[:-len("_f32")], text)
        assert re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", sib.group(1)).replace("const double* x", "const float* x"), name
        assert _lib.SYMBOLS[name][1][1] is _lib._fp and _lib.SYMBOLS[name[:-len("_f32")]][1][1] is _lib._dp
        assert _lib.SYMBOLS[name][1][2:] == _lib.SYMBOLS[name[:-len("_f32")]][1][2:], name


def test_cc_stats_matches_the_header_and_the_counter_is_an_entry_point_of_its_own(tmp_path):
    """CcStats mirrors cc_stats as it was - size and the offset of its last field -, and the points taken in single precision
    are counted by cc_f32_points(handle, int64_t*), which Handle.stats() reports as "f32_points"."""
    last = _lib.CcStats._fields_[-1][0]
    src = tmp_path / "stats.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chronoclust_hip.h"\nint main(void) {\n'
                   'printf("%%zu %%zu\\n", sizeof(cc_stats), offsetof(cc_stats, %s));\nreturn 0;\n}\n' % last)
    exe = tmp_path / "stats"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    size, off = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == ctypes.sizeof(_lib.CcStats) and off == getattr(_lib.CcStats, last).offset == size - 8
    assert "f32_points" not in [k for k, _ in _lib.CcStats._fields_]
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint cc_f32_points\s*\(\s*cc_handle\*\s*h,\s*int64_t\*\s*out\s*\)\s*;", text)
    assert _lib.SYMBOLS["cc_f32_points"] == (ctypes.c_int, [ctypes.c_void_p, _lib._i64p])
    assert callable(_lib.Handle.f32_points)


def test_read_timepoint_keeps_float32_and_nothing_else(tmp_path):
    rng = np.random.default_rng(1)
    x = rng.normal(size=(37, 5))
    cases = {"f32": x.astype(np.float32), "f64": x, "f16": x.astype(np.float16), "i32": (x * 100).astype(np.int32),
             "f32_fortran": np.asfortranarray(x.astype(np.float32))}
    for name, a in cases.items():
        path = str(tmp_path / (name + ".npy"))
        np.save(path, a)
        got = read_timepoint(path)
        assert got.dtype == (np.float32 if name.startswith("f32") else np.float64), name
        assert got.flags["C_CONTIGUOUS"] and np.array_equal(_bits(got), _bits(a)), name
    import pandas as pd
    path = str(tmp_path / "t.csv")
    pd.DataFrame(x.astype(np.float32), columns=list("abcde")).to_csv(path, index=False)
    assert read_timepoint(path).dtype == np.float64


def test_dispatch_returns_the_very_object_or_a_float64_copy():
    rng = np.random.default_rng(2)
    x32 = np.ascontiguousarray(rng.normal(size=(20, 6)).astype(np.float32))
    assert _lib.as_points(x32) is x32 and _lib.is_f32_points(x32)
    rows = x32[3:9]
    assert _lib.as_points(rows) is rows  # (a range of rows is C-contiguous: taken as it is)
    others = {"fortran": np.asfortranarray(x32), "strided rows": x32[::2], "strided columns": x32[:, 1:4],
              "float16": x32.astype(np.float16), "int32": (x32 * 10).astype(np.int32), "float64": x32.astype(np.float64),
              "list": x32.tolist()}
    for name, a in others.items():
        got = _lib.as_points(a)
        assert not _lib.is_f32_points(a), name
        assert got.dtype == np.float64 and got.flags["C_CONTIGUOUS"] and got.ndim == 2, name
        assert np.array_equal(got.view(np.int64), _bits(np.asarray(a, dtype=np.float64))), name
        if isinstance(a, np.ndarray) and a.dtype != np.float64:
            assert not np.shares_memory(got, a), name
    assert not _lib.is_f32_points(x32[0]) and not _lib.is_f32_points(x32.reshape(2, 10, 6))
    x64 = np.ascontiguousarray(x32, dtype=np.float64)
    assert _lib.as_points(x64) is x64  # (np.ascontiguousarray of what already is one: no copy, as before)


def test_xt_rows_is_the_padded_scan_width():
    assert [_lib.xt_rows(d) for d in (1, 8, 9, 13, 14, 15, 20, 33, 63, 64, 65, 1024)] == [1, 8, 14, 14, 14, 16, 20, 40, 64, 64, 65, 1024]


def test_host_scaler_fits_the_same_on_float32_files(tmp_path):
    rng = np.random.default_rng(3)
    files32, files64 = [], []
    for t in range(3):
        x = (rng.normal(size=(50 + t, 4)) * [1.0, 50.0, 1e-3, 7.0]).astype(np.float32)
        x[t, 2] = np.nan  # (np.nanmin / np.nanmax ignore it)
        for kind, files in ((np.float32, files32), (np.float64, files64)):
            path = str(tmp_path / ("t%d_%s.npy" % (t, np.dtype(kind).name)))
            np.save(path, x.astype(kind))
            files.append(path)
    a, b = Scaler(files32), Scaler(files64)
    for key in ("scale_", "min_", "data_min_", "data_max_"):
        assert getattr(a, key).dtype == np.float64
        assert np.array_equal(_bits(getattr(a, key)), _bits(getattr(b, key))), key
    x32 = read_timepoint(files32[0])
    assert np.array_equal(_bits(a.scale_data(x32)), _bits(b.scale_data(x32.astype(np.float64))))
