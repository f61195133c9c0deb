"""FCS files without a GPU: chronoclust_amd.fcs.read_fcs on files written byte by byte (fcs_util: no code shared with the
parser), the host decode of _lib.ListMode, the layouts that fall back to the host, every refusal with its keyword, the
layout of cc_list_mode against the header, and read_timepoint / get_dataset_attributes with and without the sidecar."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fcs_util as F
from chronoclust_amd import _lib
from chronoclust_amd.fcs import parse_text, range_mask, read_fcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chronoclust_hip.h")
LIST_SYMBOLS = ("cc_points_upload_list", "cc_points_prefetch_list", "cc_col_minmax_list", "cc_online_list", "cc_assign_list",
                "cc_list_points")
LITTLE, BIG = (1, 2, 3, 4), (4, 3, 2, 1)
NAMES = ["Time", "FSC-A", "CD3", "CD4", "CD8"]
STAINS = ["", "", "Pacific Blue", "FITC", "PE"]


def float_table(dtype, n=7, par=5, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1000.0, 1000.0, (n, par)).astype(dtype)
    x[0, 0], x[n - 1, par - 1], x[1, 2] = 0.0, -0.0, np.finfo(dtype).max
    return x


def int_table(bits, n=7, par=5, seed=0):
    rng = np.random.default_rng(seed + bits)
    x = rng.integers(0, 1 << bits, (n, par), dtype=np.uint64)
    x[0, 0], x[n - 1, par - 1] = 0, (1 << bits) - 1
    return x


def same_values(got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    assert got.tobytes() == np.ascontiguousarray(exp).tobytes()


# ---- header and bindings ------------------------------------------------------------------------------------------------------

def test_the_header_declares_the_list_mode_and_its_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+cc_list_mode\s*\{", text)
    for name in LIST_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.SYMBOLS, name
    assert "list_points" not in [f for f, _ in _lib.CcStats._fields_]  # (cc_stats keeps its layout: a counter of its own)


def test_the_ctypes_list_mode_matches_the_header_layout(tmp_path):
    fields = [f for f, _ in _lib.CcListMode._fields_]
    assert fields == ["data", "n", "src_cols", "dtype", "flags", "d", "cols", "masks"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "chronoclust_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(cc_list_mode));']
    for f in fields:
        lines.append('printf("%s %%zu\\n", offsetof(cc_list_mode, %s));' % (f, f))
    lines += ['printf("SWAPPED %d\\n", (int)CC_LM_SWAPPED);', 'printf("MAX_SRC_COLS %d\\n", (int)CC_MAX_SRC_COLS);']
    for name in ("F64", "F32", "U8", "U16", "U32"):
        lines.append('printf("DT_%s %%d\\n", (int)CC_DT_%s);' % (name, name))
    lines += ['return 0;', '}']
    src, exe = tmp_path / "lm.c", tmp_path / "lm"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_lib.CcListMode)
    for f in fields:
        assert int(out[f]) == getattr(_lib.CcListMode, f).offset, f
    assert int(out["SWAPPED"]) == _lib.LM_SWAPPED and int(out["MAX_SRC_COLS"]) == _lib.MAX_SRC_COLS
    for name in ("F64", "F32", "U8", "U16", "U32"):
        assert int(out["DT_" + name]) == getattr(_lib, "DT_" + name), name
    assert sorted(_lib.LIST_DTYPES.values()) == sorted(getattr(_lib, "DT_" + n) for n in ("F64", "F32", "U8", "U16", "U32"))


# ---- the writer against itself --------------------------------------------------------------------------------------------------

def test_the_two_record_writers_agree():
    for dtype in (np.float32, np.float64):
        x = float_table(dtype)
        x[2, 1] = np.nan
        for order in (LITTLE, BIG):
            assert F.fast_records(x, order) == F.float_records(x, order)
            assert F.float_records(x, order) == F.records(x.tolist(), "f", x.dtype.itemsize, order) or np.isnan(x).any()
    x = int_table(16).astype(np.uint16)
    assert F.fast_records(x, BIG) == F.records(x.tolist(), "u", 2, BIG)
    assert F.element_bytes(0x01020304, "u", 4, BIG) == b"\x01\x02\x03\x04"
    assert F.element_bytes(0x01020304, "u", 4, LITTLE) == b"\x04\x03\x02\x01"
    assert F.element_bytes(0x01020304, "u", 4, (3, 4, 1, 2)) == b"\x02\x01\x04\x03"
    assert F.element_bytes(1.0, "f", 4, BIG) == b"\x3f\x80\x00\x00"


# ---- the parser: what goes to the device as it lies ------------------------------------------------------------------------------

@pytest.mark.parametrize("version", ["FCS2.0", "FCS3.0", "FCS3.1"])
@pytest.mark.parametrize("order", [LITTLE, BIG], ids=["little", "big"])
def test_float_files(tmp_path, version, order):
    for datatype, dtype, bits in (("F", np.float32, 32), ("D", np.float64, 64)):
        x = float_table(dtype)
        fn = F.write_fcs(tmp_path / ("x%s.fcs" % datatype), F.records(x.tolist(), "f", bits // 8, order), 5, datatype, order, bits,
                         names=NAMES, stains=STAINS, tot=7, version=version)
        pts, names, text = read_fcs(fn)
        assert isinstance(pts, _lib.ListMode) and pts.shape == (7, 5) and pts.ndim == 2 and len(pts) == 7
        assert pts.dtype == np.dtype(dtype).newbyteorder("<" if order == LITTLE else ">")
        assert pts.swapped == (order == BIG) and pts.masks is None and pts.src_cols == 5
        assert names == NAMES and text["$DATATYPE"] == datatype and text["$P3S"] == "Pacific Blue"
        same_values(pts, x)  # (float32 sources decode to float32, float64 to float64)
        assert np.asarray(pts).dtype == dtype
        desc = pts.descriptor()
        assert (desc.n, desc.src_cols, desc.d, desc.flags) == (7, 5, 5, _lib.LM_SWAPPED if order == BIG else 0)
        assert desc.dtype == (_lib.DT_F32 if datatype == "F" else _lib.DT_F64) and not desc.masks
        assert [desc.cols[i] for i in range(5)] == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("bits", [8, 16, 32])
@pytest.mark.parametrize("order", [LITTLE, BIG], ids=["little", "big"])
def test_integer_files_and_their_range_masks(tmp_path, bits, order):
    x = int_table(bits)
    data = F.records(x.tolist(), "u", bits // 8, order)
    # no mask at all: $PnR = 2^bits
    pts = read_fcs(F.write_fcs(tmp_path / "full.fcs", data, 5, "I", order, bits, tot=7))[0]
    assert isinstance(pts, _lib.ListMode) and pts.masks is None and pts.dtype.itemsize == bits // 8 and pts.dtype.kind == "u"
    assert np.asarray(pts).dtype == np.float64
    same_values(pts, x.astype(np.float64))
    # $PnR below the width: the stored values keep their high bits, the decode drops them
    ranges = [1 << bits, 1 << (bits - 2), (1 << (bits - 2)) - 24, 1 << (bits - 1), 2]
    pts = read_fcs(F.write_fcs(tmp_path / "masked.fcs", data, 5, "I", order, bits, ranges=ranges, tot=7))[0]
    exp_masks = [0xFFFFFFFF, (1 << (bits - 2)) - 1, (1 << (bits - 2)) - 1, (1 << (bits - 1)) - 1, 1]
    assert pts.masks.dtype == np.uint32 and pts.masks.tolist() == exp_masks
    exp = np.stack([x[:, c] & np.uint64(m) for c, m in enumerate(exp_masks)], axis=1)
    assert (exp != x).any()
    same_values(pts, exp.astype(np.float64))


def test_range_masks_by_example():
    assert range_mask(1024, 16) == 0x3FF and range_mask(1000, 16) == 0x3FF and range_mask(1025, 16) == 0x7FF
    assert range_mask(65536, 16) is None and range_mask(70000, 16) is None and range_mask(256, 8) is None
    assert range_mask(262144, 32) == 0x3FFFF and range_mask(1 << 32, 32) is None and range_mask(1, 8) == 0 and range_mask(2, 8) == 1


def test_text_segment_details(tmp_path):
    x = float_table(np.float32)
    data = F.records(x.tolist(), "f", 4, BIG)
    # a delimiter doubled inside a value, lower-case keywords, another delimiter
    fn = F.write_fcs(tmp_path / "a.fcs", data, 5, "F", BIG, 32, names=["a/b", "c", "d", "e", "f"], tot=7, lower_keywords=True,
                     extra={"$CYT": "LSR//II", "NOTE": "x/y/z"})
    pts, names, text = read_fcs(fn)
    assert names[0] == "a/b" and text["$CYT"] == "LSR//II" and text["NOTE"] == "x/y/z" and "$TOT" in text
    same_values(pts, x)
    fn = F.write_fcs(tmp_path / "b.fcs", data, 5, "F", BIG, 32, names=NAMES, tot=7, delimiter="|", extra={"K": "1|2"})
    assert read_fcs(fn)[2]["K"] == "1|2"
    assert parse_text(b"/A/1/b/x//y/") == {"A": "1", "B": "x/y"}
    # DATA offsets from TEXT when the header's are zero; an odd DATA offset; trailing bytes; $TOT absent
    for kw in (dict(text_data_offsets=True, tot=7), dict(pad_before_data=1, tot=7), dict(pad_before_data=2, tot=7),
               dict(trailing=b"\x00" * 9 + b"CRC", tot=7), dict(tot=None), dict(tot=None, version="FCS2.0", text_data_offsets=True)):
        blob = F.fcs_bytes(data, 5, "F", BIG, 32, names=NAMES, **kw)
        fn = str(tmp_path / "c.fcs")
        open(fn, "wb").write(blob)
        pts, names, text = read_fcs(fn)
        assert pts.shape == (7, 5) and pts._bytes.tobytes() == data  # (the segment itself, wherever it starts)
        same_values(pts, x)
        if kw.get("text_data_offsets"):
            assert blob[10 + 16:10 + 32].split() == [b"0", b"0"] and int(text["$BEGINDATA"]) == blob.index(data)
    odd = [F.fcs_bytes(data, 5, "F", BIG, 32, names=NAMES, tot=7, pad_before_data=p).index(data) % 2 for p in (1, 2)]
    assert sorted(odd) == [0, 1]  # (one of the two starts at an odd byte)
    # $TOT below what the segment holds: the first $TOT events
    fn = F.write_fcs(tmp_path / "d.fcs", data, 5, "F", BIG, 32, names=NAMES, tot=4)
    same_values(read_fcs(fn)[0], x[:4])


def test_column_selection(tmp_path):
    x = int_table(16).astype(np.uint16)
    ranges = [65536, 65536, 1024, 4096, 65536]
    fn = F.write_fcs(tmp_path / "s.fcs", F.records(x.tolist(), "u", 2, BIG), 5, "I", BIG, 16, ranges=ranges, names=NAMES, stains=STAINS, tot=7)
    wide = np.stack([x[:, c] & m for c, m in enumerate([0xFFFF, 0xFFFF, 0x3FF, 0xFFF, 0xFFFF])], axis=1).astype(np.float64)
    for columns, idx in ((["CD8", "CD3"], [4, 2]), (["PE", "FITC", "Time"], [4, 3, 0]), ([3, 1, 3], [3, 1, 3]), (["CD4", 0, "PE"], [3, 0, 4])):
        pts, names, _ = read_fcs(fn, columns=columns)
        assert pts.columns.tolist() == idx and names == [NAMES[i] for i in idx] and pts.shape == (7, len(idx)) and pts.src_cols == 5
        same_values(pts, wide[:, idx])
        got = pts.masks.tolist()
        assert got == [[0xFFFFFFFF, 0xFFFFFFFF, 0x3FF, 0xFFF, 0xFFFFFFFF][i] for i in idx]
    assert read_fcs(fn, columns=["Time", "FSC-A"])[0].masks is None  # (no selected channel has a range below its width)
    for bad in (["CD19"], [5], [-1], []):
        with pytest.raises(ValueError, match="column|channel"):
            read_fcs(fn, columns=bad)


# ---- ListMode by itself ----------------------------------------------------------------------------------------------------------

def test_list_mode_decodes_what_the_writer_encoded():
    for dtype, code in ((">f4", np.float32), ("<f4", np.float32), (">f8", np.float64), ("<u2", np.uint16), (">u4", np.uint32), ("|u1", np.uint8)):
        dt = np.dtype(dtype)
        x = (float_table(code, 9, 6) if dt.kind == "f" else int_table(8 * dt.itemsize, 9, 6).astype(code))
        order = BIG if dt.byteorder == ">" else LITTLE
        blob = F.fast_records(x, order)
        for buf in (blob, bytearray(blob), F.unaligned(blob), memoryview(blob)):
            lm = _lib.ListMode(buf, 9, 6, dt, columns=[5, 0, 0, 2])
            assert lm.shape == (9, 4) and lm.swapped == (dt.byteorder == ">")
            same_values(lm, x[:, [5, 0, 0, 2]].astype(np.float32 if dtype.endswith("f4") else np.float64))
        if dt.kind == "u":
            lm = _lib.ListMode(blob, 9, 6, dt, columns=[1, 3], masks=[0x0F, 0xFFFFFFFF])
            same_values(lm, np.stack([x[:, 1] & 0x0F, x[:, 3]], axis=1).astype(np.float64))
    for args, kw in (((b"\0" * 7, 1, 2, "<f4"), {}), ((b"\0" * 8, 1, 2, "<i4"), {}), ((b"\0" * 8, 1, 2, "<f4"), dict(columns=[2])),
                     ((b"\0" * 8, 1, 2, "<f4"), dict(masks=[1, 1])), ((b"\0" * 8, 1, 2, "<u4"), dict(masks=[1])),
                     ((b"\0" * 8, -1, 2, "<f4"), {}), ((b"\0" * 8, 1, 2, "<f2"), {})):
        with pytest.raises(ValueError, match="ListMode"):
            _lib.ListMode(*args, **kw)
    # points_source is not asked and does not know the class
    assert "ListMode" not in (_lib.points_source.__doc__ + _lib.points_view.__doc__ + _lib.as_points.__doc__)


# ---- the host fallbacks ----------------------------------------------------------------------------------------------------------

def test_layouts_that_are_decoded_on_the_host(tmp_path):
    # mixed $PnB
    widths = [8, 16, 32, 16, 64]
    x = np.stack([int_table(w, seed=c)[:, 0] for c, w in enumerate(widths)], axis=1)
    x[3, 4] = (1 << 53) + 2  # (a 64-bit value that float64 holds)
    for order in (LITTLE, BIG):
        fn = F.write_fcs(tmp_path / "mixed.fcs", F.records(x.tolist(), "u", [w // 8 for w in widths], order), 5, "I", order, widths, tot=7,
                         ranges=[256, 1024, 1 << 32, 65536, 1 << 64], names=NAMES)
        pts, names, _ = read_fcs(fn, columns=["CD8", "FSC-A", "Time"])
        assert isinstance(pts, np.ndarray) and pts.dtype == np.float64 and pts.flags["C_CONTIGUOUS"] and names == ["CD8", "FSC-A", "Time"]
        exp = np.stack([x[:, 4], x[:, 1] & np.uint64(0x3FF), x[:, 0]], axis=1).astype(np.float64)
        same_values(pts, exp)
    # an odd width: 24 bits; 64-bit integers
    for bits in (24, 64):
        x = int_table(min(bits, 53))
        fn = F.write_fcs(tmp_path / "odd.fcs", F.records(x.tolist(), "u", bits // 8, BIG), 5, "I", BIG, bits, tot=7)
        pts = read_fcs(fn)[0]
        assert isinstance(pts, np.ndarray)
        same_values(pts, x.astype(np.float64))
    # mixed byte orders
    x = float_table(np.float32)
    fn = F.write_fcs(tmp_path / "pdp.fcs", F.records(x.tolist(), "f", 4, (3, 4, 1, 2)), 5, "F", (3, 4, 1, 2), 32, tot=7)
    pts = read_fcs(fn)[0]
    assert isinstance(pts, np.ndarray) and pts.dtype == np.float64
    same_values(pts, x.astype(np.float64))
    xi = int_table(32)
    fn = F.write_fcs(tmp_path / "pdpi.fcs", F.records(xi.tolist(), "u", 4, (2, 1, 4, 3)), 5, "I", (2, 1, 4, 3), 32, tot=7, ranges=1 << 20)
    same_values(read_fcs(fn)[0], (xi & np.uint64((1 << 20) - 1)).astype(np.float64))
    # 16-bit integers under a four-byte $BYTEORD: the order's direction
    x16 = int_table(16)
    fn = F.write_fcs(tmp_path / "w16.fcs", F.records(x16.tolist(), "u", 2, BIG), 5, "I", BIG, 16, tot=7)
    pts = read_fcs(fn)[0]
    assert isinstance(pts, _lib.ListMode) and pts.dtype == np.dtype(">u2")
    same_values(pts, x16.astype(np.float64))


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_keyword(tmp_path):
    x = float_table(np.float32)
    data = F.records(x.tolist(), "f", 4, LITTLE)
    good = dict(data=data, par=5, datatype="F", order=LITTLE, bits=32, tot=7)

    def written(**over):
        kw = dict(good, **over)
        fn = str(tmp_path / "r.fcs")
        open(fn, "wb").write(F.fcs_bytes(kw.pop("data"), kw.pop("par"), kw.pop("datatype"), kw.pop("order"), kw.pop("bits"), **kw))
        return fn

    same_values(read_fcs(written())[0], x)
    for over, keyword in ((dict(datatype="A"), r"\$DATATYPE"), (dict(mode="H"), r"\$MODE"), (dict(mode="C"), r"\$MODE"),
                          (dict(tot=8), r"\$TOT"), (dict(data=data[:-1], tot=7), r"\$TOT"), (dict(bits=16), r"\$P1B"),
                          (dict(datatype="I", bits=12), r"\$P1B"), (dict(omit=("$PAR",)), r"\$PAR"), (dict(omit=("$BYTEORD",)), r"\$BYTEORD"),
                          (dict(omit=("$DATATYPE",)), r"\$DATATYPE"), (dict(omit=("$MODE",)), r"\$MODE"), (dict(omit=("$P3B",)), r"\$P3B"),
                          (dict(order=(1, 2, 4, 4)), r"\$BYTEORD"), (dict(datatype="I", order=(3, 4, 1, 2), bits=16), r"\$BYTEORD"),
                          (dict(datatype="I", bits=16, data=data[:70], omit=("$P2R",)), r"\$P2R"),
                          (dict(extra={"$PAR": "five"}), r"\$PAR")):
        with pytest.raises(ValueError, match=keyword):
            read_fcs(written(**over))
    blob = F.fcs_bytes(**{k: v for k, v in good.items()})
    for mangled, what in ((b"FCS4.0" + blob[6:], "HEADER"), (blob[:40], "HEADER"), (blob[:10] + b"     abc" + blob[18:], "HEADER"),
                          (blob[:18] + b"%8d" % (len(blob) + 5) + blob[26:], "HEADER"),
                          (blob[:26] + b"%8d" % (len(blob) - 3) + b"%8d" % (len(blob) + 9) + blob[42:], "HEADER"),
                          (blob[:58] + b"/$MODE/L/$PAR/" + b" " * (len(blob) - 72), "TEXT")):
        fn = str(tmp_path / "m.fcs")
        open(fn, "wb").write(mangled)
        with pytest.raises(ValueError, match=what):
            read_fcs(fn)


# ---- read_timepoint and get_dataset_attributes -------------------------------------------------------------------------------------

class StubHandle(object):
    def __init__(self):
        self.calls = []

    def col_minmax(self, x):
        self.calls.append(x)
        return np.nanmin(np.asarray(x, np.float64), axis=0), np.nanmax(np.asarray(x, np.float64), axis=0)


def test_read_timepoint_and_dataset_attributes(tmp_path):
    from chronoclust_amd.app import get_dataset_attributes
    from chronoclust_amd.scaling.scaler import Scaler, read_timepoint
    x = float_table(np.float64, 11)
    x[:, 0] = np.nan  # (the Time channel: never selected below)
    fn = F.write_fcs(tmp_path / "tp0.fcs", F.float_records(x, BIG), 5, "D", BIG, 64, names=NAMES, stains=STAINS, tot=11)
    pts = read_timepoint(fn)
    assert isinstance(pts, _lib.ListMode) and pts.shape == (11, 5)
    assert get_dataset_attributes(fn) == NAMES
    with open(fn + ".columns", "w") as f:
        f.write("CD8\nPacific Blue\n\nFSC-A\n")
    pts = read_timepoint(fn)
    assert isinstance(pts, _lib.ListMode) and pts.columns.tolist() == [4, 2, 1]
    same_values(pts, x[:, [4, 2, 1]])
    assert get_dataset_attributes(fn) == ["CD8", "Pacific Blue", "FSC-A"]  # (as the sidecar names them)
    # the scaler's fit reduces the ListMode itself and keeps it for the run; without a handle it decodes on the host
    stub = StubHandle()
    sc = Scaler([fn], handle=stub)
    assert len(stub.calls) == 1 and isinstance(stub.calls[0], _lib.ListMode) and sc.parsed[fn] is stub.calls[0]
    ref = Scaler()
    ref.fit_scaler(x[:, [4, 2, 1]])
    assert sc.scale_.tobytes() == ref.scale_.tobytes() and sc.min_.tobytes() == ref.min_.tobytes()
    host = Scaler([fn])
    assert host.scale_.tobytes() == ref.scale_.tobytes() and host.min_.tobytes() == ref.min_.tobytes()
    # a layout of old through read_timepoint: a float64 array
    xi = int_table(24, 11)
    fn2 = F.write_fcs(tmp_path / "tp1.FCS", F.records(xi.tolist(), "u", 3, BIG), 5, "I", BIG, 24, names=NAMES, tot=11)
    got = read_timepoint(fn2)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    same_values(got, xi.astype(np.float64))
