"""The host side of the logicle scale, no GPU: the referee of logicle_util proven against a 40-digit evaluation, the library's
coefficients (cc_logicle_coefficients) against the scale's defining identities, every refusal through cc_logicle_coefficients,
ListTransform and read_fcs, the layout of cc_list_logicle, the sidecar's forms, np.asarray(ListMode) against the referee, and the
host route of a mixed-width file.

The host fallback's distance from the referee, measured on the CPU over the sweep of logicle_util.sweep (|v| log-uniform per
three decades from 1e-6 to 2 T, 20 000 values per band, both signs, +-0, +-T, the smallest subnormal and 1e300) for the eight
parameter sets of logicle_util.P, in units of np.spacing(max(|y_ref|, 0.5)): the largest is 2.0 (sets 1-4 and 6: 2.0; set 5:
1.5; set 7: 1.19; set 8: 1.06).  HOST_MEASURED_MAX_UNITS is that figure; the bound of every comparison is one unit more, for the
referee's own rounding.  Three of the four Halley steps already reach it: what is left is the rounding of b u, of the last
subtraction and of x1 + u, not the iteration."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import fcs_util as F
import logicle_util as L
import transform_util as U
from chronoclust_amd import _lib, fcs

LITTLE, BIG = U.LITTLE, U.BIG
HOST_MEASURED_MAX_UNITS = 2.0
HOST_BOUND_UNITS = HOST_MEASURED_MAX_UNITS + 1.0
NAMES = ["Time", "FSC-A", "B515-A", "G560-A", "R660-A", "V450-A"]
FLUOR = ["G560-A", "B515-A", "V450-A"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_extended = pytest.mark.skipif(not L.EXTENDED, reason=L.NEEDS_EXTENDED)

# every refusal of the contract: (what, (T, W, M, A))
REFUSED = [("a NaN T", (np.nan, 0.5, 4.5, 0.0)), ("an infinite W", (262144.0, np.inf, 4.5, 0.0)), ("a NaN M", (262144.0, 0.5, np.nan, 0.0)),
           ("an infinite A", (262144.0, 0.5, 4.5, -np.inf)), ("a NaN on a row that is off", (0.0, np.nan, 4.5, 0.0)),
           ("T < 0", (-1.0, 0.5, 4.5, 0.0)), ("M = 0", (262144.0, 0.0, 0.0, 0.0)), ("M < 0", (262144.0, 0.0, -1.0, 0.0)),
           ("W < 0", (262144.0, -0.5, 4.5, 0.0)), ("2 W > M", (262144.0, 2.5, 4.5, 0.0)), ("A < -W", (262144.0, 0.5, 4.5, -0.75)),
           ("A > M - 2 W", (262144.0, 0.5, 4.5, 3.75))]


def coefficients(twma):
    out = np.zeros(8)
    rc = _lib.load().cc_logicle_coefficients(_lib._ptr(np.array(twma, np.float64)), _lib._ptr(out))
    return rc, out


# ---- (a) the referee ------------------------------------------------------------------------------------------------------------------

@needs_extended
@pytest.mark.parametrize("p", L.P, ids=lambda p: "T%g-W%g-M%g-A%g" % p)
def test_the_referee_lies_within_a_unit_of_a_40_digit_root(p):
    mpmath = pytest.importorskip("mpmath")
    rng = np.random.default_rng(17)
    mags = np.exp(rng.uniform(np.log(1e-6), np.log(2 * p[0]), 246))
    v = np.concatenate([mags, -mags, [0.0, -0.0, p[0], -p[0], 5e-324, 1e300, 1e-6, 2 * p[0]]])
    assert v.size == 500
    ref = L.logicle(v, *p)
    worst = 0.0
    with mpmath.workdps(40):
        for x, y in zip(v.tolist(), ref.tolist()):
            exact = L.mp_logicle(x, *p)
            unit = float(np.spacing(max(abs(y), 0.5)))
            worst = max(worst, float(abs(mpmath.mpf(y) - exact) / unit))
    print("the referee: largest distance from the 40-digit root %.3f units over %d values" % (worst, v.size))
    assert worst <= 1.0
    assert np.isfinite(ref).all()


# ---- (b) the coefficients ---------------------------------------------------------------------------------------------------------------

@needs_extended
@pytest.mark.parametrize("p", L.P, ids=lambda p: "T%g-W%g-M%g-A%g" % p)
def test_the_coefficients_satisfy_the_defining_identities(p):
    rc, out = coefficients(p)
    assert rc == 0 and not out[5:].any()
    T, W, M, A = p
    x1, b, d, pa, pc = (np.longdouble(v) for v in out[:5])
    assert out[0] == np.float64(A / (M + A)) + np.float64(W / (M + A)), "x1 is the double x2 + w"
    g = L.G(dict(pa=pa, pc=pc, b=b, d=d), 1 - x1)
    print("G(1 - x1) / T - 1 = %.3g, pc d^2 / (pa b^2) - 1 = %.3g" % (float(g / T - 1), float(pc * d * d / (pa * b * b) - 1)))
    assert abs(g - T) <= 1e-12 * T
    assert abs(pa * b * b - pc * d * d) <= 1e-12 * pa * b * b
    assert _lib.logicle_coefficients(p) == tuple(out[:5].tolist())
    ref = L.coefficients(*p)
    for key, got in zip(("x1", "b", "d", "pa", "pc"), out[:5]):
        assert abs(np.longdouble(got) - ref[key]) <= 1e-14 * max(abs(ref[key]), np.longdouble(1e-300)), key
    if W == 0:
        assert out[2] == out[1], "w == 0: d = b"


def test_a_row_that_is_off_has_no_coefficients():
    rc, out = coefficients((0.0, 0.5, 4.5, 0.0))
    assert rc == 0 and not out.any()
    assert _lib.load().cc_logicle_coefficients(None, _lib._ptr(out)) == -2


# ---- (c) refusals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what,twma", REFUSED, ids=[w for w, _ in REFUSED])
def test_refusals_through_the_library_the_transform_and_read_fcs(tmp_path, what, twma):
    rc, out = coefficients(twma)
    assert rc == -2 and not out.any(), what
    with pytest.raises(ValueError, match="outside"):
        _lib.logicle_coefficients(twma)
    with pytest.raises(ValueError, match="outside"):
        _lib.ListTransform(logicle=twma)
    rows = np.array([L.P[0], twma, L.P[1]])
    with pytest.raises(ValueError, match="outside"):
        _lib.ListTransform(logicle=rows)
    if twma[0] != 0:  # (read_fcs has no way to say "off" but to leave the channel out)
        rec = U.records(np.float32, 20, len(NAMES), 3)
        fn = F.write_fcs(tmp_path / "r.fcs", F.fast_records(rec, BIG), len(NAMES), "F", BIG, 32, names=NAMES, tot=20)
        with pytest.raises(ValueError, match="logicle"):
            fcs.read_fcs(fn, columns=FLUOR, logicle={"B515-A": dict(zip("TWMA", [float(v) for v in twma]))})


def test_refusals_of_shapes_names_and_of_a_channel_with_both(tmp_path):
    with pytest.raises(ValueError, match="logicle is one"):
        _lib.ListTransform(logicle=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="logicle is one"):
        _lib.ListTransform(logicle=np.zeros((2, 3)))
    buf = np.zeros(16, np.float32)
    with pytest.raises(ValueError, match="3 logicle rows for 2"):
        _lib.ListMode(buf, 2, 4, np.float32, columns=[0, 1], transform=_lib.ListTransform(logicle=np.array([L.P[0]] * 3)))
    with pytest.raises(ValueError, match="dimension 1 has a cofactor and a logicle scale"):
        _lib.ListMode(buf, 2, 4, np.float32, columns=[0, 1], transform=_lib.ListTransform(cofactor=[0.0, 5.0], logicle=L.P[0]))
    # a cofactor of 0 beside a row that is on, a cofactor beside a row that is off: neither carries both
    lm = _lib.ListMode(buf, 2, 4, np.float32, columns=[0, 1],
                       transform=_lib.ListTransform(cofactor=[0.0, 5.0], logicle=[L.P[0], (0.0, 0.0, 0.0, 0.0)]))
    assert lm.logicle_descriptor().d == 2 and lm.transform_descriptor() is not None
    # every row off: the `_list_xf` sibling
    off = _lib.ListMode(buf, 2, 4, np.float32, columns=[0, 1], transform=_lib.ListTransform(logicle=np.zeros((2, 4))))
    assert off.logicle_descriptor() is None and off.transform_descriptor() is not None
    assert _lib.ListMode(buf, 2, 4, np.float32).logicle_descriptor() is None
    rec = U.records(np.float32, 20, len(NAMES), 3)
    fn = F.write_fcs(tmp_path / "r.fcs", F.fast_records(rec, BIG), len(NAMES), "F", BIG, 32, names=NAMES, tot=20, ranges=262144)
    for bad, message in (({"Nope-A": {}}, "Nope-A"), ({"T": "big"}, "logicle must be"), (True, "logicle must be"), ({}, None),
                         ({"B515-A": {"Q": 1}}, "logicle must be"), ({"B515-A": 5}, "logicle must be"),
                         ({"T": True}, "logicle must be")):
        if message is None:
            continue
        with pytest.raises(ValueError, match=message):
            fcs.read_fcs(fn, columns=FLUOR, logicle=bad)
    with pytest.raises(ValueError, match="B515-A has a cofactor and a logicle scale"):
        fcs.read_fcs(fn, columns=FLUOR, cofactor={"B515-A": 5}, logicle={"B515-A": {}})
    # $PnE / $PnG are refused as for a cofactor
    fn = F.write_fcs(tmp_path / "g.fcs", F.fast_records(rec, BIG), len(NAMES), "F", BIG, 32, names=NAMES, tot=20,
                     extra={"$P%dG" % (NAMES.index("V450-A") + 1): "2"})
    with pytest.raises(ValueError, match="P6G"):
        fcs.read_fcs(fn, columns=FLUOR, logicle={})
    assert fcs.read_fcs(fn, columns=["B515-A"], logicle={})[0].transform is not None


# ---- (d) the layout -----------------------------------------------------------------------------------------------------------------------

def test_cc_list_logicle_matches_the_header_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("\n".join([
        '#include <stdio.h>', '#include <stddef.h>', '#include "chronoclust_hip.h"', 'int main(void) {',
        'printf("%zu %zu %zu %zu\\n", sizeof(cc_list_logicle), offsetof(cc_list_logicle, d), offsetof(cc_list_logicle, reserved), '
        'offsetof(cc_list_logicle, twma));', 'return 0;', '}']))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = tuple(int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    t = _lib.CcListLogicle
    assert got == (ctypes.sizeof(t), t.d.offset, t.reserved.offset, t.twma.offset) == (16, 0, 4, 8)
    for name in ("cc_points_upload_list_xl", "cc_points_prefetch_list_xl", "cc_col_minmax_list_xl", "cc_online_list_xl",
                 "cc_assign_list_xl", "cc_logicle_coefficients"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    for op, table in _lib._INGEST.items():
        assert table["list_xl"] == table["list_xf"][:-2] + "xl", op


# ---- (e) the sidecar ----------------------------------------------------------------------------------------------------------------------

def test_the_sidecar_forms(tmp_path):
    from chronoclust_amd.scaling.scaler import read_timepoint
    spill = U.spillover(3, 1)[0]
    rec = U.records(np.float32, 70, len(NAMES), 3)
    ranges = [262144, 262144, 10000, 262144, 4096, 1000]
    fn = F.write_fcs(tmp_path / "a.fcs", F.fast_records(rec, BIG), len(NAMES), "F", BIG, 32, names=NAMES, tot=70, ranges=ranges,
                     extra={"$SPILLOVER": U.spillover_text(FLUOR, spill)})
    with open(fn + ".columns", "w") as f:
        f.write("B515-A\nFSC-A\nV450-A\n")

    def sidecar(spec):
        with open(fn + ".transform", "w") as f:
            json.dump(spec, f)
        return fcs.sidecar_transform(fn)

    # one object for every channel: the defaults, T from $PnR
    assert sidecar({"compensate": True, "logicle": {}}) == dict(compensate=True, cofactor=None, logicle={})
    lm = read_timepoint(fn)
    assert lm.transform.m == 3 and lm._cofactors is None
    assert lm._logicle.tolist() == [[10000.0, 0.5, 4.5, 0.0], [262144.0, 0.5, 4.5, 0.0], [1000.0, 0.5, 4.5, 0.0]]
    assert lm.logicle_descriptor().d == 3
    # ... with some parameters given, and a cofactor by name: that channel stays on its cofactor
    assert sidecar({"cofactor": {"FSC-A": 150}, "logicle": {"W": 1, "A": 0.5}}) == \
        dict(compensate=False, cofactor={"FSC-A": 150}, logicle={"W": 1, "A": 0.5})
    lm = read_timepoint(fn)
    assert lm._cofactors.tolist() == [0.0, 150.0, 0.0]
    assert lm._logicle.tolist() == [[10000.0, 1.0, 4.5, 0.5], [0.0, 0.0, 0.0, 0.0], [1000.0, 1.0, 4.5, 0.5]]
    # per channel
    spec = {"V450-A": {"T": 4096, "W": 0.25, "M": 4}, "B515-A": {}}
    assert sidecar({"logicle": spec}) == dict(compensate=False, cofactor=None, logicle=spec)
    lm = read_timepoint(fn)
    assert lm.transform.m == 0
    assert lm._logicle.tolist() == [[10000.0, 0.5, 4.5, 0.0], [0.0, 0.0, 0.0, 0.0], [4096.0, 0.25, 4.0, 0.0]]
    # a channel that holds both a cofactor and a logicle row
    sidecar({"cofactor": {"V450-A": 5}, "logicle": spec})
    with pytest.raises(ValueError, match="V450-A has a cofactor and a logicle scale"):
        read_timepoint(fn)
    # today's sidecars answer as they did
    assert sidecar({"compensate": True, "cofactor": {"B515-A": 5}}) == dict(compensate=True, cofactor={"B515-A": 5})
    for text in ('{"logicle": true}', '{"logicle": 5}', '{"logicle": [1, 2, 3, 4]}', '{"logicle": {"T": "x"}}',
                 '{"logicle": {"B515-A": 5}}', '{"logicle": {"B515-A": {"Q": 1}}}', '{"logicle": {"T": 1, "B515-A": {}}}',
                 '{"logicle": null}'):
        with open(fn + ".transform", "w") as f:
            f.write(text)
        with pytest.raises(ValueError, match="expected.*logicle"):
            fcs.sidecar_transform(fn)


# ---- (f) the host fallback ----------------------------------------------------------------------------------------------------------------

@needs_extended
@pytest.mark.parametrize("p", L.P, ids=lambda p: "T%g-W%g-M%g-A%g" % p)
def test_the_host_fallback_against_the_referee(p):
    v = L.sweep(p[0]).reshape(-1, 4)
    lm = U.list_mode(v, LITTLE, None, None, _lib.ListTransform(logicle=p))
    got = np.asarray(lm)
    assert got.dtype == np.float64 and got.shape == v.shape and np.isfinite(got).all()
    ref = L.logicle(v, *p)
    dist = L.units(got, ref)
    for lo, hi in L.sweep_bands(p[0]):
        band = (np.abs(v) >= lo) & (np.abs(v) <= hi)
        print("|v| in [%g, %g]: largest distance %.3f units over %d values" % (lo, hi, dist[band].max(), band.sum()))
    print("largest distance %.3f units" % dist.max())
    assert dist.max() <= HOST_BOUND_UNITS
    x1 = _lib.logicle_coefficients(p)[0]
    U.same_bits(got[v == 0], np.full(2, x1), "logicle(+-0) = x1")
    assert np.abs(got[np.abs(v) == p[0]] - (1.0, 2 * x1 - 1.0)).max() <= 4 * np.spacing(1.0), "T maps to 1, -T to 2 x1 - 1"


def test_the_host_fallback_composes_with_compensation_and_cofactors():
    n, m = 130, 9
    rng = np.random.default_rng(5)
    src_cols = 20
    rec = U.records(np.float32, n, src_cols, 9)
    perm = rng.permutation(src_cols)
    comp_cols = perm[:m]
    cols = np.concatenate([comp_cols[[5, 2, 7]], perm[m:m + 3]])
    inv = U.spillover(m, 4)[1]
    cof = np.array([0.0, 150.0, 0.0, 0.0, 150.0, 0.0])
    rows = np.array([L.P[0], [0.0] * 4, [0.0] * 4, L.P[2], [0.0] * 4, [0.0] * 4])
    lm = U.list_mode(rec, BIG, cols, None, _lib.ListTransform(comp_cols, inv, cof, rows))
    got = np.asarray(lm)
    comp = U.compensated(U.decoded(rec, cols), U.comp_inputs(rec, cols, None, comp_cols), cols, comp_cols, inv)
    U.same_bits(got[:, [2, 5]], comp[:, [2, 5]], "neither: the compensated value")
    U.same_bits(got[:, [1, 4]], np.arcsinh(comp[:, [1, 4]] / 150.0), "cofactor: what it was")
    if L.EXTENDED:
        for k, p in ((0, L.P[0]), (3, L.P[2])):
            assert L.units(got[:, k], L.logicle(comp[:, k], *p)).max() <= HOST_BOUND_UNITS
    # NaN and Inf come out non-finite
    with np.errstate(all="ignore"):
        bad = _lib.logicle_host(np.array([np.nan, np.inf, -np.inf]), L.P[0])
    assert not np.isfinite(bad).any()


# ---- (g) the host route ---------------------------------------------------------------------------------------------------------------------

def test_a_mixed_width_file_takes_the_host_route_with_logicle_applied(tmp_path):
    n = 40
    rng = np.random.default_rng(2)
    values = rng.integers(0, 200, (n, 4))
    widths = [16, 8, 16, 32]
    names = ["A", "B", "C", "D"]
    spill = U.spillover(2, 6)[0]
    data = F.records(values.tolist(), "u", [w // 8 for w in widths], BIG)
    fn = F.write_fcs(tmp_path / "mixed.fcs", data, 4, "I", BIG, widths, names=names, tot=n, ranges=[256, 256, 256, 256],
                     extra={"$SPILLOVER": U.spillover_text(["C", "A"], spill)})
    got = fcs.read_fcs(fn, columns=["D", "A", "B"], compensate=True, cofactor={"D": 5}, logicle={"W": 0.25, "M": 4})[0]
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (n, 3)
    rec = values.astype(np.float64)
    comp = U.compensated(U.decoded(rec, [3, 0, 1]), U.comp_inputs(rec, [3, 0, 1], None, [2, 0]), [3, 0, 1], [2, 0], np.linalg.inv(spill))
    U.same_bits(got[:, 0], np.arcsinh(rec[:, 3] / 5.0), "the channel with a cofactor keeps it")
    p = (256.0, 0.25, 4.0, 0.0)
    for k in (1, 2):
        U.same_bits(got[:, k], _lib.logicle_host(comp[:, k], p), "the host solve of the compensated values")
        if L.EXTENDED:
            assert L.units(got[:, k], L.logicle(comp[:, k], *p)).max() <= HOST_BOUND_UNITS
    assert (got[:, 2] >= _lib.logicle_coefficients(p)[0]).all() and got[:, 2].max() < 1.0


def test_read_fcs_without_the_keyword_is_what_it_was(tmp_path):
    rec = U.records(np.float32, 30, len(NAMES), 3)
    fn = F.write_fcs(tmp_path / "a.fcs", F.fast_records(rec, BIG), len(NAMES), "F", BIG, 32, names=NAMES, tot=30)
    lm = fcs.read_fcs(fn, columns=["B515-A"], cofactor=5, logicle=None)[0]
    assert lm._logicle is None and lm.logicle_descriptor() is None and lm.transform.logicle is None
    assert fcs.read_fcs(fn, columns=["B515-A"])[0].transform is None
