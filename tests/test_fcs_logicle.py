"""List-mode event records put on the logicle scale on the device (cc_points_upload_list_xl and its kin, the logicle
instances of k_ingest_list_xf / k_col_minmax_list_xf).  The solve is held to its measured distance from the referee of
logicle_util - the root in extended precision, derived from T, W, M, A alone, rounded once - and never to the host route of the
code under test; the two resident copies, the column reduction and the scaled upload hold one value everywhere; compensation and
cofactors compose with it and stay what they were, bit for bit; lg = NULL and rows that are all off ARE the `_list_xf` sibling;
the online phase, the read-only assignment and a group of two cannot tell the records from their own read-back; a prefetch is
adopted by the bits of the logicle rows; every malformed cc_list_logicle is refused before anything runs; app.run on `.fcs`
timepoints with `.transform` sidecars that hold `logicle` writes the files of the run over the read-back.
Shapes are the kernel's edges: n around a 64-event tile, d around a 64-dimension block, slab seams at 64 and 128 events, every
element type and byte order that has a kernel instance."""
import ctypes
import json
import os

import numpy as np
import pytest

import assign_util as A
import fcs_util as F
import logicle_util as L
import scenarios
import table_util as T
import transform_util as U
from pipeline_util import knobs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

LITTLE, BIG = U.LITTLE, U.BIG
NS = (1, 63, 64, 65, 130, 200)
DS = (1, 5, 64, 65)
SLABS = (None, 64, 128)
TYPES = [(t, o) for t in (np.float32, np.float64, np.uint16, np.uint8, np.uint32) for o in (LITTLE, BIG)]  # (every kernel instance)
# The largest distance, in units of np.spacing(max(|y_ref|, 0.5)), of the device's logicle solve from the referee over the sweep
# of test_the_accuracy_sweep - the eight parameter sets of logicle_util.P, |v| log-uniform per three decades from 1e-6 to 2 T,
# 20 000 values per band, both signs, +-0, +-T, the smallest subnormal and 1e300 -, measured on the MI355X
# (profiles/ingest_logicle.txt); the bound of every comparison against the referee is this plus 1 unit for the referee's own
# rounding.
LOGICLE_MEASURED_MAX_UNITS = 2.0
LOGICLE_BOUND_UNITS = LOGICLE_MEASURED_MAX_UNITS + 1.0

needs_extended = pytest.mark.skipif(not L.EXTENDED, reason=L.NEEDS_EXTENDED)


@pytest.fixture(scope="module", params=SLABS, ids=lambda s: "slab%s" % s)
def handle(request):
    from chronoclust_amd import _lib
    env = {} if request.param is None else dict(CHRONOCLUST_HIP_INGEST_SLAB=request.param)
    with knobs(**env):
        h = _lib.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def plain():
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def resident(h, d):
    return h.points_download(d), h.points_download_xt(d)


def one_value(h, d, what):
    """Both resident copies hold the same doubles, the pad rows +0.0; returns the row-major copy."""
    from chronoclust_amd import _lib
    x, xt = resident(h, d)
    assert xt.shape == (_lib.xt_rows(d), x.shape[0]), what
    U.same_bits(xt[:d], x.T, what + ": dimension-major against row-major")
    assert not U.bits(xt[d:]).any(), what + ": pad rows"
    return x


def read_back(lm):
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    try:
        h.points_upload(lm)
        return h.points_download(lm.shape[1])
    finally:
        h.close()


def case(n, d, m, dtype, order, seed, cofactor=None, rows=None):
    """test_fcs_transform's case (its layout, records, masks and the restatement's compensated values) with logicle rows."""
    import test_fcs_transform as X
    from chronoclust_amd import _lib
    c = X.case(n, d, m, dtype, order, seed, cofactor=np.zeros(d) if cofactor is None else cofactor)
    c["rows"] = rows
    c["transform"] = _lib.ListTransform(c["comp_cols"] if m else None, c["inv"], cofactor, rows)
    c["lm"] = U.list_mode(c["rec"], order, c["cols"], c["masks"], c["transform"])
    return c


def thirds(d):
    """(logicle rows [d, 4], cofactors [d]): dimension c on the logicle scale (c % 3 == 0, the parameter sets in turn), on
    cofactor 150 (c % 3 == 1) or on nothing."""
    rows = np.zeros((d, 4))
    for c in range(0, d, 3):
        rows[c] = L.P[(c // 3) % len(L.P)]
    return rows, np.where(np.arange(d) % 3 == 1, 150.0, 0.0)


# ---- 1. the accuracy sweep ----------------------------------------------------------------------------------------------------------

@needs_extended
@pytest.mark.parametrize("p", L.P, ids=lambda p: "T%g-W%g-M%g-A%g" % p)
def test_the_accuracy_sweep(plain, p):
    from chronoclust_amd import _lib
    v = L.sweep(p[0]).reshape(-1, 4)
    lm = U.list_mode(v, LITTLE, None, None, _lib.ListTransform(logicle=p))
    before = plain.stats()["list_points"]
    plain.points_upload(lm)
    assert plain.stats()["list_points"] == before + len(v)
    got = one_value(plain, 4, "sweep")
    assert np.isfinite(got).all()
    x1 = _lib.logicle_coefficients(p)[0]
    U.same_bits(got[v == 0], np.full(2, x1), "logicle(+-0) has the bits of x1")
    ref = L.logicle(v, *p)
    dist = L.units(got, ref)
    bands = L.sweep_bands(p[0])
    for lo, hi in bands:
        band = (np.abs(v) >= lo) & (np.abs(v) <= hi)
        print("(T, W, M, A) = %r, |v| in [%g, %g]: largest distance %.3f units over %d values, %.2f %% off by one or more"
              % (p, lo, hi, dist[band].max(), band.sum(), 100.0 * (dist[band] >= 1).mean()))
        assert band.sum() >= 40000
    for what, sel in (("+-T", np.abs(v) == p[0]), ("the smallest subnormal", v == 5e-324), ("1e300", v == 1e300)):
        print("(T, W, M, A) = %r, %s: %r, distance %.3f units" % (p, what, got[sel].tolist(), dist[sel].max()))
    print("(T, W, M, A) = %r: largest distance %.3f units over %d values" % (p, dist.max(), dist.size))
    assert dist.max() <= LOGICLE_BOUND_UNITS
    # the sweep reached both ends of the range
    mags = np.abs(v[v != 0])
    assert mags.min() == 5e-324 and np.sort(mags)[1] == 1e-6 and (mags == 2 * p[0]).any() and mags.max() == 1e300
    assert got.min() < x1 < got.max() and got[v == 2 * p[0]].min() > 1.0 and got[v == -2 * p[0]].max() < 2 * x1 - 1.0


# ---- 2. one value, everywhere -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
def test_one_value_everywhere(handle, n):
    from chronoclust_amd.scaling.scaler import Scaler
    for di, d in enumerate(DS):
        for mi, m in enumerate((0, 9)):
            ti = (NS.index(n) + 3 * di + 5 * mi) % len(TYPES)
            dtype, order = TYPES[ti]
            rows = np.array([L.P[(c + di) % len(L.P)] if c % 4 != 3 else (0.0,) * 4 for c in range(d)])  # (every fourth: off)
            c = case(n, d, m, dtype, order, 9000 + 100 * n + 10 * d + m, rows=rows)
            what = "%s %s %d x %d, m = %d" % (np.dtype(dtype).name, "big" if order == BIG else "little", n, d, m)
            lm = c["lm"]
            before = handle.stats()["list_points"]
            handle.points_upload(lm)
            assert handle.stats()["list_points"] == before + n, what
            x = one_value(handle, d, what)
            assert np.isfinite(x).all(), what
            off = rows[:, 0] == 0
            U.same_bits(x[:, off], c["exp"][:, off], what + ": a row that is off passes through")
            if L.EXTENDED:
                for k in np.flatnonzero(~off):
                    dist = L.units(x[:, k], L.logicle(c["exp"][:, k], *rows[k]))
                    assert dist.max() <= LOGICLE_BOUND_UNITS, "%s, dimension %d: %.3f units from the referee" % (what, k, dist.max())
            # the column reduction: the very doubles the upload holds (== : the sign of a zero is free)
            before = handle.stats()["list_points"]
            mn, mx = handle.col_minmax(lm)
            assert handle.stats()["list_points"] == before, what
            assert np.array_equal(mn, x.min(axis=0)) and np.array_equal(mx, x.max(axis=0)), what + ": col_minmax"
            # the scaler's fit on it: the scaled upload is numpy's two roundings, the column minimum lands on 0.0
            sc = Scaler()
            sc._finish_fit(mn.copy(), mx.copy())
            handle.points_upload_scaled(lm, sc.scale_, sc.min_)
            xs = one_value(handle, d, what + ", scaled")
            U.same_bits(xs, x * sc.scale_ + sc.min_, what + ": scaled upload")
            assert (xs.min(axis=0) == 0.0).all(), what + ": the column minimum under the scaler's fit"
            assert np.isfinite(xs).all(), what


def test_every_type_and_order_at_130_by_5(plain):
    """Every kernel instance, whichever the parametrised walk above happens to reach."""
    for dtype, order in TYPES:
        rows = np.array([L.P[k] for k in (0, 2, 3, 5, 7)])
        c = case(130, 5, 9, dtype, order, 41, rows=rows)
        what = "%s %s 130 x 5" % (np.dtype(dtype).name, order[0])
        plain.points_upload(c["lm"])
        x = one_value(plain, 5, what)
        assert np.isfinite(x).all()
        mn, mx = plain.col_minmax(c["lm"])
        assert np.array_equal(mn, x.min(axis=0)) and np.array_equal(mx, x.max(axis=0)), what
        if L.EXTENDED:
            for k in range(5):
                assert L.units(x[:, k], L.logicle(c["exp"][:, k], *rows[k])).max() <= LOGICLE_BOUND_UNITS, (what, k)


# ---- 3. composition -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", (0, 1, 9, 64))
def test_composition_with_compensation_and_cofactors(handle, m):
    from chronoclust_amd import _lib
    n, d = 130, 13
    rows, cof = thirds(d)
    for dtype, order in ((np.float32, BIG), (np.uint16, LITTLE), (np.float64, BIG)):
        c = case(n, d, m, dtype, order, 300 + m, cofactor=cof, rows=rows)
        what = "%s, m = %d" % (np.dtype(dtype).name, m)
        handle.points_upload(c["lm"])
        x = one_value(handle, d, what)
        sibling = U.list_mode(c["rec"], order, c["cols"], c["masks"], _lib.ListTransform(c["comp_cols"] if m else None, c["inv"], cof))
        handle.points_upload(sibling)
        held = handle.points_download(d)
        on, with_cof = rows[:, 0] > 0, cof > 0
        nothing = ~on & ~with_cof
        assert on.sum() >= 4 and with_cof.sum() >= 4 and nothing.sum() >= 4
        U.same_bits(x[:, nothing], c["exp"][:, nothing], what + ": neither - the restatement's compensated values")
        U.same_bits(x[:, with_cof], held[:, with_cof], what + ": cofactor 150 - what the `_list_xf` route holds")
        U.same_bits(held[:, on], c["exp"][:, on], what + ": the sibling holds the compensated values")
        assert np.isfinite(x).all()
        if L.EXTENDED:
            for k in np.flatnonzero(on):
                dist = L.units(x[:, k], L.logicle(c["exp"][:, k], *rows[k]))
                print("%s, dimension %d %r: largest distance %.3f units" % (what, k, tuple(rows[k]), dist.max()))
                assert dist.max() <= LOGICLE_BOUND_UNITS, (what, k)


# ---- 4. lg = NULL and all-zero T ------------------------------------------------------------------------------------------------------

def test_null_and_rows_that_are_all_off_are_the_sibling(plain):
    from chronoclust_amd import _lib
    n, d, m = 130, 6, 3
    import test_fcs_transform as X
    c = X.case(n, d, m, np.float32, BIG, 5, cofactor=np.full(d, 5.0))
    lm = c["lm"]
    lib, hh = plain._lib, plain._h
    desc, xf = lm.descriptor(), lm.transform_descriptor()
    plain.points_upload(lm)
    own = resident(plain, d)
    zeros = np.zeros((d, 4))
    zeros[:, 1:] = (0.5, 4.5, 0.0)  # (T == 0 alone switches a row off)
    off = _lib.CcListLogicle(d, 0, _lib._ptr(zeros))
    mn0, mx0 = plain.col_minmax(lm)
    for what, lg in (("lg = NULL", None), ("every T == 0", ctypes.byref(off))):
        before = plain.stats()["list_points"]
        plain._check(lib.cc_points_upload_list_xl(hh, ctypes.byref(desc), ctypes.byref(xf), lg, None, None))
        assert plain.stats()["list_points"] == before + n, what
        x, xt = resident(plain, d)
        U.same_bits(x, own[0], what)
        U.same_bits(xt, own[1], what + ", dimension-major")
        mn, mx = np.zeros(d), np.zeros(d)
        plain._check(lib.cc_col_minmax_list_xl(hh, ctypes.byref(desc), ctypes.byref(xf), lg, _lib._ptr(mn), _lib._ptr(mx)))
        assert np.array_equal(mn, mn0) and np.array_equal(mx, mx0), what
        # a prefetch through the sibling is adopted by the `_xl` upload that says the same
        plain._check(lib.cc_points_prefetch_list_xf(hh, ctypes.byref(desc), ctypes.byref(xf), None, None))
        plain._check(lib.cc_points_upload_list_xl(hh, ctypes.byref(desc), ctypes.byref(xf), lg, None, None))
        U.same_bits(plain.points_download(d), own[0], what + ", prefetched")
    # without a transform beside it: the `_list` sibling
    bare = _lib.ListMode(lm.buffer, n, lm.src_cols, lm.dtype, columns=c["cols"])
    plain._check(lib.cc_points_upload_list_xl(hh, ctypes.byref(desc), None, ctypes.byref(off), None, None))
    U.same_bits(plain.points_download(d), np.asarray(bare, np.float64), "no transform, rows off")
    # through Python: rows that are all off route to the sibling
    same = _lib.ListMode(lm.buffer, n, lm.src_cols, lm.dtype, columns=c["cols"],
                         transform=_lib.ListTransform(c["comp_cols"], c["inv"], np.full(d, 5.0), zeros))
    assert plain._source(same)[0] == "list_xf"
    plain.points_upload(same)
    U.same_bits(plain.points_download(d), own[0], "ListMode with rows that are all off")


# ---- 5. downstream does not notice --------------------------------------------------------------------------------------------------

def raw_for(X, seed, p=L.P[0], extra=4):
    """Big-endian float64 records whose logicle gives (about) X: logicle_util.inverse(X), the first half of the dimensions
    spilled into each other, `extra` channels of NaN between them.  Returns the ListMode."""
    from chronoclust_amd import _lib
    n, d = X.shape
    rng = np.random.default_rng(seed)
    m = max(1, min(d // 2, 9))
    spill, inv = U.spillover(m, seed)
    perm = rng.permutation(d + extra)
    cols = perm[:d]
    truth = L.inverse(X, *p)
    truth[:, :m] = truth[:, :m] @ spill  # (building an input: any rounding will do)
    rec = np.full((n, d + extra), np.nan)
    rec[:, cols] = truth
    return U.list_mode(rec, BIG, cols, None, _lib.ListTransform(cols[:m], inv, None, p))


@needs_extended
@pytest.mark.parametrize("d,prune", [(5, None), (13, None), (13, 2)])
def test_the_online_phase_does_not_notice(d, prune):
    import test_fcs_points as P
    n = 300
    cfg, Xs = P.stream(d, n)
    lms = [raw_for(X, 50 + t) for t, X in enumerate(Xs)]
    backs = [read_back(lm) for lm in lms]
    assert all(np.abs(b - X).max() < 1e-9 for b, X in zip(backs, Xs)), "the records do not hold the blobs"
    with knobs(**({} if prune is None else dict(CHRONOCLUST_HIP_PRUNE=prune))):
        _, exp = P.run_stream(cfg, backs)
        _, got = P.run_stream(cfg, lms)
    P.same_run(got, exp, "d=%d prune=%s" % (d, prune), np.cumsum([n, n]).tolist())
    assert len(set(got[-1]["path"].tolist())) > 1, "every point took one path: nothing was compared"


@needs_extended
def test_assign_with_a_chunk_of_100_does_not_notice():
    import test_fcs_points as P
    cfg, Xs = P.stream(13, 300)
    with knobs(CHRONOCLUST_HIP_ASSIGN_CHUNK=100, CHRONOCLUST_HIP_INGEST_SLAB=64):
        hdd, _ = P.run_stream(cfg, [Xs[0]])
    h = hdd._h
    q = np.vstack([Xs[0][:100], Xs[1][:65]])
    lm = raw_for(q, 9)
    back = read_back(lm)
    exp = h.assign(back, want_dist=True)
    before = h.stats()
    got = h.assign(lm, want_dist=True)
    after = h.stats()
    A.same_assign(got, exp, "records on the logicle scale")
    U.same_bits(got[2], exp[2], "dist")
    assert after["assign_launches"] == 2 and after["assign_points"] == 165
    assert after["list_points"] == before["list_points"] + 165
    assert len(set(got[1].tolist())) > 1, "the queries all took one path: nothing was compared"


@needs_extended
def test_a_group_of_two_does_not_notice():
    pcores, outliers, par, X, meta = T.build_online("stale-3000+1096x20")
    from chronoclust_amd import _lib
    lm = raw_for(X, 21)
    back = read_back(lm)
    assert np.abs(back - X).max() < 1e-9
    h = _lib.Handle(0)
    try:
        single = T.handle_online(h, (pcores, outliers, par, back, meta))
        lists = [h.export(kind) for kind in (0, 1)]
        counters = h.counters()
    finally:
        h.close()
    hs, labels, stats = T.group_online(2, (pcores, outliers, par, lm, meta))
    try:
        for rank in range(2):
            for key, a, b in (("uid", labels[rank][0][0], single[0][0]), ("path", labels[rank][0][1], single[0][1])):
                diff = T._first_diff(a, b)
                assert diff is None, "rank %d %s: %s" % (rank, key, diff)
            for kind in (0, 1):
                got = hs[rank].export(kind)
                for key in T.KEYS:
                    assert got[key].tobytes() == lists[kind][key].tobytes(), (rank, kind, key)
            assert hs[rank].counters() == counters
            assert stats[rank]["list_points"] == len(X) and stats[rank]["sharded_windows"] > 0, stats[rank]
    finally:
        for g in hs:
            g.close()


# ---- 6. prefetch ----------------------------------------------------------------------------------------------------------------------

def test_prefetch_is_adopted_by_the_same_logicle_rows_only(handle):
    from chronoclust_amd import _lib
    n, d, m = 200, 13, 9
    rows, cof = thirds(d)
    c = case(n, d, m, np.float32, BIG, 77, cofactor=cof, rows=rows)
    lm, cols = c["lm"], c["cols"]

    def variant(rows_, cof_=cof):
        tr = None if rows_ is None and cof_ is None else _lib.ListTransform(c["comp_cols"], c["inv"], cof_, rows_)
        return _lib.ListMode(lm.buffer, n, lm.src_cols, lm.dtype, columns=cols, transform=tr)

    def values(v):
        handle.points_upload(v)
        return handle.points_download(d)

    own = values(lm)
    before = handle.stats()["list_points"]
    handle.points_prefetch(lm)
    handle.points_upload(lm)  # adopted
    assert handle.stats()["list_points"] == before + n
    U.same_bits(one_value(handle, d, "prefetched"), own, "prefetched")
    # equal rows built anew: adopted too
    handle.points_prefetch(lm)
    handle.points_upload(variant(rows.copy(), cof.copy()))
    U.same_bits(handle.points_download(d), own, "equal rows")
    one_bit = rows.copy()
    one_bit[3, 1] = np.nextafter(one_bit[3, 1], 0.0)  # (one bit of one W)
    moved = rows.copy()
    moved[[3, 5]] = moved[[5, 3]]  # (a row that is on moves to a dimension that was on nothing)
    other = rows.copy()
    other[0], other[3] = rows[3], rows[0]  # (two rows that are on change places)
    variants = {"one bit of W": variant(one_bit), "a row moved to another dimension": variant(moved),
                "two rows exchanged": variant(other), "no logicle rows": variant(None)}
    for what, v in variants.items():
        assert v._bytes.ctypes.data == lm._bytes.ctypes.data
        want = values(v)
        assert not np.array_equal(want, own), what
        for first, second, exp in ((lm, v, want), (v, lm, own)):
            handle.points_prefetch(first)
            handle.points_upload(second)  # discarded: other rows
            U.same_bits(one_value(handle, d, what), exp, "only %s differs" % what)
    # scaled prefetch with the rows, adopted
    scale, min_ = np.full(d, 0.25), np.full(d, 0.5)
    handle.points_prefetch(lm, scale, min_)
    handle.points_upload_scaled(lm, scale, min_)
    U.same_bits(handle.points_download(d), own * scale + min_, "scaled prefetch")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_at_the_boundary_leave_the_handle_as_it_was(plain):
    from chronoclust_amd import _lib
    handle = plain
    n, d, m = 40, 6, 3
    rows = np.array([L.P[0], (0.0,) * 4, L.P[1], (0.0,) * 4, L.P[2], (0.0,) * 4])
    cof = np.array([0.0, 5.0, 0.0, 5.0, 0.0, 0.0])
    c = case(n, d, m, np.float32, BIG, 5, cofactor=cof, rows=rows)
    lm = c["lm"]
    handle.points_upload(lm)
    held = resident(handle, d)
    desc, xf = lm.descriptor(), lm.transform_descriptor()
    keep = []

    def lg(twma=rows, d_=d, reserved=0, null=False):
        a = np.ascontiguousarray(twma, dtype=np.float64)
        keep.append(a)
        return _lib.CcListLogicle(d_, reserved, None if null else _lib._ptr(a))

    def with_row(k, row):
        out = rows.copy()
        out[k] = row
        return out

    cases = [("d differs", lg(d_=d - 1), "d is 5"), ("d differs, upwards", lg(np.vstack([rows, rows[:1]]), d_=d + 1), "d is 7"),
             ("twma is null", lg(null=True), "twma is null"),
             ("a NaN T", lg(with_row(2, (np.nan, 0.5, 4.5, 0.0))), "dimension 2: a parameter is not finite"),
             ("an infinite M", lg(with_row(0, (262144.0, 0.5, np.inf, 0.0))), "dimension 0: a parameter is not finite"),
             ("a NaN on a row that is off", lg(with_row(5, (0.0, 0.5, 4.5, np.nan))), "dimension 5: a parameter is not finite"),
             ("T < 0", lg(with_row(4, (-1.0, 0.5, 4.5, 0.0))), "dimension 4: T is negative"),
             ("M = 0", lg(with_row(0, (262144.0, 0.0, 0.0, 0.0))), "M must be positive"),
             ("W < 0", lg(with_row(0, (262144.0, -0.5, 4.5, 0.0))), "W is negative"),
             ("2 W > M", lg(with_row(0, (262144.0, 2.5, 4.5, 0.0))), "2 W exceeds M"),
             ("A < -W", lg(with_row(0, (262144.0, 0.5, 4.5, -0.75))), "A is below -W"),
             ("A > M - 2 W", lg(with_row(0, (262144.0, 0.5, 4.5, 3.75))), "A exceeds M - 2 W"),
             ("a cofactor and a row", lg(with_row(3, L.P[3])), "dimension 3 has a cofactor and a logicle scale"),
             ("reserved", lg(reserved=1), "reserved")]
    before = handle.stats()
    counters = handle.counters()
    mn, mx = np.zeros(d), np.zeros(d)
    uid, path = np.zeros(n, np.int64), np.zeros(n, np.int8)
    lib, hh = handle._lib, handle._h
    p_desc, p_xf = ctypes.byref(desc), ctypes.byref(xf)
    for what, g, reason in cases:
        p_lg = ctypes.byref(g)
        calls = [lib.cc_points_upload_list_xl(hh, p_desc, p_xf, p_lg, None, None),
                 lib.cc_points_prefetch_list_xl(hh, p_desc, p_xf, p_lg, None, None),
                 lib.cc_col_minmax_list_xl(hh, p_desc, p_xf, p_lg, _lib._ptr(mn), _lib._ptr(mx)),
                 lib.cc_online_list_xl(hh, p_desc, p_xf, p_lg, _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p)),
                 lib.cc_assign_list_xl(hh, p_desc, p_xf, p_lg, _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p), None)]
        assert calls == [-2] * 5, (what, calls)  # CC_ERR_BAD_ARG
        assert reason in lib.cc_last_error(hh).decode(), (what, lib.cc_last_error(hh))
    # the siblings' refusals stand beside them
    good = lg()
    bad_xf = lm.transform_descriptor()
    bad_xf.reserved = 1
    assert lib.cc_points_upload_list_xl(hh, p_desc, ctypes.byref(bad_xf), ctypes.byref(good), None, None) == -2
    assert lib.cc_points_upload_list_xl(hh, p_desc, p_xf, ctypes.byref(good), _lib._ptr(mn), None) == -2
    # nothing moved, nothing was launched or counted
    after = handle.stats()
    for key in ("list_points", "view_points", "f32_points", "assign_launches", "assign_points", "scan_launches", "scan_u_launches",
                "scan_p_launches", "windows", "points"):
        assert after[key] == before[key], key
    assert handle.counters() == counters
    x, xt = resident(handle, d)
    U.same_bits(x, held[0], "resident points behind refused calls")
    U.same_bits(xt, held[1], "resident points behind refused calls, dimension-major")
    # and the good one is taken
    handle._check(lib.cc_points_upload_list_xl(hh, p_desc, p_xf, ctypes.byref(good), None, None))
    U.same_bits(handle.points_download(d), held[0], "the rows as they were")


# ---- 8. NaN -----------------------------------------------------------------------------------------------------------------------------

def test_nan_in_a_logicle_channel_is_refused_and_elsewhere_is_not(plain):
    n, d = 130, 5
    for dtype in (np.float32, np.float64):
        rows = np.array([L.P[0]] * d)
        c = case(n, d, 0, dtype, BIG, 31, rows=rows)
        src_cols = c["rec"].shape[1]
        neither = [v for v in range(src_cols) if v not in c["cols"]]
        assert neither
        plain.points_upload(c["lm"])
        clean = plain.points_download(d)
        for value in (np.nan, np.inf, -np.inf):
            rec = c["rec"].copy()
            rec[100, neither[0]] = value
            lm = U.list_mode(rec, BIG, c["cols"], None, c["transform"])
            plain.points_upload(lm)  # unselected, uncompensated: never read
            U.same_bits(plain.points_download(d), clean, "a %r in a channel that is neither selected nor compensated" % value)
            rec[100, c["cols"][2]] = value
            lm = U.list_mode(rec, BIG, c["cols"], None, c["transform"])
            with pytest.raises(ValueError, match="non-finite"):
                plain.points_upload(lm)
            plain.points_prefetch(lm)
            with pytest.raises(ValueError, match="non-finite"):
                plain.points_upload(lm)


# ---- 9. app.run end to end --------------------------------------------------------------------------------------------------------------

@needs_extended
def test_app_run_on_fcs_timepoints_with_logicle_sidecars(tmp_path, monkeypatch):
    from chronoclust_amd import _lib, app, fcs
    from test_app_end_to_end import _reset_logging
    n, d = 400, 5
    markers = ["CD%d" % i for i in range(d)]
    names = ["Time", markers[3], "FSC-A", markers[0], markers[4], "SSC-A", markers[1], markers[2]]
    comp_names = [markers[1], "FSC-A", markers[3]]  # (one compensated channel is not clustered on)
    spill = U.spillover(3, 8)[0]
    params = scenarios.blob_params(n)
    spec = {"compensate": True, "logicle": {"W": 0.25, "M": 4}}  # (T: the channels' $PnR)
    p = (10000.0, 0.25, 4.0, 0.0)
    files, backs = [], []
    for t in range(2):
        X = scenarios.make_blobs(900 + t, n, d, 8, 0.01)
        truth = np.zeros((n, len(names)), np.float32)
        for k, name in enumerate(markers):
            truth[:, names.index(name)] = L.inverse(X[:, k], *p)
        truth[:, names.index("FSC-A")] = np.random.default_rng(t).uniform(0, 0.01, n)
        idx = [names.index(c) for c in comp_names]
        rec = truth.copy()
        rec[:, idx] = truth[:, idx] @ spill.astype(np.float32)
        rec.view(np.uint32)[:, names.index("Time")] = 0x7FC00000  # (a NaN pattern in a channel nobody reads)
        fn = os.path.join(str(tmp_path), "tp%d.fcs" % t)
        F.write_fcs(fn, F.fast_records(rec, BIG), len(names), "F", BIG, 32, names=names, tot=n, pad_before_data=t % 2, ranges=10000,
                    extra={"$SPILLOVER": U.spillover_text(comp_names, spill)})
        with open(fn + ".columns", "w") as f:
            f.write("\n".join(markers) + "\n")
        with open(fn + ".transform", "w") as f:
            json.dump(spec, f)
        files.append(fn)
        lm = fcs.read_fcs(fn, columns=markers, compensate=True, logicle=spec["logicle"])[0]
        assert isinstance(lm, _lib.ListMode) and lm.transform.m == 3 and lm._logicle.tolist() == [list(p)] * d
        backs.append(read_back(lm))
        assert np.abs(backs[-1] - X).max() < 1e-4
    npys = []
    for t, b in enumerate(backs):
        fn = os.path.join(str(tmp_path), "tp%d.npy" % t)
        np.save(fn, b)
        with open(fn + ".columns", "w") as f:
            f.write("\n".join(markers) + "\n")
        npys.append(fn)
    seen, made = [], []

    class Recording(app.HDDStream):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

        def online_microcluster_maintenance(self, input_dataset, *a, **kw):
            seen.append(input_dataset)
            return super().online_microcluster_maintenance(input_dataset, *a, **kw)

    outs = []
    try:
        out = os.path.join(str(tmp_path), "out_npy")
        os.makedirs(out)
        app.run(data=npys, output_directory=out, normalise_data=True, **params)
        outs.append(out)
        _reset_logging()
        # the events of the .fcs run are never decoded on the host: ListMode's host decode is out of reach during it
        monkeypatch.setattr(app, "HDDStream", Recording)
        monkeypatch.setattr(_lib.ListMode, "__array__", lambda *a, **kw: pytest.fail("the events were decoded on the host"))
        out = os.path.join(str(tmp_path), "out_fcs")
        os.makedirs(out)
        app.run(data=files, output_directory=out, normalise_data=True, **params)
        outs.append(out)
    finally:
        _reset_logging()
    assert len(seen) == 2 and all(isinstance(x, _lib.ListMode) and x.logicle_descriptor() is not None for x in seen)
    stats = made[0].stats()
    assert stats["list_points"] >= 2 * n and stats["view_points"] == 0 and stats["f32_points"] == 0
    for fn in ["result.csv"] + ["cluster_points_D%d.csv" % t for t in range(2)]:
        a, b = (open(os.path.join(o, fn), "rb").read() for o in outs)
        assert a == b and len(a) > 0, fn
    assert len(open(os.path.join(outs[1], "result.csv")).read().splitlines()) > 2, "no cluster was written: nothing was compared"
