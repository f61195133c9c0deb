"""Point views compensated and arcsinh- or logicle-transformed on the device (cc_points_upload_view_xl and its kin: k_ingest_xf /
k_col_minmax_view_xf for the columns form, the list kernels over rows for the rows form), through _lib.TransformedPoints.
The referee: every value of the nine view types is exact in double, so the widened values laid out as native float64 event
records and sent through the `_list_xl` route with the same transform - the kernels this route was modelled on - are what the
view route must hold BIT FOR BIT: the row-major copy, the dimension-major copy with its pad rows, the column reduction.
Beside it, independent of that route: the compensation alone against transform_util's explicit loop on inputs that tell the
specified order from a fused and from a descending sum; asinh within the bound test_fcs_transform.py keeps against the
extended-precision reference; the logicle scale within the bound test_fcs_logicle.py keeps against its referee.
Shapes are the kernels' edges: n around a 64-point tile and a 256-row chunk of the reduction, slab seams at 128 points, d around
the pad rows and the 64-dimension block, m from none to CC_MAX_COMP with compensated columns on both sides of a block boundary."""
import ctypes

import numpy as np
import pytest

import assign_util as A
import logicle_util as L
import table_util as T
import transform_util as U
import view_transform_util as V
from pipeline_util import knobs
from test_fcs_logicle import LOGICLE_BOUND_UNITS
from test_fcs_transform import ASINH_BOUND_ULP

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

NS = (1, 63, 64, 65, 257)
SEAM_NS = (129, 300)
DS = (1, 3, 13, 20, 64, 65, 130)
MS = (0, 1, 2, 9, 64)
COFACTORS = ("none", "scalar", "per dimension")
LOGICLES = ("none", "all", "some", "off")


@pytest.fixture(scope="module")
def plain():
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def seamed():
    """slabs of 128 points: n = 129 is a full slab and one point, n = 300 three slabs, the last partial"""
    from chronoclust_amd import _lib
    with knobs(CHRONOCLUST_HIP_INGEST_SLAB=128):
        h = _lib.Handle(0)
    yield h
    h.close()


def one_value(h, d, what):
    """Both resident copies hold the same doubles, the pad rows +0.0; returns (row-major, dimension-major)."""
    from chronoclust_amd import _lib
    x, xt = V.resident(h, d)
    assert xt.shape == (_lib.xt_rows(d), x.shape[0]), what
    U.same_bits(xt[:d], x.T, what + ": dimension-major against row-major")
    assert not U.bits(xt[d:]).any(), what + ": pad rows"
    return x, xt


def against_the_referee(h, a, tr, what, scaled=True):
    """`a` with `tr` through the view route against the same values through the `_list_xl` route: X, Xt, col_minmax, and under
    the scaler fitted from col_minmax the scaled upload, whose column minima are exactly 0.0.  Returns the unscaled X."""
    from chronoclust_amd import _lib
    from chronoclust_amd.scaling.scaler import Scaler
    n, d = a.shape
    tp = _lib.TransformedPoints(a, tr)
    ref = V.referee_source(a, tr)
    h.points_upload(ref)
    exp = one_value(h, d, what + " (referee)")
    exp_mm = h.col_minmax(ref)
    before = h.stats()
    h.points_upload(tp)
    after = h.stats()
    assert after["view_points"] == before["view_points"] + n and after["list_points"] == before["list_points"], what
    got = one_value(h, d, what)
    U.same_bits(got[0], exp[0], what + ": X")
    U.same_bits(got[1], exp[1], what + ": Xt with its pad rows")
    got_mm = h.col_minmax(tp)
    assert h.stats()["view_points"] == after["view_points"], what
    U.same_bits(got_mm[0], exp_mm[0], what + ": col_minmax, minima")
    U.same_bits(got_mm[1], exp_mm[1], what + ": col_minmax, maxima")
    if scaled and np.isfinite(got_mm[0]).all():
        sc = Scaler()
        sc._finish_fit(got_mm[0].copy(), got_mm[1].copy())
        h.points_upload_scaled(ref, sc.scale_, sc.min_)
        exp_s = one_value(h, d, what + " (referee, scaled)")
        h.points_upload_scaled(tp, sc.scale_, sc.min_)
        got_s = one_value(h, d, what + ", scaled")
        U.same_bits(got_s[0], exp_s[0], what + ": scaled X")
        U.same_bits(got_s[1], exp_s[1], what + ": scaled Xt")
        assert (got_s[0].min(axis=0) == 0.0).all(), what + ": the resident minimum under the scaler's fit"
    return got[0]


def combos(n, turn):
    """Every (d, m) with the element type, the layout, the cofactors and the logicle rows turning, so that within one n every
    type meets both forms and every variant of the transform."""
    k = turn
    for d in DS:
        for m in MS:
            dtype = V.TYPES[k % len(V.TYPES)]
            layout = V.LAYOUTS[(k // 2) % len(V.LAYOUTS)]
            cof = COFACTORS[(k // 3) % len(COFACTORS)]
            lg = LOGICLES[(k // 5) % len(LOGICLES)]
            if m == 0 and cof == "none" and lg in ("none", "off"):
                cof = "scalar"  # (a transform that asks for nothing is the sibling: its own test)
            k += 1
            yield d, m, dtype, layout, cof, lg


def run_combos(h, n, turn):
    seen_types, seen_layouts = set(), set()
    for d, m, dtype, layout, cof, lg in combos(n, turn):
        a = V.laid_out(V.values(dtype, n, d, 1000 * n + 10 * d + m), layout)
        cofactor = V.cofactors(cof, d)
        tr = V.transform(d, m, 7 * d + m, cofactor, V.logicle_rows(lg, d, cofactor))[0]
        what = "%s %s %d x %d, m = %d, cofactors %s, logicle %s" % (np.dtype(dtype).name, layout, n, d, m, cof, lg)
        against_the_referee(h, a, tr, what)
        seen_types.add(dtype)
        seen_layouts.add(layout)
    assert len(seen_types) == len(V.TYPES) and len(seen_layouts) == len(V.LAYOUTS)


# ---- 1. the referee: the `_list_xl` route over the widened values -----------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
def test_bit_for_bit_against_the_list_route(plain, n):
    run_combos(plain, n, NS.index(n))


@pytest.mark.parametrize("n", SEAM_NS)
def test_bit_for_bit_across_a_slab_seam(seamed, n):
    run_combos(seamed, n, 3 + SEAM_NS.index(n))


def test_every_type_in_every_layout(plain):
    """All nine element types x the three rows forms and the three columns forms, with and without the logicle solve: every new
    kernel instance, and C-contiguous float64 / float32, which take the view route when transformed."""
    n, d, m = 130, 13, 9
    for ti, dtype in enumerate(V.TYPES):
        for li, layout in enumerate(V.LAYOUTS):
            a = V.laid_out(V.values(dtype, n, d, 50 + ti), layout)
            for lg in ("none", "some"):
                cofactor = V.cofactors("per dimension", d)
                tr = V.transform(d, m, 3 + li, cofactor, V.logicle_rows(lg, d, cofactor))[0]
                against_the_referee(plain, a, tr, "%s %s logicle %s" % (np.dtype(dtype).name, layout, lg), scaled=lg == "some")


def test_rows_that_are_all_off_and_a_transform_that_asks_for_nothing_are_the_sibling(plain):
    from chronoclust_amd import _lib
    n, d = 130, 13
    for layout in ("c", "f"):
        a = V.laid_out(V.values(np.float32, n, d, 5), layout)
        wide = V.widened(a)
        off = np.zeros((d, 4))
        for tr in (None, _lib.ListTransform(), _lib.ListTransform(logicle=off)):
            before = plain.stats()["view_points"]
            plain.points_upload(_lib.TransformedPoints(a, tr))
            assert plain.stats()["view_points"] == before + n
            x, _ = one_value(plain, d, layout)
            U.same_bits(x, wide, "%s: no transform" % layout)
        # all rows off beside a compensation: the transform without logicle rows
        with_off, cc, inv = V.transform(d, 9, 4, 5.0, off)
        without = _lib.ListTransform(cc, inv, 5.0)
        plain.points_upload(_lib.TransformedPoints(a, without))
        exp = plain.points_download(d)
        plain.points_upload(_lib.TransformedPoints(a, with_off))
        U.same_bits(plain.points_download(d), exp, "%s: rows that are all off" % layout)


# ---- 2. direct checks, independent of the list route ----------------------------------------------------------------------------------

def compensation_case(dtype, layout, seed=11):
    n, d = 130, 9
    a = V.laid_out(V.values(dtype, n, d, seed), layout)
    tr, cc, inv = V.transform(d, 9, seed)
    x = V.widened(a)
    xs = np.ascontiguousarray(x[:, cc])
    return a, tr, cc, inv, x, xs


def test_compensation_alone_is_the_explicit_loop(plain):
    """Bit for bit against transform_util.compensated, on inputs of which at least a tenth would be another double under the
    sum with every step fused and under the descending sum (asserted first: a test that cannot tell them apart shows nothing)."""
    from chronoclust_amd import _lib
    cols = np.arange(9)
    for ti, dtype in enumerate(V.TYPES):
        layout = V.LAYOUTS[ti % len(V.LAYOUTS)]
        a, tr, cc, inv, x, xs = compensation_case(dtype, layout)
        exp = U.compensated(x, xs, cols, cc, inv)
        fused = U.compensated_fused(x, xs, cols, cc, inv)
        desc = U.compensated(x, xs, cols, cc, inv, descending=True)
        for what, other in (("fused", fused), ("descending", desc)):
            share = float((U.bits(other) != U.bits(exp)).mean())
            assert share >= 0.10, (np.dtype(dtype).name, what, share)
        for lay in (layout, V.LAYOUTS[(ti + 3) % len(V.LAYOUTS)]):  # (one rows form and one columns form)
            tp = _lib.TransformedPoints(V.laid_out(a, lay), tr)
            plain.points_upload(tp)
            what = "%s %s 130 x 9" % (np.dtype(dtype).name, lay)
            U.same_bits(one_value(plain, 9, what)[0], exp, what)
            U.same_bits(np.asarray(tp), exp, what + ": TransformedPoints' host transform")


def test_asinh_is_within_the_kept_bound(plain):
    from chronoclust_amd import _lib
    from test_fcs_transform import sweep
    v, c = sweep()
    for layout in ("c", "f"):
        plain.points_upload(_lib.TransformedPoints(V.laid_out(v, layout), _lib.ListTransform(cofactor=c)))
        got = one_value(plain, 4, "sweep " + layout)[0]
        q = np.divide(v, c)
        dist = U.ulp_distance(got, U.asinh_reference(q))
        print("asinh, %s: largest distance from the reference %d ulp over %d values" % (layout, dist.max(), dist.size))
        assert (got[q == 0] == 0).all()
        assert dist.max() <= ASINH_BOUND_ULP
    # compensated values through the same division and asinh: v bit for bit from the explicit loop
    a, tr, cc, inv, x, xs = compensation_case(np.float32, "f")
    cof = np.full(9, 150.0)
    plain.points_upload(_lib.TransformedPoints(a, _lib.ListTransform(cc, inv, cof)))
    dist = U.ulp_distance(one_value(plain, 9, "compensated")[0], U.with_cofactors(U.compensated(x, xs, np.arange(9), cc, inv), cof))
    assert dist.max() <= ASINH_BOUND_ULP


@pytest.mark.skipif(not L.EXTENDED, reason=L.NEEDS_EXTENDED)
def test_logicle_is_within_the_kept_bound(plain):
    from chronoclust_amd import _lib
    for pi, p in enumerate(L.P[:3]):
        v = np.ascontiguousarray(L.sweep(p[0], per_band=2000).reshape(-1, 4))
        for layout in ("wasteful", "frange"):
            plain.points_upload(_lib.TransformedPoints(V.laid_out(v, layout), _lib.ListTransform(logicle=p)))
            got = one_value(plain, 4, "logicle sweep")[0]
            dist = L.units(got, L.logicle(v, *p))
            print("logicle %r, %s: %.3f units from the referee over %d values" % (p, layout, dist.max(), dist.size))
            assert dist.max() <= LOGICLE_BOUND_UNITS
    # behind a compensation: v bit for bit from the explicit loop, then the referee's scale
    a, tr, cc, inv, x, xs = compensation_case(np.int16, "transpose")
    plain.points_upload(_lib.TransformedPoints(a, _lib.ListTransform(cc, inv, logicle=V.LOGICLE)))
    exp = L.logicle(U.compensated(x, xs, np.arange(9), cc, inv), *V.LOGICLE)
    assert L.units(one_value(plain, 9, "compensated")[0], exp).max() <= LOGICLE_BOUND_UNITS


# ---- 3. non-finite values and refusals -------------------------------------------------------------------------------------------------

def test_nan_and_overflow_in_a_compensated_column_refuse_the_upload(plain):
    from chronoclust_amd import _lib
    n, d = 130, 20
    for layout in ("c", "f"):
        base = V.values(np.float64, n, d, 9)
        tr, cc, inv = V.transform(d, 9, 2, 5.0)
        plain.points_upload(_lib.TransformedPoints(V.laid_out(base, layout), tr))
        for value in (np.nan, np.inf):
            a = base.copy()
            a[100, cc[4]] = value
            tp = _lib.TransformedPoints(V.laid_out(a, layout), tr)
            with pytest.raises(ValueError, match="non-finite"):
                plain.points_upload(tp)
            plain.points_prefetch(tp)
            with pytest.raises(ValueError, match="non-finite"):
                plain.points_upload(tp)
        # finite inputs whose compensated sum overflows: the finiteness test is compiled in for every instance
        huge = np.full((n, d), 1e308)
        big_inv = np.full((9, 9), 4.0)
        with pytest.raises(ValueError, match="non-finite"):
            plain.points_upload(_lib.TransformedPoints(V.laid_out(huge, layout), _lib.ListTransform(cc, big_inv)))
        ints = V.values(np.uint16, n, d, 3)
        with pytest.raises(ValueError, match="non-finite"):
            plain.points_upload(_lib.TransformedPoints(V.laid_out(ints, layout), _lib.ListTransform(cc, np.full((9, 9), 1e307))))
        # the handle stays usable
        against_the_referee(plain, V.laid_out(base, layout), tr, "behind refused uploads, " + layout)


def test_entry_refusals_name_their_reason_and_leave_the_handle_usable(plain):
    from chronoclust_amd import _lib
    n, d = 40, 6
    a = V.laid_out(V.values(np.float32, n, d, 1), "f")
    cof = np.full(d, 5.0)
    tr, cc, inv = V.transform(d, 3, 1, cof)
    tp = _lib.TransformedPoints(a, tr)
    plain.points_upload(tp)
    held = V.resident(plain, d)
    view = tp.descriptor()
    i32, f64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    keep = []

    def xf(**over):
        out = tp.transform_descriptor()
        for k, v in over.items():
            setattr(out, k, v)
        return out

    def ints(v):
        keep.append(np.array(v, np.int32))
        return keep[-1].ctypes.data_as(i32)

    def doubles(v):
        keep.append(np.array(v, np.float64))
        return keep[-1].ctypes.data_as(f64)

    def lg(rows, d_=d, reserved=0):
        return _lib.CcListLogicle(d_, reserved, doubles(rows))

    c3 = cc.tolist()
    flat = inv.ravel().tolist()
    on = [list(V.LOGICLE)] * d
    none = [[0.0] * 4] * d
    cases = [("m < 0", xf(m=-1), None, "m must be"),
             ("m = 65", xf(m=65, comp_cols=ints(list(range(65))), comp=doubles(np.eye(65).ravel())), None, "m must be"),
             ("null comp_cols", xf(comp_cols=None), None, "null"),
             ("null comp", xf(comp=None), None, "null"),
             ("a column beyond the view's", xf(comp_cols=ints([c3[0], d, c3[2]])), None, "compensated column %d" % d),
             ("a negative column", xf(comp_cols=ints([c3[0], -1, c3[2]])), None, "compensated column -1"),
             ("a column that repeats", xf(comp_cols=ints([c3[0], c3[1], c3[0]])), None, "repeats"),
             ("a NaN matrix entry", xf(comp=doubles(flat[:4] + [np.nan] + flat[5:])), None, "not finite"),
             ("a negative cofactor", xf(cofactor=doubles([5, 5, -1, 5, 5, 5])), None, "cofactor 2"),
             ("an infinite cofactor", xf(cofactor=doubles([np.inf, 5, 5, 5, 5, 5])), None, "cofactor 0"),
             ("reserved", xf(reserved=1), None, "reserved"),
             ("logicle rows of another d", xf(cofactor=None), lg(on, d_=d + 1), "d is %d" % (d + 1)),
             ("logicle reserved", xf(cofactor=None), lg(on, reserved=1), "reserved"),
             ("a logicle row outside the contract", xf(cofactor=None), lg([[262144.0, 3.0, 4.5, 0.0]] + none[1:]), "dimension 0"),
             ("a cofactor and a logicle row", xf(), lg(none[:4] + [list(V.LOGICLE)] + none[5:]), "dimension 4 has a cofactor and a logicle scale")]
    before = plain.stats()
    mn, mx = np.zeros(d), np.zeros(d)
    uid, path = np.zeros(n, np.int64), np.zeros(n, np.int8)
    lib, hh = plain._lib, plain._h
    for what, t, g, reason in cases:
        gp = None if g is None else ctypes.byref(g)
        calls = [lib.cc_points_upload_view_xl(hh, ctypes.byref(view), ctypes.byref(t), gp, None, None),
                 lib.cc_points_prefetch_view_xl(hh, ctypes.byref(view), ctypes.byref(t), gp, None, None),
                 lib.cc_col_minmax_view_xl(hh, ctypes.byref(view), ctypes.byref(t), gp, _lib._ptr(mn), _lib._ptr(mx)),
                 lib.cc_online_view_xl(hh, ctypes.byref(view), ctypes.byref(t), gp, _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p)),
                 lib.cc_assign_view_xl(hh, ctypes.byref(view), ctypes.byref(t), gp, _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p), None)]
        assert calls == [-2] * 5, (what, calls)  # CC_ERR_BAD_ARG
        assert reason in lib.cc_last_error(hh).decode(), (what, lib.cc_last_error(hh))
    # the sibling's refusals stand beside them
    bad_view = tp.descriptor()
    bad_view.row_stride = 2
    good = xf()
    assert lib.cc_points_upload_view_xl(hh, ctypes.byref(bad_view), ctypes.byref(good), None, None, None) == -2
    assert "stride" in lib.cc_last_error(hh).decode()
    assert lib.cc_points_upload_view_xl(hh, ctypes.byref(view), ctypes.byref(good), None, _lib._ptr(mn), None) == -2
    # through Python: a ValueError
    with pytest.raises(ValueError, match="bad argument"):
        plain.points_upload(_lib.TransformedPoints(a, _lib.ListTransform(cc, inv, -1.0)))
    with pytest.raises(ValueError, match="compensated column %d" % d):
        plain.points_upload(_lib.TransformedPoints(a, _lib.ListTransform([0, d], np.eye(2))))
    # nothing moved, nothing was launched or counted
    after = plain.stats()
    for key in ("list_points", "view_points", "f32_points", "assign_launches", "assign_points", "scan_launches", "windows", "points"):
        assert after[key] == before[key], key
    x, xt = V.resident(plain, d)
    U.same_bits(x, held[0], "resident points behind refused calls")
    U.same_bits(xt, held[1], "resident points behind refused calls, dimension-major")
    # two nulls, and a transform that asks for nothing, are the sibling; the handle is as usable as before
    nothing = _lib.CcListTransform(0, 0, None, None, None)
    for t in (None, ctypes.byref(nothing)):
        plain._check(lib.cc_points_upload_view_xl(hh, ctypes.byref(view), t, None, None, None))
        U.same_bits(plain.points_download(d), V.widened(a), "no transform")
    against_the_referee(plain, a, tr, "behind the refusals")


# ---- 4. prefetch -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["f", "pitch"])
def test_prefetch_is_adopted_by_the_same_transform_only(seamed, layout):
    from chronoclust_amd import _lib
    handle = seamed
    n, d, m = 300, 13, 9
    a = V.laid_out(V.values(np.float32, n, d, 77), layout)
    cof = np.where(np.arange(d) % 2 == 0, 5.0, 0.0)
    rows = V.logicle_rows("all", d, cof)
    tr, cc, inv = V.transform(d, m, 8, cof, rows)
    tp = _lib.TransformedPoints(a, tr)

    def values(v):
        handle.points_upload(v)
        return handle.points_download(d)

    own = values(tp)
    before = handle.stats()["view_points"]
    handle.points_prefetch(tp)
    handle.points_upload(tp)  # adopted
    assert handle.stats()["view_points"] == before + n
    U.same_bits(one_value(handle, d, "prefetched")[0], own, "prefetched")
    # an equal transform built anew over the same array: adopted too
    handle.points_prefetch(tp)
    handle.points_upload(_lib.TransformedPoints(a, _lib.ListTransform(cc.copy(), inv.copy(), cof.copy(), rows.copy())))
    U.same_bits(handle.points_download(d), own, "an equal transform")
    other_inv = inv.copy()
    other_inv[4, 2] = np.nextafter(other_inv[4, 2], np.inf)  # (one bit of one matrix entry)
    other_cof = cof.copy()
    other_cof[2] = 6.0
    other_rows = rows.copy()
    other_rows[np.flatnonzero(rows[:, 0])[0]] = (262144.0, 1.0, 4.5, 0.0)
    variants = {"one matrix bit": _lib.ListTransform(cc, other_inv, cof, rows),
                "one cofactor": _lib.ListTransform(cc, inv, other_cof, rows),
                "one logicle row": _lib.ListTransform(cc, inv, cof, other_rows),
                "no logicle rows": _lib.ListTransform(cc, inv, cof),
                "no transform": None}
    for what, other_tr in variants.items():
        other = _lib.TransformedPoints(a, other_tr)
        assert other.points.ctypes.data == tp.points.ctypes.data
        want = values(other)
        assert not np.array_equal(want, own), what
        for first, second, exp in ((tp, other, want), (other, tp, own)):
            handle.points_prefetch(first)
            handle.points_upload(second)  # discarded: another transform
            U.same_bits(one_value(handle, d, what)[0], exp, "only %s differs" % what)
    # the plain view of the same array is another upload, in both directions
    handle.points_prefetch(tp)
    handle.points_upload(a)
    U.same_bits(handle.points_download(d), V.widened(a), "the plain view behind a transformed prefetch")
    handle.points_prefetch(a)
    handle.points_upload(tp)
    U.same_bits(handle.points_download(d), own, "the transformed view behind a plain prefetch")
    # scaled prefetch with a transform, adopted
    scale, min_ = np.full(d, 0.25), np.full(d, 0.5)
    handle.points_prefetch(tp, scale, min_)
    handle.points_upload_scaled(tp, scale, min_)
    U.same_bits(handle.points_download(d), own * scale + min_, "scaled prefetch")


# ---- 5. downstream: the same labels, tables and answers as the same values through `_list_xl` ------------------------------------------

def fortran_and_records(X, seed, logicle=False):
    """A Fortran-order float64 array whose transform gives (about) X - sinh(X) * 5 (or the logicle scale's inverse), the first
    dimensions spilled into each other - as TransformedPoints and as the referee's ListMode."""
    from chronoclust_amd import _lib
    n, d = X.shape
    m = max(1, min(d // 2, 9))
    spill, inv = U.spillover(m, seed)
    truth = L.inverse(X, *V.LOGICLE) if logicle else np.sinh(X) * 5.0
    truth[:, :m] = truth[:, :m] @ spill  # (building an input: any rounding will do)
    tr = _lib.ListTransform(np.arange(m), inv, None if logicle else 5.0, V.LOGICLE if logicle else None)
    a = np.asfortranarray(truth)
    return _lib.TransformedPoints(a, tr), V.referee_source(a, tr)


@pytest.mark.parametrize("d,prune,logicle", [(13, 2, False), (20, 2, True), (5, None, False)])
def test_the_online_phase_gives_the_list_routes_labels_and_tables(d, prune, logicle):
    import test_fcs_points as P
    n = 300
    cfg, Xs = P.stream(d, n)
    pairs = [fortran_and_records(X, 50 + t, logicle) for t, X in enumerate(Xs)]
    with knobs(**({} if prune is None else dict(CHRONOCLUST_HIP_PRUNE=prune))):
        _, exp = P.run_stream(cfg, [p[1] for p in pairs])
        _, got = P.run_stream(cfg, [p[0] for p in pairs])
    for t, (ra, rb) in enumerate(zip(got, exp)):
        assert np.abs(ra["resident"] - Xs[t]).max() < 1e-6, "the array does not hold the blobs"
        for key in ("uid", "path"):
            assert T._first_diff(ra[key], rb[key]) is None, (t, key)
        for kind in (0, 1):
            for key in T.KEYS:
                assert ra["tables"][kind][key].tobytes() == rb["tables"][kind][key].tobytes(), (t, kind, key)
        assert ra["counters"] == rb["counters"] and ra["members"] == rb["members"] and ra["points_of"] == rb["points_of"], t
        U.same_bits(ra["resident"], rb["resident"], "t=%d resident points" % t)
        for key, val in rb["stats"].items():
            if key not in P.TIME_FIELDS and key not in ("list_points", "view_points"):
                assert ra["stats"][key] == val, "t=%d cc_stats.%s: %r / %r" % (t, key, ra["stats"][key], val)
        assert ra["stats"]["view_points"] == n * (t + 1) and ra["stats"]["list_points"] == 0
    assert len(set(got[-1]["path"].tolist())) > 1, "every point took one path: nothing was compared"


def test_assign_gives_the_list_routes_answers():
    import test_fcs_points as P
    cfg, Xs = P.stream(13, 300)
    with knobs(CHRONOCLUST_HIP_ASSIGN_CHUNK=100, CHRONOCLUST_HIP_INGEST_SLAB=64):
        hdd, _ = P.run_stream(cfg, [Xs[0]])
    h = hdd._h
    q = np.vstack([Xs[0][:100], Xs[1][:65]])
    tp, lm = fortran_and_records(q, 9)
    exp = h.assign(lm, want_dist=True)
    before = h.stats()
    got = h.assign(tp, want_dist=True)
    after = h.stats()
    A.same_assign(got, exp, "a transformed Fortran array")
    U.same_bits(got[2], exp[2], "dist")
    assert after["assign_launches"] == 2 and after["assign_points"] == 165
    assert after["view_points"] == before["view_points"] + 165 and after["list_points"] == before["list_points"]
    assert len(set(got[1].tolist())) > 1, "the queries all took one path: nothing was compared"


def test_a_group_of_two_gives_the_single_handles_run():
    from chronoclust_amd import _lib
    pcores, outliers, par, X, meta = T.build_online("stale-3000+1096x20")
    tp, lm = fortran_and_records(X, 21)
    h = _lib.Handle(0)
    try:
        single = T.handle_online(h, (pcores, outliers, par, lm, meta))
        lists = [h.export(kind) for kind in (0, 1)]
        counters = h.counters()
    finally:
        h.close()
    hs, labels, stats = T.group_online(2, (pcores, outliers, par, tp, meta))
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
            assert stats[rank]["view_points"] == len(X) and stats[rank]["sharded_windows"] > 0, stats[rank]
    finally:
        for g in hs:
            g.close()
