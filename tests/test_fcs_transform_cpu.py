"""The host side of the list-mode transform, no GPU: the spillover keyword of an FCS file ($SPILLOVER / $SPILL / SPILL, names
matched against $PnN, every malformed form by its message), the $PnE / $PnG refusals, the `.transform` sidecar,
np.asarray(ListMode) with a transform against transform_util's independent restatement, the host-route fallback of a
mixed-width file, and read_fcs without the new arguments returning what it always returned."""
import json

import numpy as np
import pytest

import fcs_util as F
import transform_util as U
from chronoclust_amd import _lib, fcs

LITTLE, BIG = U.LITTLE, U.BIG
NAMES = ["Time", "FSC-A", "B515-A", "G560-A", "R660-A", "V450-A"]
FLUOR = ["G560-A", "B515-A", "V450-A"]  # (the matrix order is not the file's)


def f32_file(tmp_path, n=70, extra=None, name="a.fcs", **kw):
    rec = U.records(np.float32, n, len(NAMES), 3)
    fn = F.write_fcs(tmp_path / name, F.fast_records(rec, BIG), len(NAMES), "F", BIG, 32, names=NAMES, tot=n, extra=extra, **kw)
    return fn, rec


def expected(rec, cols, comp_cols, inv, cofactor=None, masks=None):
    x = U.decoded(rec, cols, masks)
    xs = U.comp_inputs(rec, cols, masks, comp_cols)
    v = U.compensated(x, xs, cols, comp_cols, inv) if len(comp_cols) else x
    return v if cofactor is None else U.with_cofactors(v, cofactor)


@pytest.mark.parametrize("key", ["$SPILLOVER", "$SPILL", "SPILL"])
def test_spillover_is_parsed_matched_and_inverted(tmp_path, key):
    spill, inv = U.spillover(3, 1)
    fn, rec = f32_file(tmp_path, extra={key: U.spillover_text(FLUOR, spill)})
    got_key, idx, got = fcs.parse_spillover(fcs.read_fcs(fn)[2], NAMES)
    assert got_key == key and idx == [NAMES.index(c) for c in FLUOR]
    U.same_bits(got, spill, "the matrix, row-major")
    lm, picked, _ = fcs.read_fcs(fn, columns=["V450-A", "FSC-A", "G560-A"], compensate=True)
    assert isinstance(lm, _lib.ListMode) and picked == ["V450-A", "FSC-A", "G560-A"]
    tr = lm.transform
    assert tr.m == 3 and tr.comp_cols.tolist() == idx and tr.cofactor is None
    U.same_bits(tr.comp, np.linalg.inv(spill), "the inverse")
    cols = [NAMES.index(c) for c in picked]
    U.same_bits(np.asarray(lm), expected(rec, cols, idx, tr.comp), "np.asarray(ListMode) against the restatement")
    assert np.asarray(lm).dtype == np.float64


def test_the_first_spelling_present_wins(tmp_path):
    spill = U.spillover(3, 1)[0]
    other = U.spillover(3, 2)[0]
    fn, _ = f32_file(tmp_path, extra={"SPILL": U.spillover_text(FLUOR, other), "$SPILLOVER": U.spillover_text(FLUOR, spill)})
    U.same_bits(fcs.read_fcs(fn, compensate=True)[0].transform.comp, np.linalg.inv(spill), "$SPILLOVER before SPILL")


@pytest.mark.parametrize("value,message", [
    (None, "none of"),
    ("x,B515-A,1", "channel count"),
    ("0", "names 0 channels"),
    ("2,B515-A,G560-A,1,0,0", "holds 6 fields"),
    ("2,B515-A,Nope-A,1,0,0,1", "Nope-A"),
    ("2,B515-A,B515-A,1,0,0,1", "twice"),
    ("2,B515-A,G560-A,1,0,zero,1", "no number"),
    ("2,B515-A,G560-A,1,nan,0,1", "not finite"),
    ("2,B515-A,G560-A,1,2,0.5,1", "singular"),
    (",".join(["65"] + ["c%d" % i for i in range(65)] + ["0"] * 65 * 65), "at most 64"),
])
def test_malformed_spillover_by_its_message(tmp_path, value, message):
    fn, _ = f32_file(tmp_path, extra=None if value is None else {"$SPILL": value})
    with pytest.raises(ValueError, match=message) as e:
        fcs.read_fcs(fn, compensate=True)
    assert "SPILL" in str(e.value)
    assert isinstance(fcs.read_fcs(fn)[0], _lib.ListMode)  # (nobody asked: nothing is refused)


def test_cofactors_by_number_and_by_name(tmp_path):
    fn, rec = f32_file(tmp_path)
    picked = ["R660-A", "Time", "B515-A"]
    cols = [NAMES.index(c) for c in picked]
    lm = fcs.read_fcs(fn, columns=picked, cofactor=150)[0]
    assert lm.transform.m == 0 and lm._cofactors.tolist() == [150.0] * 3
    got = np.asarray(lm)
    assert U.ulp_distance(got, expected(rec, cols, [], None, [150.0] * 3)).max() <= 1  # (numpy's own arcsinh: 1 ulp of the reference)
    lm = fcs.read_fcs(fn, columns=picked, cofactor={"B515-A": 5, "R660-A": 150.0})[0]
    assert lm._cofactors.tolist() == [150.0, 0.0, 5.0]
    got = np.asarray(lm)
    U.same_bits(got[:, 1], rec[:, cols[1]].astype(np.float64), "cofactor 0 passes through")
    U.same_bits(got[:, 2], np.arcsinh(rec[:, cols[2]].astype(np.float64) / 5.0), "np.arcsinh of one double division")
    for bad, message in (({"Nope": 5}, "Nope"), (-1, "negative"), (float("nan"), "not finite"), ({"Time": float("inf")}, "not finite")):
        with pytest.raises(ValueError, match=message):
            fcs.read_fcs(fn, columns=picked, cofactor=bad)


def test_amplified_channels_are_refused_once_a_transform_is_asked_for(tmp_path):
    spill = U.spillover(3, 1)[0]
    base = {"$SPILLOVER": U.spillover_text(FLUOR, spill)}
    v450 = NAMES.index("V450-A") + 1
    for extra, key in (({"$P%dE" % v450: "4,1"}, "P%dE" % v450), ({"$P%dG" % v450: "2"}, "P%dG" % v450),
                       ({"$P%dG" % v450: "fast"}, "P%dG" % v450)):
        fn, rec = f32_file(tmp_path, extra=dict(base, **extra))  # (a keyword given twice: the later one counts)
        plain = fcs.read_fcs(fn)[0]
        assert plain.transform is None  # (as stored, silently, as ever)
        # compensated though not selected; selected with a cofactor; neither: not refused
        with pytest.raises(ValueError, match=key) as e:
            fcs.read_fcs(fn, columns=["B515-A"], compensate=True)
        assert "V450-A" in str(e.value)
        with pytest.raises(ValueError, match=key):
            fcs.read_fcs(fn, columns=["V450-A", "Time"], cofactor=5)
        assert fcs.read_fcs(fn, columns=["Time", "FSC-A"], cofactor=5)[0].transform is not None
    fn, _ = f32_file(tmp_path, extra=dict(base, **{"$P%dG" % v450: "1.0"}))
    assert fcs.read_fcs(fn, compensate=True, cofactor=5)[0].transform.m == 3  # ($PnG 1: nothing to apply)


def test_the_sidecar(tmp_path):
    spill = U.spillover(3, 1)[0]
    fn, rec = f32_file(tmp_path, extra={"$SPILLOVER": U.spillover_text(FLUOR, spill)})
    assert fcs.sidecar_transform(fn) is None
    from chronoclust_amd.scaling.scaler import read_timepoint
    assert read_timepoint(fn).transform is None
    with open(fn + ".transform", "w") as f:
        json.dump({"compensate": True, "cofactor": {"B515-A": 5}}, f)
    assert fcs.sidecar_transform(fn) == dict(compensate=True, cofactor={"B515-A": 5})
    with open(fn + ".columns", "w") as f:
        f.write("B515-A\nFSC-A\n")
    lm = read_timepoint(fn)
    assert lm.shape == (70, 2) and lm.transform.m == 3 and lm._cofactors.tolist() == [5.0, 0.0]
    with open(fn + ".transform", "w") as f:
        json.dump({"cofactor": 150}, f)
    assert fcs.sidecar_transform(fn) == dict(compensate=False, cofactor=150)
    assert read_timepoint(fn).transform.m == 0
    for text, message in (("{", "not JSON"), ('{"compensate": 1}', "true or false"), ('{"cofactor": "5"}', "number"),
                          ('{"cofactor": {"B515-A": true}}', "number"), ('{"logicle": true}', "expected"), ("[]", "expected")):
        with open(fn + ".transform", "w") as f:
            f.write(text)
        with pytest.raises(ValueError, match=message):
            fcs.sidecar_transform(fn)


@pytest.mark.parametrize("dtype,order", [(t, o) for t in (np.float32, np.float64, np.uint16, np.uint8, np.uint32) for o in (LITTLE, BIG)])
def test_list_modes_host_transform_against_the_restatement(dtype, order):
    rng = np.random.default_rng(5)
    n, src_cols, m = 130, 20, 9
    rec = U.records(dtype, n, src_cols, 9)
    perm = rng.permutation(src_cols)
    comp_cols = perm[:m]
    cols = np.concatenate([comp_cols[[5, 2, 7]], perm[m:m + 4], comp_cols[[2]]])  # (an unselected rest, a repeat)
    masks = [0x3F, 0xFFFFFFFF, 0x7F, 0x1F, 0xFF, 0xFFFFFFFF, 0x0F, 0xFFFFFFFF] if np.dtype(dtype).kind == "u" else None
    inv = U.spillover(m, 4)[1]
    cof = np.array([5.0, 0.0, 150.0, 5.0, 0.0, 5.0, 5.0, 5.0])
    lm = U.list_mode(rec, order, cols, masks, _lib.ListTransform(comp_cols, inv))
    got = np.asarray(lm)
    assert got.dtype == np.float64
    U.same_bits(got, expected(rec, cols, comp_cols, inv, None, masks), "compensation alone: bit for bit")
    lm = U.list_mode(rec, order, cols, masks, _lib.ListTransform(comp_cols, inv, cof))
    got, ref = np.asarray(lm), expected(rec, cols, comp_cols, inv, cof, masks)
    assert U.ulp_distance(got, ref).max() <= 1
    U.same_bits(got[:, cof == 0], ref[:, cof == 0], "cofactor 0")
    assert np.asarray(lm, dtype=np.float32).dtype == np.float32
    # without a transform: what it always was
    lm = U.list_mode(rec, order, cols, masks)
    assert np.asarray(lm).dtype == (np.float32 if dtype == np.float32 else np.float64)
    U.same_bits(np.asarray(lm, np.float64), U.decoded(rec, cols, masks), "no transform")


def test_list_transform_checks_its_shapes():
    with pytest.raises(ValueError, match="go together"):
        _lib.ListTransform(comp_cols=[1, 2])
    with pytest.raises(ValueError, match=r"\[2, 2\]"):
        _lib.ListTransform([1, 2], np.eye(3))
    tr = _lib.ListTransform(cofactor=[5, 5, 5])
    with pytest.raises(ValueError, match="3 cofactors for 2"):
        _lib.ListMode(np.zeros(16, np.float32), 2, 4, np.float32, columns=[0, 1], transform=tr)
    with pytest.raises(ValueError, match="ListTransform"):
        _lib.ListMode(np.zeros(16, np.float32), 2, 4, np.float32, transform="asinh")
    assert _lib.ListMode(np.zeros(16, np.float32), 2, 4, np.float32).transform_descriptor() is None
    assert ctypes_sizes() == (32, 0, 4, 8, 16, 24)


def ctypes_sizes():
    t = _lib.CcListTransform
    return (__import__("ctypes").sizeof(t), t.m.offset, t.reserved.offset, t.comp_cols.offset, t.comp.offset, t.cofactor.offset)


def test_a_mixed_width_file_takes_the_host_route_with_the_transform_applied(tmp_path):
    n = 40
    rng = np.random.default_rng(2)
    values = rng.integers(0, 200, (n, 4))
    widths = [16, 8, 16, 32]
    names = ["A", "B", "C", "D"]
    spill = U.spillover(2, 6)[0]
    data = F.records(values.tolist(), "u", [w // 8 for w in widths], BIG)
    fn = F.write_fcs(tmp_path / "mixed.fcs", data, 4, "I", BIG, widths, names=names, tot=n, ranges=[256, 256, 256, 256],
                     extra={"$SPILLOVER": U.spillover_text(["C", "A"], spill)})
    plain = fcs.read_fcs(fn, columns=["D", "A", "B"])[0]
    assert isinstance(plain, np.ndarray) and plain.dtype == np.float64
    got = fcs.read_fcs(fn, columns=["D", "A", "B"], compensate=True, cofactor={"A": 5, "D": 5})[0]
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (n, 3)
    rec = values.astype(np.float64)
    ref = expected(rec, [3, 0, 1], [2, 0], np.linalg.inv(spill), [5.0, 5.0, 0.0])
    assert U.ulp_distance(got, ref).max() <= 1
    U.same_bits(got[:, 2], rec[:, 1], "an uncompensated channel without a cofactor")


def test_an_unselected_compensated_channel_that_needs_a_mask_takes_the_host_route(tmp_path):
    n = 30
    rec = U.records(np.uint16, n, 3, 1)
    spill = U.spillover(2, 6)[0]
    kw = dict(names=["A", "B", "C"], tot=n, extra={"$SPILLOVER": U.spillover_text(["A", "B"], spill)})
    fn = F.write_fcs(tmp_path / "m.fcs", F.fast_records(rec, BIG), 3, "I", BIG, 16, ranges=[1024, 1024, 65536], **kw)
    assert isinstance(fcs.read_fcs(fn, columns=["A", "B"], compensate=True)[0], _lib.ListMode)  # (selected: masked on the device)
    got = fcs.read_fcs(fn, columns=["A", "C"], compensate=True)[0]
    assert isinstance(got, np.ndarray)
    masked = rec & np.array([1023, 1023, 0xFFFF], np.uint16)
    U.same_bits(got, expected(masked, [0, 2], [0, 1], np.linalg.inv(spill)), "B under its range mask")


def test_read_fcs_without_the_new_arguments_is_what_it_was(tmp_path):
    spill = U.spillover(3, 1)[0]
    fn, rec = f32_file(tmp_path, extra={"$SPILLOVER": U.spillover_text(FLUOR, spill), "$P3G": "4"})
    lm, picked, text = fcs.read_fcs(fn, columns=["B515-A", "Time"])
    assert isinstance(lm, _lib.ListMode) and lm.transform is None and lm.transform_descriptor() is None
    assert picked == ["B515-A", "Time"] and "$SPILLOVER" in text
    got = np.asarray(lm)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), rec[:, [2, 0]].view(np.uint32))
    same = fcs.read_fcs(fn, columns=["B515-A", "Time"], compensate=False, cofactor=None)[0]
    assert same.transform is None and np.array_equal(np.asarray(same).view(np.uint32), got.view(np.uint32))
