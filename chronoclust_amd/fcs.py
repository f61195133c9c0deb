"""Flow Cytometry Standard files (FCS 2.0 / 3.0 / 3.1, list mode) read where they lie.

read_fcs memory-maps the file, parses HEADER and TEXT and hands the DATA segment out as a `_lib.ListMode` - the bytes the
file holds, in the file's byte order, every channel of an event interleaved - which Handle.points_upload and its kin move to
the device as they are: the byte swap, the selection of the channels, the `$PnR` range mask and the widening happen there
(cc_points_upload_list).  Layouts the device route does not take are decoded on the host into a float64 array.
With compensate / cofactor the file's own spillover matrix is inverted here and travels with the ListMode as a
`_lib.ListTransform`: the compensation and arcsinh(x / cofactor) happen on the device too (cc_points_upload_list_xf);
with logicle the channels of fluorescence flow cytometry take the logicle (biexponential) scale there instead, solved per value
(cc_points_upload_list_xl); sidecar_transform reads the `<file>.transform` that asks for them beside a timepoint of app.run.
estimate_logicle takes the width W of that scale from the events - the 5th percentile of a channel's negative compensated values,
pooled over the files of a series and selected on the device (Handle.negative_quantiles) -, estimate_sidecars for a whole run."""
import numpy as np

from ._lib import MAX_COMP, ListMode, ListTransform

VERSIONS = (b"FCS2.0", b"FCS3.0", b"FCS3.1")


def _header_offsets(head):
    """The six offsets of the HEADER: TEXT, DATA, ANALYSIS begin / end (end offsets inclusive; blank = 0)."""
    if len(head) < 58:
        raise ValueError("FCS HEADER: the file is shorter than the 58 bytes of a header")
    if head[:6] not in VERSIONS:
        raise ValueError("FCS HEADER: version %r is none of FCS2.0, FCS3.0, FCS3.1" % head[:6])
    out = []
    for i in range(6):
        field = head[10 + 8 * i:18 + 8 * i].strip()
        try:
            out.append(int(field) if field else 0)
        except ValueError:
            raise ValueError("FCS HEADER: offset %d is %r, not a number" % (i, field)) from None
        if out[-1] < 0:
            raise ValueError("FCS HEADER: offset %d is negative" % i)
    return out


def parse_text(segment):
    """The TEXT segment as a dict, keywords upper-cased: the first byte is the delimiter, keywords and values alternate, a
    doubled delimiter inside a keyword or value is a literal one (so no value is empty)."""
    if len(segment) < 2:
        raise ValueError("FCS TEXT: the segment is empty")
    delim = segment[0:1]
    tokens, cur, i, n = [], bytearray(), 1, len(segment)
    while i < n:
        c = segment[i:i + 1]
        if c == delim:
            if segment[i + 1:i + 2] == delim:
                cur += delim
                i += 2
                continue
            tokens.append(bytes(cur))
            cur = bytearray()
        else:
            cur += c
        i += 1
    if cur.strip(b" \x00\r\n"):
        tokens.append(bytes(cur))  # (a last value without its closing delimiter)
    if len(tokens) % 2:
        raise ValueError("FCS TEXT: keyword %r has no value" % tokens[-1].decode("latin-1"))
    text = {}
    for k, v in zip(tokens[0::2], tokens[1::2]):
        text[k.decode("latin-1").strip().upper()] = v.decode("latin-1")
    return text


def _need(text, key):
    if key not in text:
        raise ValueError("FCS TEXT: %s is missing" % key)
    return text[key].strip()


def _int(text, key):
    val = _need(text, key)
    try:
        return int(val)
    except ValueError:
        try:
            f = float(val)
            if f == int(f):
                return int(f)
        except ValueError:
            pass
        raise ValueError("FCS TEXT: %s is %r, not an integer" % (key, val)) from None


def range_mask(pnr, bits):
    """The AND mask of an integer channel of `bits` bits whose $PnR is pnr: 2^ceil(log2(pnr)) - 1 where that is below the
    all-ones of the channel's width, else None."""
    m = (1 << max(int(pnr) - 1, 0).bit_length()) - 1
    return m if m < (1 << bits) - 1 else None


def _select(columns, names, stains):
    if columns is None:
        return list(range(len(names)))
    out = []
    for c in columns:
        if isinstance(c, (int, np.integer)):
            if not 0 <= int(c) < len(names):
                raise ValueError("FCS: column index %d is outside 0..%d" % (c, len(names) - 1))
            out.append(int(c))
        elif c in names:
            out.append(names.index(c))
        elif c in stains:
            out.append(stains.index(c))
        else:
            raise ValueError("FCS: no channel whose $PnN or $PnS is %r (channels: %s)" % (c, ", ".join(names)))
    if not out:
        raise ValueError("FCS: the column list is empty")
    return out


def _host_decode(raw, tot, par, datatype, widths, order, masks):
    """[tot, par] float64 of a list-mode layout the device route does not take: channel widths that differ or are no 8, 16 or
    32 bits (whole bytes up to 64 bits), byte orders that are a permutation of the element's bytes."""
    ascending, descending = order == sorted(order), order == sorted(order, reverse=True)
    nbytes = [w // 8 for w in widths]
    rec = np.frombuffer(raw, dtype=np.uint8, count=tot * sum(nbytes)).reshape(tot, sum(nbytes))
    out = np.empty((tot, par), np.float64)
    at = 0
    for c, nb in enumerate(nbytes):
        field = rec[:, at:at + nb]
        at += nb
        if ascending or descending:
            sig = list(range(nb)) if ascending else list(range(nb - 1, -1, -1))
        elif len(order) == nb:
            sig = [o - 1 for o in order]
        else:
            raise ValueError("FCS TEXT: $BYTEORD %s does not describe an element of %d bytes ($P%dB)"
                             % (",".join(map(str, order)), nb, c + 1))
        le = np.zeros((tot, 8), np.uint8)  # the element's bytes, least significant first
        for i, s in enumerate(sig):
            le[:, s] = field[:, i]
        if datatype == "I":
            val = le.view("<u8")[:, 0]
            out[:, c] = (val if masks[c] is None else val & np.uint64(masks[c])).astype(np.float64)
        elif nb == 4:
            out[:, c] = np.ascontiguousarray(le[:, :4]).view("<f4")[:, 0]
        else:
            out[:, c] = le.view("<f8")[:, 0]
    return out


SPILLOVER_KEYWORDS = ("$SPILLOVER", "$SPILL", "SPILL")


def parse_spillover(text, names):
    """(keyword, channel indices, spillover matrix [n, n]) of the file's own spillover keyword - $SPILLOVER, else $SPILL, else
    SPILL: `n,name_1..name_n,` and n * n values, row-major; the names matched against `names` (the $PnN).  ValueError naming
    the keyword where it is absent, malformed or names an unknown channel."""
    key = next((k for k in SPILLOVER_KEYWORDS if k in text), None)
    if key is None:
        raise ValueError("FCS TEXT: compensation asked for, but none of %s is present" % ", ".join(SPILLOVER_KEYWORDS))
    fields = [f.strip() for f in text[key].split(",")]
    try:
        n = int(fields[0])
    except ValueError:
        raise ValueError("FCS TEXT: %s does not begin with a channel count (%r)" % (key, fields[0])) from None
    if n < 1:
        raise ValueError("FCS TEXT: %s names %d channels" % (key, n))
    if n > MAX_COMP:
        raise ValueError("FCS TEXT: %s names %d channels, at most %d are taken" % (key, n, MAX_COMP))
    if len(fields) != 1 + n + n * n:
        raise ValueError("FCS TEXT: %s holds %d fields, %d channels need %d" % (key, len(fields), n, 1 + n + n * n))
    idx = []
    for name in fields[1:1 + n]:
        if name not in names:
            raise ValueError("FCS TEXT: %s names channel %r, which is no $PnN (channels: %s)" % (key, name, ", ".join(names)))
        idx.append(names.index(name))
    if len(set(idx)) != n:
        raise ValueError("FCS TEXT: %s names a channel twice" % key)
    try:
        values = [float(v) for v in fields[1 + n:]]
    except ValueError:
        raise ValueError("FCS TEXT: %s holds a value that is no number" % key) from None
    spill = np.array(values, np.float64).reshape(n, n)
    if not np.isfinite(spill).all():
        raise ValueError("FCS TEXT: %s holds a value that is not finite" % key)
    return key, idx, spill


def _compensation(text, names):
    """(channel indices, inverse spillover matrix) for read_fcs(compensate=True)."""
    key, idx, spill = parse_spillover(text, names)
    return idx, invert_spillover(spill, "FCS TEXT: the matrix of %s" % key)


def invert_spillover(spill, what):
    """The inverse of a spillover matrix (numpy.linalg.inv) as the transform takes it - the one place it is inverted, for the
    file's own keyword (read_fcs) and for a sidecar's "spillover" (array_transform).  ValueError `what` is singular."""
    try:
        inv = np.linalg.inv(spill)
    except np.linalg.LinAlgError:
        raise ValueError("%s is singular" % what) from None
    if not np.isfinite(inv).all():
        raise ValueError("%s is singular" % what)
    return np.ascontiguousarray(inv)


def _cofactors(cofactor, picked):
    """One cofactor per selected channel: a number for all, or a dict from channel name to number (unnamed channels: 0)."""
    if cofactor is None:
        return None
    if isinstance(cofactor, dict):
        unknown = [k for k in cofactor if k not in picked]
        if unknown:
            raise ValueError("FCS: cofactor names %r, which is no selected channel (selected: %s)" % (unknown[0], ", ".join(picked)))
        out = np.array([float(cofactor.get(name, 0.0)) for name in picked], np.float64)
    else:
        out = np.full(len(picked), float(cofactor), np.float64)
    if not np.isfinite(out).all() or (out < 0).any():
        raise ValueError("FCS: a cofactor is negative or not finite")
    return out


LOGICLE_KEYS = ("T", "W", "M", "A")
LOGICLE_DEFAULTS = dict(W=0.5, M=4.5, A=0.0)  # (T: the channel's $PnR)


ESTIMATE = "estimate"  # a row's W that estimate_logicle resolves from the events


def _is_logicle_row(spec):
    """True for {"T": number, "W": ..., "M": ..., "A": ...}, every key optional: the parameters of one logicle scale.  W may be
    the string "estimate" - the width is then taken from the events (estimate_logicle) -, and only beside it "q": number, the
    quantile of the negative values it is taken at."""
    if not isinstance(spec, dict) or not set(spec) <= set(LOGICLE_KEYS) | {"q"}:
        return False
    unresolved = _is_unresolved(spec)
    if "q" in spec and not unresolved:
        return False
    return all((isinstance(v, (int, float)) and not isinstance(v, bool)) or (k == "W" and unresolved) for k, v in spec.items())


def _is_unresolved(row):
    return isinstance(row.get("W"), str) and row["W"] == ESTIMATE


def _is_logicle_spec(spec):
    """True for the two forms `logicle` takes: one row for every channel, or {channel name: row}."""
    return _is_logicle_row(spec) or (isinstance(spec, dict) and len(spec) > 0 and all(_is_logicle_row(v) for v in spec.values()))


def _logicles(logicle, picked, sel, cof, text):
    """[d, 4] rows T, W, M, A, one per selected channel (T == 0: off the scale), or None.  One row: every selected channel
    without a cofactor; by name: the channels named - one that has a cofactor too is refused.  An omitted T is the channel's
    $PnR, W 0.5, M 4.5, A 0."""
    if logicle is None:
        return None
    if not _is_logicle_spec(logicle):
        raise ValueError("FCS: logicle must be {T, W, M, A: number} (every key optional) or {channel name: such an object}")
    by_name = not _is_logicle_row(logicle)
    if by_name:
        unknown = [k for k in logicle if k not in picked]
        if unknown:
            raise ValueError("FCS: logicle names %r, which is no selected channel (selected: %s)" % (unknown[0], ", ".join(picked)))
    out = np.zeros((len(picked), 4), np.float64)
    for k, name in enumerate(picked):
        has_cof = cof is not None and cof[k] > 0
        if by_name:
            if name not in logicle:
                continue
            if has_cof:
                raise ValueError("FCS: channel %s has a cofactor and a logicle scale: it takes one or the other" % name)
            row = logicle[name]
        elif has_cof:
            continue
        else:
            row = logicle
        if _is_unresolved(row):
            raise ValueError('FCS: the logicle scale of channel %s has "W": "estimate": read_fcs does not look at the events - '
                             "resolve the width with estimate_logicle first (over every file of the series) and pass its rows" % name)
        T = float(row["T"]) if "T" in row else float(_need(text, "$P%dR" % (sel[k] + 1)))
        out[k] = [T] + [float(row.get(key, LOGICLE_DEFAULTS[key])) for key in LOGICLE_KEYS[1:]]
        if not out[k, 0] > 0 or not np.isfinite(out[k]).all():
            raise ValueError("FCS: the logicle scale of channel %s needs a positive, finite T (%r) and finite W, M, A" % (name, T))
    return out


def _refuse_amplified(text, channels, names):
    """With a transform asked for, $PnE other than 0,0 and $PnG other than 1 stay unapplied - but no longer silently."""
    for c in channels:
        e = text.get("$P%dE" % (c + 1))
        if e is not None:
            try:
                flat = [float(v) for v in e.split(",")] == [0.0, 0.0]
            except ValueError:
                flat = False
            if not flat:
                raise ValueError("FCS TEXT: $P%dE is %s (channel %s): logarithmic amplification is not applied, so the channel "
                                 "takes no compensation or cofactor" % (c + 1, e.strip(), names[c]))
        g = text.get("$P%dG" % (c + 1))
        if g is not None:
            try:
                unit = float(g) == 1.0
            except ValueError:
                unit = False
            if not unit:
                raise ValueError("FCS TEXT: $P%dG is %s (channel %s): linear gain is not applied, so the channel takes no "
                                 "compensation or cofactor" % (c + 1, g.strip(), names[c]))


def read_fcs(path, columns=None, compensate=False, cofactor=None, logicle=None):
    """(points, names, text) of a list-mode FCS file.

    points: the DATA segment as a `_lib.ListMode` over the memory-mapped file - nothing is decoded or copied on the host -
    when $DATATYPE is F (32 bits) or D (64 bits), or I with every $PnB equal and 8, 16 or 32, $BYTEORD is 1,2,3,4 or 4,3,2,1
    (or 1,2 / 2,1) and the segment holds at least $TOT * $PAR elements.  For I the mask of a channel is
    2^ceil(log2($PnR)) - 1 where that is below the all-ones of $PnB bits.  Any other list-mode layout - $PnB that differ,
    24 / 40 / 48 / 56 / 64-bit integers, byte orders such as 3,4,1,2 - comes back decoded on the host as a float64 ndarray
    [n, d], which takes the routes an ndarray has always taken.
    columns: the channels to take, in this order - names matched against $PnN, then $PnS, or indices; None: all, in file order.
    names: the $PnN of the channels taken.  text: the TEXT segment's keywords (upper-cased) and values.
    The values are the channel values AS STORED: the amplification keywords $PnE (logarithmic decades) and $PnG (linear gain)
    are NOT applied.
    compensate: the file's own spillover matrix ($SPILLOVER, else $SPILL, else SPILL: `n,name_1..name_n,` and n * n values,
    row-major, the names matched against $PnN) is inverted (numpy.linalg.inv) and the channels it names are compensated -
    whether they are selected or not, every one of them is read.  cofactor: a number for every selected channel or a dict
    from channel name ($PnN of a selected channel) to number, unnamed channels 0 - arcsinh(value / cofactor) where it is
    positive, the value as it is where it is 0 (5 for mass cytometry, about 150 for flow).  With either, `points` is a
    ListMode with that transform (`_lib.ListTransform`: applied on the device as the events land), or, for a layout that
    takes the host route, the float64 array with the transform applied on the host; a selected or compensated channel whose
    $PnE is not 0,0 or whose $PnG is present and not 1 is a ValueError naming it, and so is a spillover keyword that is
    absent, malformed, names an unknown channel or holds a singular matrix.  Without either nothing changes.
    logicle: the logicle (biexponential) scale of fluorescence flow cytometry (Moore and Parks 2012), after the compensation, on
    the unit display scale (T maps to 1, 0 to (A + W) / (M + A)) - {"T": .., "W": .., "M": .., "A": ..} for every selected
    channel that has no cofactor, or {channel name: {...}} per channel; an omitted T is the channel's $PnR, W 0.5, M 4.5, A 0.
    A channel takes a cofactor or the logicle scale: one that is given both by name is a ValueError, as are parameters outside
    T > 0, M > 0, 0 <= W, 2 W <= M, -W <= A <= M - 2 W.  $PnE and $PnG are refused as for a cofactor.  The scale is solved on
    the device as the events land (cc_points_upload_list_xl), or on the host for a layout that takes the host route.
    A row whose W is "estimate" is a ValueError that names estimate_logicle: this function never looks at the events, and the
    width of a series is one number over all its files - resolve it there and pass the rows it returns.
    ValueError naming the keyword for: $DATATYPE A, a $MODE other than L, a DATA segment shorter than $TOT * $PAR elements,
    channel widths that are no whole bytes, a malformed HEADER or TEXT."""
    mm = np.memmap(path, dtype=np.uint8, mode="c")  # (copy-on-write: the pages are the file's until somebody writes, nobody does)
    size = mm.size
    text_lo, text_hi, data_lo, data_hi = _header_offsets(bytes(mm[:58]))[:4]
    if not 58 <= text_lo <= text_hi < size:
        raise ValueError("FCS HEADER: the TEXT offsets %d..%d lie outside the file (%d bytes)" % (text_lo, text_hi, size))
    text = parse_text(bytes(mm[text_lo:text_hi + 1]))
    if data_lo == 0 and data_hi == 0:  # (files beyond 99 999 999 bytes: the header's fields are too narrow)
        data_lo, data_hi = _int(text, "$BEGINDATA"), _int(text, "$ENDDATA")
    mode = _need(text, "$MODE").upper()
    if mode != "L":
        raise ValueError("FCS TEXT: $MODE %s is not list mode (L)" % mode)
    datatype = _need(text, "$DATATYPE").upper()
    if datatype not in ("I", "F", "D"):
        raise ValueError("FCS TEXT: $DATATYPE %s is not taken (I, F and D are)" % datatype)
    par = _int(text, "$PAR")
    if par < 1:
        raise ValueError("FCS TEXT: $PAR is %d" % par)
    byteord = _need(text, "$BYTEORD")
    try:
        order = [int(v) for v in byteord.split(",")]
    except ValueError:
        raise ValueError("FCS TEXT: $BYTEORD is %r" % byteord) from None
    if sorted(order) != list(range(1, len(order) + 1)):
        raise ValueError("FCS TEXT: $BYTEORD %s is no permutation of 1..%d" % (text["$BYTEORD"], len(order)))
    widths = [_int(text, "$P%dB" % (i + 1)) for i in range(par)]
    names = [text.get("$P%dN" % (i + 1), "P%d" % (i + 1)).strip() for i in range(par)]
    stains = [text.get("$P%dS" % (i + 1), "").strip() for i in range(par)]
    if datatype in ("F", "D"):
        want = 32 if datatype == "F" else 64
        for i, w in enumerate(widths):
            if w != want:
                raise ValueError("FCS TEXT: $P%dB is %d with $DATATYPE %s (%d bits)" % (i + 1, w, datatype, want))
    for i, w in enumerate(widths):
        if w % 8 or not 8 <= w <= 64:
            raise ValueError("FCS TEXT: $P%dB is %d: channels of whole bytes up to 64 bits are taken" % (i + 1, w))
    event_bytes = sum(widths) // 8
    if not 0 < data_lo <= data_hi < size:
        if not (data_lo == 0 and data_hi == 0 and "$TOT" in text and _int(text, "$TOT") == 0):
            raise ValueError("FCS HEADER: the DATA offsets %d..%d ($BEGINDATA / $ENDDATA) lie outside the file (%d bytes)"
                             % (data_lo, data_hi, size))
    held = (data_hi - data_lo + 1) // event_bytes if data_hi else 0
    tot = _int(text, "$TOT") if "$TOT" in text else held  # (FCS 2.0 may omit it: what the segment holds)
    if tot < 0 or tot > held:
        raise ValueError("FCS TEXT: $TOT %d x $PAR %d elements need %d bytes, the DATA segment %d..%d holds %d"
                         % (tot, par, tot * event_bytes, data_lo, data_hi, data_hi - data_lo + 1 if data_hi else 0))
    sel = _select(columns, names, stains)
    picked = [names[c] for c in sel]
    raw = mm[data_lo:data_lo + tot * event_bytes]
    transform = comp_idx = None
    if compensate or cofactor is not None or logicle is not None:
        comp_idx, inv = _compensation(text, names) if compensate else ([], None)
        cof = _cofactors(cofactor, picked)
        _refuse_amplified(text, list(dict.fromkeys(sel + comp_idx)), names)
        rows = _logicles(logicle, picked, sel, cof, text)
        try:
            transform = ListTransform(comp_cols=comp_idx if compensate else None, comp=inv, cofactor=cof, logicle=rows)
        except ValueError as e:
            raise ValueError("FCS: %s" % e) from None
    ascending, descending = order == sorted(order), order == sorted(order, reverse=True)
    uniform = len(set(widths)) == 1 and widths[0] in ((32,) if datatype == "F" else (64,) if datatype == "D" else (8, 16, 32))
    if uniform and (ascending or descending):
        kind = {"F": "f4", "D": "f8"}.get(datatype) or "u%d" % (widths[0] // 8)
        dtype = np.dtype(("<" if ascending else ">") + kind)
        masks = None
        if datatype == "I":
            got = [range_mask(_int(text, "$P%dR" % (c + 1)), widths[0]) for c in sel]
            if any(m is not None for m in got):
                masks = [0xFFFFFFFF if m is None else m for m in got]
            # (a compensated channel that is not selected is read without a mask on the device: where its range asks for
            # one, the file takes the host route below)
            if any(c not in sel and range_mask(_int(text, "$P%dR" % (c + 1)), widths[0]) is not None for c in comp_idx or ()):
                uniform = False
    if uniform and (ascending or descending):
        return ListMode(raw, tot, par, dtype, columns=sel, masks=masks, transform=transform), picked, text
    # the layouts of old, on the host
    masks = [range_mask(_int(text, "$P%dR" % (c + 1)), widths[c]) if datatype == "I" else None for c in range(par)]
    out = _host_decode(raw, tot, par, datatype, widths, order, masks)
    if transform is not None:
        # the host transform of ListMode, over the decoded channels: a native float64 record of every channel
        return np.asarray(ListMode(np.ascontiguousarray(out), tot, par, np.float64, columns=sel, transform=transform)), picked, text
    return np.ascontiguousarray(out[:, sel]), picked, text


def sidecar_columns(path):
    """The names in `<file>.columns` (one per line, the `.npy` convention), or None without that file."""
    import os
    names_file = str(path) + ".columns"
    if not os.path.exists(names_file):
        return None
    with open(names_file) as f:
        return [line.strip() for line in f if line.strip()]


def sidecar_transform(path):
    """The transform in `<file>.transform`, as keyword arguments of read_fcs, or None without that file.  The file is JSON:
    {"compensate": bool, "cofactor": number | {channel name: number}, "logicle": {"T": number, "W": .., "M": .., "A": ..} |
    {channel name: {...}}}, every key optional (and every key of a logicle object: read_fcs has the defaults); the returned
    dict carries "logicle" only where the file does.  A logicle object's W may be "estimate", with an optional "q" beside it:
    the width is then taken from the events of the whole run (estimate_sidecars, which app.run calls).
    Beside a `.csv` or `.npy` timepoint one more key is taken, "spillover": {"channels": [names], "matrix": [[...]]} - square,
    finite, one row and one column per channel -, the matrix "compensate" then inverts (array_transform): such a file has no
    $SPILLOVER of its own.  The returned dict carries it only where the file does.  Beside an `.fcs` file the key is refused:
    the file's own spillover keyword is the contract there."""
    import json
    import os
    name = str(path) + ".transform"
    if not os.path.exists(name):
        return None
    with open(name) as f:
        try:
            spec = json.load(f)
        except ValueError as e:
            raise ValueError("%s: not JSON (%s)" % (name, e)) from None
    if isinstance(spec, dict) and "spillover" in spec and str(path).lower().endswith(".fcs"):
        raise ValueError('%s: "spillover" is for .csv and .npy timepoints; an .fcs file is compensated by its own spillover '
                         'keyword (%s)' % (name, ", ".join(SPILLOVER_KEYWORDS)))
    if not isinstance(spec, dict) or set(spec) - {"compensate", "cofactor", "logicle", "spillover"} or \
            ("logicle" in spec and not _is_logicle_spec(spec["logicle"])):
        raise ValueError('%s: expected {"compensate": bool, "cofactor": number or {name: number}, "logicle": {T, W, M, A: number} '
                         'or {name: {T, W, M, A: number}}}' % name)
    compensate, cofactor = spec.get("compensate", False), spec.get("cofactor")
    if not isinstance(compensate, bool):
        raise ValueError("%s: compensate must be true or false" % name)
    numbers = list(cofactor.values()) if isinstance(cofactor, dict) else [] if cofactor is None else [cofactor]
    if any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in numbers):
        raise ValueError("%s: cofactor must be a number or an object of channel name: number" % name)
    out = dict(compensate=compensate, cofactor=cofactor)
    if "logicle" in spec:
        out["logicle"] = spec["logicle"]
    if "spillover" in spec:
        out["spillover"] = _sidecar_spillover(name, spec["spillover"])
    return out


def _sidecar_spillover(name, spill):
    """(channel names, matrix [n, n]) of a sidecar's "spillover" object; ValueError naming the key for a malformed one."""
    ok = isinstance(spill, dict) and set(spill) == {"channels", "matrix"} and isinstance(spill["channels"], list) and \
        len(spill["channels"]) > 0 and all(isinstance(c, str) for c in spill["channels"]) and isinstance(spill["matrix"], list)
    if not ok:
        raise ValueError('%s: "spillover" must be {"channels": [names], "matrix": [[numbers]]}' % name)
    n = len(spill["channels"])
    if n > MAX_COMP:
        raise ValueError('%s: "spillover" names %d channels, at most %d are taken' % (name, n, MAX_COMP))
    if len(set(spill["channels"])) != n:
        raise ValueError('%s: "spillover" names a channel twice' % name)
    rows = spill["matrix"]
    if len(rows) != n or any(not isinstance(r, list) or len(r) != n for r in rows):
        raise ValueError('%s: the matrix of "spillover" is not square: %d channels need %d rows of %d numbers' % (name, n, n, n))
    if any(isinstance(v, bool) or not isinstance(v, (int, float)) for r in rows for v in r):
        raise ValueError('%s: the matrix of "spillover" holds a value that is no number' % name)
    matrix = np.array(rows, np.float64).reshape(n, n)
    if not np.isfinite(matrix).all():
        raise ValueError('%s: the matrix of "spillover" holds a value that is not finite' % name)
    return list(spill["channels"]), matrix


def array_transform(path, names, compensate=False, cofactor=None, logicle=None, spillover=None):
    """The `_lib.ListTransform` a `.csv` or `.npy` timepoint's sidecar asks for (sidecar_transform's keywords), over the
    array's columns `names` - the CSV header, `<file>.columns` for a `.npy` -, or None where it asks for nothing: what
    read_fcs builds for an `.fcs` file from its TEXT segment.  compensate needs "spillover" - there is no $SPILLOVER to read -,
    whose channels are matched against `names` and whose matrix is inverted by the function read_fcs uses; cofactor and
    logicle by name resolve against `names`; a logicle row must carry T - there is no $PnR to default to - and a W of
    "estimate" is refused: the estimate selects over list-mode events only.  ValueError naming the key or the channel."""
    name = str(path) + ".transform"
    names = list(names)
    comp_idx = inv = None
    if compensate:
        if spillover is None:
            raise ValueError('%s: "compensate" needs "spillover": {"channels": [names], "matrix": [[...]]} - a .csv or .npy '
                             'timepoint has no spillover keyword of its own' % name)
        channels, matrix = spillover
        for ch in channels:
            if ch not in names:
                raise ValueError('%s: "spillover" names channel %r, which is no column (columns: %s)' % (name, ch, ", ".join(names)))
        comp_idx = [names.index(ch) for ch in channels]
        inv = invert_spillover(matrix, '%s: the matrix of "spillover"' % name)
    try:
        cof = _cofactors(cofactor, names)
    except ValueError as e:
        raise ValueError("%s: %s" % (name, e)) from None
    rows = None
    if logicle is not None:
        if not _is_logicle_spec(logicle):
            raise ValueError("%s: logicle must be {T, W, M, A: number} or {channel name: such an object}" % name)
        by_name = not _is_logicle_row(logicle)
        for k, ch in enumerate(names):
            row = logicle.get(ch) if by_name else (None if cof is not None and cof[k] > 0 else logicle)
            if row is None:
                continue
            if _is_unresolved(row):
                raise ValueError('%s: the logicle scale of channel %s has "W": "estimate": the width is estimated from list-mode '
                                 '(.fcs) events only, not for .csv or .npy timepoints - give W as a number' % (name, ch))
            if "T" not in row:
                raise ValueError('%s: the logicle scale of channel %s needs "T": a .csv or .npy timepoint has no $PnR to take '
                                 "it from" % (name, ch))
        try:
            rows = _logicles(logicle, names, list(range(len(names))), cof, {})
        except ValueError as e:
            raise ValueError("%s: %s" % (name, e)) from None
    if comp_idx is None and cof is None and (rows is None or not (rows[:, 0] != 0).any()):
        return None
    try:
        return ListTransform(comp_cols=comp_idx, comp=inv, cofactor=cof, logicle=rows)
    except ValueError as e:
        raise ValueError("%s: %s" % (name, e)) from None


def logicle_w(count, lo, hi, frac, T, M):
    """The logicle width of Parks, Roederer and Moore 2006 from the order statistics of a channel's negative compensated values
    (Handle.negative_quantiles): r = numpy's linear interpolation of (lo, hi) at frac - np.quantile of the negative values -,
    W = (M - log10(T / |r|)) / 2 clamped to [0, M / 2]; 0 where there is no negative value (count == 0).  ValueError where r
    is -Inf."""
    if int(count) == 0:
        return 0.0
    with np.errstate(all="ignore"):
        r = np.quantile(np.array([lo, hi], np.float64), np.float64(frac))
        if np.isinf(lo) or not np.isfinite(r):
            raise ValueError("the quantile of the negative values is not finite (%r)" % float(lo))
        T, M = np.float64(T), np.float64(M)
        W = (M - np.log10(T / np.abs(r))) / 2
    return float(min(max(W, np.float64(0.0)), M / 2))


def _channels(text, columns):
    """(indices, $PnN of all channels) of the channels read_fcs takes for `columns`."""
    par = _int(text, "$PAR")
    names = [text.get("$P%dN" % (i + 1), "P%d" % (i + 1)).strip() for i in range(par)]
    stains = [text.get("$P%dS" % (i + 1), "").strip() for i in range(par)]
    return _select(columns, names, stains), names


def estimate_logicle(paths, columns=None, compensate=False, logicle=None, q=0.05, handle=None):
    """{channel name: {"T": .., "W": .., "M": .., "A": ..}}: the rows of `logicle` (read_fcs's two forms: one row for every
    selected channel, or {channel name: row}) resolved over the files `paths`, POOLED - a time series takes one W per channel
    over all its timepoints.  A row whose W is "estimate" gets W = (M - log10(T / |r|)) / 2, clamped to [0, M / 2], r the
    quantile q (the row's own "q", else `q`: 0.05) of the channel's NEGATIVE values after compensation - no negative value:
    W = 0 -; a row with a numeric W passes through with the defaults filled in (T: the channel's $PnR, M 4.5, A 0).
    handle: a `_lib.Handle` - the events stream through its staging and the order statistics are selected on the device
    (Handle.negative_quantiles), nothing is decoded on the host; None: the same answer on the host, bit for bit.  Files of the
    layouts read_fcs decodes on the host are handed on as native float64 records and pool with the rest.
    ValueError where the files disagree on a channel's T, M or A or on the channels themselves, where a named channel is
    missing from a file, for $PnE / $PnG as in read_fcs, for q outside [0, 1], for a quantile of -Inf (naming the channel) and
    for a resolved row outside the logicle scale's contract."""
    from . import _lib
    if logicle is None or not _is_logicle_spec(logicle):
        raise ValueError('FCS: logicle must be {T, W, M, A: number, W may be "estimate"} or {channel name: such an object}')
    paths = list(paths)
    if not paths:
        raise ValueError("FCS: estimate_logicle needs at least one file")
    by_name = not _is_logicle_row(logicle)
    sources, first, first_picked = [], None, None
    for path in paths:
        points, picked, text = read_fcs(path, columns=columns, compensate=compensate)
        sel, names = _channels(text, columns)
        _refuse_amplified(text, sel, names)
        if first_picked is None:
            first_picked = picked
        elif picked != first_picked:
            raise ValueError("FCS: %s holds the channels %s, the files before it %s" % (path, ", ".join(picked), ", ".join(first_picked)))
        if by_name:
            unknown = [k for k in logicle if k not in picked]
            if unknown:
                raise ValueError("FCS: logicle names %r, which is no selected channel of %s (selected: %s)"
                                 % (unknown[0], path, ", ".join(picked)))
        rows = {}
        for k, name in enumerate(picked):
            row = logicle.get(name) if by_name else logicle
            if row is None:
                continue
            T = float(row["T"]) if "T" in row else float(_need(text, "$P%dR" % (sel[k] + 1)))
            W = row.get("W", LOGICLE_DEFAULTS["W"])
            rows[name] = dict(T=T, W=W if _is_unresolved(row) else float(W), M=float(row.get("M", LOGICLE_DEFAULTS["M"])),
                              A=float(row.get("A", LOGICLE_DEFAULTS["A"])), q=float(row.get("q", q)), k=k)
            if not 0.0 <= rows[name]["q"] <= 1.0:
                raise ValueError("FCS: the quantile of channel %s must be in [0, 1] (%r)" % (name, rows[name]["q"]))
        if first is None:
            first = rows
        for name, row in rows.items():
            for key in ("T", "M", "A"):
                if row[key] != first[name][key]:
                    raise ValueError("FCS: %s gives channel %s the logicle %s %r, the files before it %r: a series takes one scale"
                                     % (path, name, key, row[key], first[name][key]))
        if not isinstance(points, ListMode):
            points = ListMode(np.ascontiguousarray(points, dtype=np.float64), points.shape[0], points.shape[1], np.float64)
        sources.append(points)
    d = len(first_picked)
    for qq in sorted(set(row["q"] for row in first.values() if row["W"] == ESTIMATE)):
        want = np.zeros(d, bool)
        for row in first.values():
            want[row["k"]] |= row["W"] == ESTIMATE and row["q"] == qq
        if handle is not None:
            count, lo, hi, frac = handle.negative_quantiles(sources, qq, want)
        else:
            count, lo, hi, frac = _lib.negative_quantiles_host(sources, qq, want)
        for name, row in first.items():
            k = row["k"]
            if want[k] and row["W"] == ESTIMATE:
                try:
                    row["W"] = logicle_w(count[k], lo[k], hi[k], frac[k], row["T"], row["M"])
                except ValueError as e:
                    raise ValueError("FCS: channel %s: %s" % (name, e)) from None
    out = {}
    for name, row in first.items():
        out[name] = {key: row[key] for key in LOGICLE_KEYS}
        try:
            _lib.logicle_coefficients([out[name][key] for key in LOGICLE_KEYS])
        except ValueError as e:
            raise ValueError("FCS: channel %s: %s" % (name, e)) from None
    return out


def estimate_sidecars(paths, handle=None):
    """({path: resolved logicle rows by channel name}, {channel name: row}) for the `.fcs` files among `paths` whose
    `<file>.transform` holds a logicle row with "W": "estimate": estimate_logicle over all of them, pooled (files whose
    sidecars ask for the same channels, compensation and rows are one pool).  The first result is what read_timepoint and
    Scaler take as `logicle`; both are empty where no sidecar asks for an estimate."""
    import json
    groups = {}
    for path in paths:
        if not str(path).lower().endswith(".fcs"):
            continue
        kw = sidecar_transform(path)
        spec = (kw or {}).get("logicle")
        if spec is None or not any(_is_unresolved(row) for row in ([spec] if _is_logicle_row(spec) else spec.values())):
            continue
        columns = sidecar_columns(path)
        if _is_logicle_row(spec):
            # one row for every selected channel that has no cofactor, spelled by name
            picked = read_fcs(path, columns=columns)[1]
            cof = _cofactors(kw.get("cofactor"), picked)
            spec = {name: spec for k, name in enumerate(picked) if cof is None or not cof[k] > 0}
        key = json.dumps([columns, kw["compensate"], spec], sort_keys=True)
        groups.setdefault(key, (columns, kw["compensate"], spec, []))[3].append(path)
    overrides, resolved = {}, {}
    for columns, compensate, spec, members in groups.values():
        rows = estimate_logicle(members, columns=columns, compensate=compensate, logicle=spec, handle=handle)
        for name, row in rows.items():
            if resolved.setdefault(name, row) != row:
                raise ValueError("FCS: the sidecars of this run give channel %s two logicle scales (%r, %r)" % (name, resolved[name], row))
        for path in members:
            overrides[path] = rows
    return overrides, resolved
