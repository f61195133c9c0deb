"""Writes FCS files and raw list-mode record buffers byte by byte, independently of chronoclust_amd.fcs: every element is laid
down with struct.pack / int.to_bytes from Python numbers, never through a numpy byte-order conversion, so the parser and
ListMode's host decode are checked against something that shares no code with them."""
import struct

import numpy as np

FLOAT_CODES = {4: "f", 8: "d"}


def element_bytes(value, kind, nbytes, order):
    """One element: kind 'f' (IEEE, 4 or 8 bytes) or 'u' (unsigned, nbytes bytes); order: the $BYTEORD list, 1 = the least
    significant byte - (1, 2, 3, 4) little-endian, (4, 3, 2, 1) big-endian, (3, 4, 1, 2) mixed."""
    if kind == "f":
        little = struct.pack("<" + FLOAT_CODES[nbytes], value)
    else:
        little = int(value).to_bytes(nbytes, "little")
    order = tuple(order)
    if order == tuple(sorted(order)):
        sig = list(range(nbytes))
    elif order == tuple(sorted(order, reverse=True)):
        sig = list(range(nbytes - 1, -1, -1))
    else:
        assert len(order) == nbytes
        sig = [o - 1 for o in order]
    return bytes(little[s] for s in sig)


def records(values, kind, nbytes, order):
    """The DATA bytes of `values` [n][par] (numbers; for kind 'f' numpy scalars of the element's own precision), event by event.
    nbytes: one width for all channels or one per channel."""
    out = bytearray()
    for row in values:
        for c, v in enumerate(row):
            nb = nbytes if isinstance(nbytes, int) else nbytes[c]
            out += element_bytes(v, kind, nb, order)
    return bytes(out)


def float_records(a, order):
    """records() of a float32 / float64 array, bit patterns kept (NaN payloads, signed zeros): through the integer image."""
    a = np.ascontiguousarray(a)
    nb = a.dtype.itemsize
    ints = a.view("u%d" % nb)
    return records(ints.tolist(), "u", nb, order)


def fast_records(a, order):
    """records() of a whole array [n, par] (float32 / float64 / uint8 / uint16 / uint32) at once: the element's bytes moved
    plane by plane into the order asked for - no byte-order conversion of numpy's.  Bit patterns are kept."""
    import sys
    assert sys.byteorder == "little"
    a = np.ascontiguousarray(a)
    nb = a.dtype.itemsize
    little = a.view(np.uint8).reshape(a.shape[0], a.shape[1], nb)
    order = tuple(order)
    if order == tuple(sorted(order)):
        sig = list(range(nb))
    elif order == tuple(sorted(order, reverse=True)):
        sig = list(range(nb - 1, -1, -1))
    else:
        assert len(order) == nb
        sig = [o - 1 for o in order]
    out = np.empty_like(little)
    for i, s in enumerate(sig):
        out[:, :, i] = little[:, :, s]
    return out.tobytes()


def fcs_bytes(data, par, datatype, order, bits, ranges=None, names=None, stains=None, version="FCS3.1", delimiter="/",
              tot=None, text_data_offsets=False, pad_before_data=0, trailing=b"", lower_keywords=False, extra=None,
              mode="L", omit=()):
    """A whole FCS file around the DATA bytes `data`.  bits: one $PnB for all or a list; ranges: $PnR likewise (default
    2^bits); tot: $TOT (None: keyword left out); text_data_offsets: HEADER's DATA offsets zero, $BEGINDATA / $ENDDATA say
    where; pad_before_data: bytes between TEXT and DATA (moves DATA to an odd offset); extra: further keywords."""
    bits = [bits] * par if isinstance(bits, int) else list(bits)
    ranges = [1 << b if b < 64 else (1 << 64) for b in bits] if ranges is None else ([ranges] * par if isinstance(ranges, int) else list(ranges))
    names = ["P%d" % (i + 1) for i in range(par)] if names is None else names
    kw = [("$MODE", mode), ("$DATATYPE", datatype), ("$PAR", str(par)), ("$BYTEORD", ",".join(str(o) for o in order)),
          ("$NEXTDATA", "0")]
    if tot is not None:
        kw.append(("$TOT", str(tot)))
    for i in range(par):
        kw += [("$P%dB" % (i + 1), str(bits[i])), ("$P%dR" % (i + 1), str(ranges[i])), ("$P%dN" % (i + 1), names[i]),
               ("$P%dE" % (i + 1), "0,0")]
        if stains is not None and stains[i]:
            kw.append(("$P%dS" % (i + 1), stains[i]))
    kw += list((extra or {}).items())
    kw = [(k, v) for k, v in kw if k not in omit]

    def text_of(begin, end):
        items = list(kw)
        if text_data_offsets:
            items = [("$BEGINDATA", "%d" % begin), ("$ENDDATA", "%d" % end)] + items
        out = delimiter
        for k, v in items:
            k = k.lower() if lower_keywords else k
            out += k.replace(delimiter, delimiter * 2) + delimiter + v.replace(delimiter, delimiter * 2) + delimiter
        return out.encode("latin-1")

    text_lo = 58
    # (the offsets are part of TEXT when text_data_offsets: fixed-width guesses first, then the real ones - same length)
    probe = text_of(10 ** 9, 10 ** 9 + 1)
    data_lo = text_lo + len(probe) + pad_before_data
    data_hi = data_lo + len(data) - 1
    text = text_of(data_lo, data_hi).ljust(len(probe), b" ") if text_data_offsets else text_of(0, 0)
    data_lo = text_lo + len(text) + pad_before_data
    data_hi = data_lo + len(data) - 1
    if text_data_offsets:
        text = text_of(data_lo, data_hi).ljust(len(probe), b" ")
    text_hi = text_lo + len(text) - 1
    hd = (0, 0) if text_data_offsets else (data_lo, max(data_hi, 0) if data else 0)
    header = version.encode() + b"    " + b"".join(("%8d" % v).encode() for v in (text_lo, text_hi, hd[0], hd[1], 0, 0))
    assert len(header) == 58
    return header + text + b"\0" * pad_before_data + data + trailing


def write_fcs(path, data, par, datatype, order, bits, **kw):
    blob = fcs_bytes(data, par, datatype, order, bits, **kw)
    with open(str(path), "wb") as f:
        f.write(blob)
    return str(path)


def unaligned(blob, shift=1):
    """A uint8 array holding `blob` that starts `shift` bytes past a 64-byte-aligned address."""
    buf = np.zeros(len(blob) + 64 + shift, np.uint8)
    start = (-buf.ctypes.data) % 64 + shift
    out = buf[start:start + len(blob)]
    out[:] = np.frombuffer(blob, np.uint8)
    assert out.ctypes.data % 64 == shift
    return out
