"""The CPU model of libdeflate_amd_parquet_decode_batch (include/libdeflate_amd.h;
libdeflate_amd/csrc/parquet_plan.h): the RLE / bit-packed hybrid decoder, the
decode of a page and the verdicts, in numpy and plain Python, over the rows that
libdeflate_amd.parquet.pages() or tests/parquet_pages.py make.  The tests
compare the device against it byte for byte."""
import zlib

import numpy as np

WORDS = 8
DATA_V1, DICT, DATA_V2 = 0, 2, 3
PLAIN, PLAIN_DICTIONARY, RLE_DICTIONARY = 0, 2, 8
SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
# parquet_plan.h: the slots of an expand tile, the values of a piece of a
# bit-packed level run
TILE, LEVEL_PIECE = 1024, 512
WBITS = {"gzip": 31, "zlib": 15, "deflate": -15}


def unpack(row):
    """a row's words -> a dict of its fields"""
    r = [int(x) for x in row]
    return dict(off=r[0], csize=r[1], usize=r[2], kind=r[3] & 15, enc=r[3] >> 4 & 255,
                compressed=r[3] >> 12 & 1, max_def=r[3] >> 13 & 1, width=(r[3] >> 16 & 255) + 1,
                count=r[4] & 0xFFFFFFFF, def_len=r[4] >> 32, out=r[5], valid=r[6], dict=r[7])


def hybrid(stream, w, n, levels=False):
    """the n values a hybrid stream of bit width w owes -> int64 array, or None
    where the header's rules say BAD_DATA"""
    stream = bytes(stream)
    vals, done, p, vb = np.zeros(n, dtype=np.int64), 0, 0, (w + 7) // 8
    while done < n:
        h = k = 0
        while True:
            if k == 5 or p >= len(stream):
                return None
            b = stream[p]
            p += 1
            h |= (b & 0x7F) << (7 * k)
            k += 1
            if not b & 0x80:
                break
        cnt = h >> 1
        if cnt == 0:
            return None
        if h & 1:
            take = min(cnt * 8, n - done)
            need = (take * w + 7) // 8
            if need > len(stream) - p:
                return None
            if w:
                bits = np.unpackbits(np.frombuffer(stream[p:p + need], dtype=np.uint8),
                                     bitorder="little")[:take * w].reshape(take, w)
                vals[done:done + take] = (bits.astype(np.int64) << np.arange(w)).sum(axis=1)
            p += min(cnt * w, len(stream) - p)
        else:
            if vb > len(stream) - p:
                return None
            val = int.from_bytes(stream[p:p + vb], "little")
            p += vb
            if levels and val > 1:
                return None
            take = min(cnt, n - done)
            vals[done:done + take] = val
        done += take
    return vals


def inflate(fmt, data, want):
    """(what libdeflate_<fmt>_decompress_ex reports for data with
    out_nbytes_avail = want and a NULL actual_out, the bytes)"""
    d = zlib.decompressobj(WBITS[fmt])
    try:
        out = d.decompress(bytes(data), want + 1)
        if len(out) > want:
            return INSUFFICIENT_SPACE, b""
        out += d.flush()
    except zlib.error:
        return BAD_DATA, b""
    if not d.eof:
        return BAD_DATA, b""
    if len(out) > want:
        return INSUFFICIENT_SPACE, b""
    return (SHORT_OUTPUT if len(out) < want else SUCCESS), out


def section(f, buf, fmt):
    """(the result of the section of page f, its bytes)"""
    a, n = f["off"] + f["def_len"], f["csize"] - f["def_len"]
    if not f["compressed"]:
        return SUCCESS, bytes(buf[a:a + n])
    return inflate(fmt, buf[a:a + n], f["usize"] - f["def_len"])


def data_page(f, sec, lev, entries, dictionary):
    """a data page whose section decoded to sec (lev: a V2 page's level bytes);
    dictionary: None, or its section's bytes, of `entries` entries ->
    (BAD_DATA, None, None) or (SUCCESS, uint8 [count, width], uint8 [count])"""
    n, width, val_at = f["count"], f["width"], 0
    bad = (BAD_DATA, None, None)
    levels = np.ones(n, dtype=np.int64)
    if f["max_def"]:
        if f["kind"] == DATA_V2:
            stream = lev
        else:
            if len(sec) < 4 or int.from_bytes(sec[:4], "little") > len(sec) - 4:
                return bad
            val_at = 4 + int.from_bytes(sec[:4], "little")
            stream = sec[4:val_at]
        levels = hybrid(stream, 1, n, levels=True)
        if levels is None:
            return bad
    nv = int(levels.sum())
    values = np.zeros((nv, width), dtype=np.uint8)
    if f["enc"] != PLAIN:
        if nv:
            if val_at >= len(sec) or sec[val_at] > 32:
                return bad
            idx = hybrid(sec[val_at + 1:], sec[val_at], nv)
            if idx is None or (idx >= entries).any():
                return bad
            values = np.frombuffer(dictionary[:entries * width], dtype=np.uint8).reshape(
                entries, width)[idx]
    else:
        if nv * width > len(sec) - val_at:
            return bad
        values = np.frombuffer(sec[val_at:val_at + nv * width], dtype=np.uint8).reshape(nv, width)
    out = np.zeros((n, width), dtype=np.uint8)
    out[levels == 1] = values
    return SUCCESS, out, levels.astype(np.uint8)


def decode(rows, buf, fmt, out_nbytes, valid_nbytes, fill=0):
    """The whole call -> (results, out, valid, out_defined, valid_defined): the
    two arrays start as `fill`; a page that ends in SUCCESS writes its slots
    and validity bytes; a failed data page leaves its own undefined (False in
    the two masks)."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, WORDS)
    out = np.full(out_nbytes, fill, dtype=np.uint8)
    valid = np.full(valid_nbytes, fill, dtype=np.uint8)
    out_def, valid_def = np.ones(out_nbytes, dtype=bool), np.ones(valid_nbytes, dtype=bool)
    results, secs = [], {}
    for k, row in enumerate(rows):
        f = unpack(row)
        res, sec = section(f, buf, fmt)
        vals = lev = None
        if f["kind"] == DICT:
            if res == SUCCESS and f["count"] * f["width"] > len(sec):
                res = BAD_DATA
            secs[k] = (res, sec, f["count"])
        elif res == SUCCESS:
            d = secs[f["dict"]] if f["enc"] != PLAIN else (SUCCESS, None, 0)
            if d[0] != SUCCESS:
                res = BAD_DATA
            else:
                res, vals, lev = data_page(f, sec, bytes(buf[f["off"]:f["off"] + f["def_len"]]),
                                           d[2], d[1])
        results.append(res)
        if f["kind"] == DICT:
            continue
        a, n = f["out"], f["count"] * f["width"]
        if vals is None:
            out_def[a:a + n] = False
            if f["max_def"]:
                valid_def[f["valid"]:f["valid"] + f["count"]] = False
        else:
            out[a:a + n] = vals.reshape(-1)
            if f["max_def"]:
                valid[f["valid"]:f["valid"] + f["count"]] = lev
    return results, out, valid, out_def, valid_def
