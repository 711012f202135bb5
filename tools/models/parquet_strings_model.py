"""The CPU model of libdeflate_amd_parquet_decode_batch_ex
(include/libdeflate_amd.h; libdeflate_amd/csrc/parquet_strings_plan.h): the
whole call over the rows that libdeflate_amd.parquet.pages(strings=True) or
tests/parquet_string_pages.py make - int64 offsets, the strings' bytes,
validity, the total and the verdicts - in numpy and plain Python on top of
parquet_model.py.  The tests compare the device against it byte for byte."""
import numpy as np

from . import parquet_model as pm

BYTE_ARRAY = 1 << 14
SUCCESS, BAD_DATA, INSUFFICIENT_SPACE = pm.SUCCESS, pm.BAD_DATA, pm.INSUFFICIENT_SPACE


def is_string(row):
    return bool(int(row[3]) & BYTE_ARRAY)


def unpack(row):
    """pm.unpack() of the row less the BYTE_ARRAY bit (a width of 1), and
    the bit"""
    r = [int(x) for x in row]
    f = pm.unpack(r[:3] + [r[3] & ~BYTE_ARRAY] + r[4:])
    f["byte_array"] = is_string(row)
    return f


def walk(sec, at, n):
    """the n length-prefixed values of sec from `at` -> a list of bytes, or
    None where a prefix or a value leaves the section"""
    vals = []
    for _ in range(n):
        if at + 4 > len(sec):
            return None
        ln = int.from_bytes(sec[at:at + 4], "little")
        if ln > len(sec) - at - 4:
            return None
        vals.append(bytes(sec[at + 4:at + 4 + ln]))
        at += 4 + ln
    return vals


def string_page(f, sec, lev, entries):
    """a BYTE_ARRAY data page whose section decoded to sec; entries: None
    (PLAIN) or the list of its dictionary's values -> (result, the slots'
    values as a list of bytes - the room the page takes -, levels); a failed
    page that takes no room: (BAD_DATA, None, None)"""
    n, val_at = f["count"], 0
    bad = (BAD_DATA, None, None)
    levels = np.ones(n, dtype=np.int64)
    if f["max_def"]:
        if f["kind"] == pm.DATA_V2:
            stream = lev
        else:
            if len(sec) < 4 or int.from_bytes(sec[:4], "little") > len(sec) - 4:
                return bad
            val_at = 4 + int.from_bytes(sec[:4], "little")
            stream = sec[4:val_at]
        levels = pm.hybrid(stream, 1, n, levels=True)
        if levels is None:
            return bad
    nv, res = int(levels.sum()), SUCCESS
    if entries is not None:
        vals = []
        if nv:
            if val_at >= len(sec) or sec[val_at] > 32:
                return bad
            idx = pm.hybrid(sec[val_at + 1:], sec[val_at], nv)
            if idx is None:
                return bad
            if (idx >= len(entries)).any():
                res = BAD_DATA      # (and the bad indices count as length 0)
            vals = [entries[i] if i < len(entries) else b"" for i in idx]
    else:
        # (the old call's check with width 1 asks less than the walk)
        vals = walk(sec, val_at, nv)
        if vals is None:
            return bad
    slots, k = [], 0
    for lv in levels:
        slots.append(vals[k] if lv else b"")
        k += int(lv)
    return res, slots, levels.astype(np.uint8)


def decode(rows, buf, fmt, out_nbytes, valid_nbytes, bytes_avail, fill=0):
    """The whole call -> a dict: results; out, valid, data (bytes_avail bytes)
    - arrays that start as `fill` -; total; out_defined, valid_defined,
    data_defined: False where a failed page leaves its own bytes undefined."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, pm.WORDS)
    out = np.full(out_nbytes, fill, dtype=np.uint8)
    valid = np.full(valid_nbytes, fill, dtype=np.uint8)
    data = np.full(bytes_avail, fill, dtype=np.uint8)
    out_def, valid_def = np.ones(out_nbytes, dtype=bool), np.ones(valid_nbytes, dtype=bool)
    data_def = np.ones(bytes_avail, dtype=bool)
    results, secs, pos = [], {}, 0
    for k, row in enumerate(rows):
        f = unpack(row)
        res, sec = pm.section(f, buf, fmt)
        vals = lev = None
        if f["kind"] == pm.DICT:
            entries = None
            if res == SUCCESS and f["count"] * f["width"] > len(sec):
                res = BAD_DATA
            if res == SUCCESS and f["byte_array"]:
                entries = walk(sec, 0, f["count"])
                if entries is None:
                    res = BAD_DATA
            secs[k] = (res, sec, f["count"], entries)
            results.append(res)
            continue
        d = secs[f["dict"]] if f["enc"] != pm.PLAIN else (SUCCESS, None, 0, None)
        levbytes = bytes(buf[f["off"]:f["off"] + f["def_len"]])
        if not f["byte_array"]:
            if res == SUCCESS:
                if d[0] != SUCCESS:
                    res = BAD_DATA
                else:
                    res, vals, lev = pm.data_page(f, sec, levbytes, d[2], d[1])
            results.append(res)
            a, n = f["out"], f["count"] * f["width"]
            if vals is None:
                out_def[a:a + n] = False
            else:
                out[a:a + n] = vals.reshape(-1)
        else:
            if res == SUCCESS:
                if d[0] != SUCCESS:
                    res = BAD_DATA
                else:
                    res, vals, lev = string_page(f, sec, levbytes,
                                                 d[3] if f["enc"] != pm.PLAIN else None)
            a, n = f["out"], (f["count"] + 1) * 8
            if vals is None:
                out_def[a:a + n] = False
            else:
                offs = pos + np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.int64)
                end = int(offs[-1])
                if res == SUCCESS and end > bytes_avail:
                    res = INSUFFICIENT_SPACE
                if res == BAD_DATA:
                    out_def[a:a + n] = False
                    data_def[min(pos, bytes_avail):min(end, bytes_avail)] = False
                    lev = None
                else:
                    out[a:a + n] = offs.astype("<i8").view(np.uint8)
                    if res == SUCCESS:
                        data[pos:end] = np.frombuffer(b"".join(vals), dtype=np.uint8)
                pos = end
            results.append(res)
        if f["max_def"]:
            if lev is None:
                valid_def[f["valid"]:f["valid"] + f["count"]] = False
            else:
                valid[f["valid"]:f["valid"] + f["count"]] = lev
    return dict(results=results, out=out, valid=valid, data=data, total=pos, out_defined=out_def,
                valid_defined=valid_def, data_defined=data_def)
