"""CPU model of the ZIP reader (libdeflate_amd_zip_index_batch /
_decompress_batch / _read_batch): the whole rule of include/libdeflate_amd.h
in plain Python - the end record's choice, ZIP64, the directory's candidates,
the chain, the index rows, the per-entry results and the verdict's precedence.
The kernels (csrc/zip_kernels.hip) are checked against it word for word, and
it is checked against Python's zipfile (tests/test_zip_abi.py)."""
import struct
import zlib
from collections import namedtuple

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
MORE_ENTRIES, MORE_CANDIDATES, UNSUPPORTED = 16, 17, 18
RESULT_WORDS, WORDS, SLACK, ZIP64 = 5, 8, 1024, 1
WINDOW = 65557              # an end record and the longest comment
END_BYTES, CEN_BYTES, LOCAL_BYTES = 22, 46, 30
SIG_END, SIG_LOC64, SIG_END64 = b"PK\5\6", b"PK\6\7", b"PK\6\6"
SIG_CEN, SIG_LOCAL = b"PK\1\2", b"PK\3\4"
FLAGS_REFUSED = 0x2061      # bits 0, 5, 6, 13
MARK32, MARK16 = 0xFFFFFFFF, 0xFFFF
EXTRA_RECORDS = 65535 // 4  # what the walk for the ZIP64 extra is bounded by

End = namedtuple("End", "p entries cd_off cd_size flags")
Result = namedtuple("Result", "words rows results plain")


def _u16(b, o):
    return struct.unpack_from("<H", b, o)[0]


def _u32(b, o):
    return struct.unpack_from("<I", b, o)[0]


def _u64(b, o):
    return struct.unpack_from("<Q", b, o)[0]


def end_offset(data):
    """the highest offset of the search window that carries the signature with
    a comment that stays inside the file, or None"""
    n = len(data)
    w0 = n - min(n, WINDOW)
    p = n - END_BYTES
    while p >= w0:
        p = data.rfind(SIG_END, w0, p + 4)
        if p < 0:
            return None
        if p + END_BYTES + _u16(data, p + 20) <= n:
            return p
        p -= 1
    return None


def find_end(data):
    """-> End, or None where the archive is BAD_DATA before its directory is
    looked at"""
    p = end_offset(data)
    if p is None:
        return None
    ok = _u16(data, p + 4) == 0 and _u16(data, p + 6) == 0 and \
        _u16(data, p + 8) == _u16(data, p + 10)
    entries, cd_size, cd_off = _u16(data, p + 10), _u32(data, p + 12), _u32(data, p + 16)
    anchor, flags = p, 0
    if p >= 20 and data[p - 20:p - 16] == SIG_LOC64:
        q = _u64(data, p - 12)
        if not (_u32(data, p - 4) <= 1 and q + 56 <= p - 20 and data[q:q + 4] == SIG_END64):
            return None
        ok = _u32(data, q + 16) == 0 and _u32(data, q + 20) == 0 and \
            _u64(data, q + 24) == _u64(data, q + 32)
        entries, cd_size, cd_off = _u64(data, q + 32), _u64(data, q + 40), _u64(data, q + 48)
        anchor, flags = q, ZIP64
    if not ok or cd_size > MARK32 or cd_size > anchor or cd_off != anchor - cd_size:
        return None
    return End(p, entries, cd_off, cd_size, flags)


def candidates(data, end):
    """every offset of the directory with the signature and 46 bytes of
    directory behind it, relative to cd_off, ascending"""
    lo, hi = end.cd_off, end.cd_off + end.cd_size
    out, p = [], data.find(SIG_CEN, lo, hi)
    while p >= 0 and p + CEN_BYTES <= hi:
        out.append(p - lo)
        p = data.find(SIG_CEN, p + 1, hi)
    return out


def record_size(data, end, rel):
    c = end.cd_off + rel
    return CEN_BYTES + _u16(data, c + 28) + _u16(data, c + 30) + _u16(data, c + 32)


def chain(data, end, cands):
    """the candidates reached from cd_off when the chain ends exactly at
    cd_off + cd_size, else None"""
    if end.cd_size == 0:
        return []
    have, at, out = set(cands), 0, []
    while at != end.cd_size:
        if at not in have:
            return None
        out.append(at)
        at += record_size(data, end, at)
        if at > end.cd_size:
            return None
    return out


def resolve(data, end, rel):
    """-> (row words 0..6, pre-decode result) of the entry whose central
    record stands at cd_off + rel"""
    c = end.cd_off + rel
    flags, method, crc = _u16(data, c + 8), _u16(data, c + 10), _u32(data, c + 16)
    csize, usize, lho = _u32(data, c + 20), _u32(data, c + 24), _u32(data, c + 42)
    name_len, extra_len, disk = _u16(data, c + 28), _u16(data, c + 30), _u16(data, c + 34)
    r = SUCCESS
    if MARK32 in (csize, usize, lho) or disk == MARK16:
        x = data[c + CEN_BYTES + name_len:c + CEN_BYTES + name_len + extra_len]
        z, at = b"", 0
        for _ in range(EXTRA_RECORDS):
            if at + 4 > extra_len:
                break
            rid, sz = _u16(x, at), _u16(x, at + 2)
            if at + 4 + sz > extra_len:
                break
            if rid == 1:
                z = x[at + 4:at + 4 + sz]
                break
            at += 4 + sz
        o = 0
        if usize == MARK32:
            usize, r = (_u64(z, o), r) if o + 8 <= len(z) else (usize, BAD_DATA)
            o += 8
        if csize == MARK32:
            csize, r = (_u64(z, o), r) if o + 8 <= len(z) else (csize, BAD_DATA)
            o += 8
        if lho == MARK32:
            lho, r = (_u64(z, o), r) if o + 8 <= len(z) else (lho, BAD_DATA)
            o += 8
        if disk == MARK16:
            disk, r = (_u32(z, o), r) if o + 4 <= len(z) else (disk, BAD_DATA)
    if r == SUCCESS and disk != 0:
        r = BAD_DATA
    if r == SUCCESS and ((flags & FLAGS_REFUSED) or method not in (0, 8)
                         or csize > MARK32 or usize > MARK32):
        r = UNSUPPORTED
    data_off = 0
    if r == SUCCESS:
        r = BAD_DATA
        if lho + LOCAL_BYTES <= end.cd_off and data[lho:lho + 4] == SIG_LOCAL:
            d = lho + LOCAL_BYTES + _u16(data, lho + 26) + _u16(data, lho + 28)
            if d <= end.cd_off:
                data_off = d
                if d + csize <= end.cd_off:
                    r = SUCCESS
    if r == SUCCESS and method == 0 and csize != usize:
        r = BAD_DATA
    return [c, name_len, method | flags << 16, crc, data_off, csize, usize], r


def decode_entry(data, row):
    """-> (result, bytes or None): method 8 must use exactly csize bytes and
    give exactly usize bytes; the CRC-32 is the row's"""
    method, crc, data_off, csize, usize = row[2] & 0xFFFF, row[3], row[4], row[5], row[6]
    raw = data[data_off:data_off + csize]
    if method == 0:
        got = raw
    else:
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(raw) + d.flush()
        except zlib.error:
            return BAD_DATA, None
        if not d.eof:
            return BAD_DATA, None
        if len(got) > usize:
            return INSUFFICIENT_SPACE, None
        if len(got) < usize:
            return SHORT_OUTPUT, None
        if d.unused_data:
            return BAD_DATA, None
    if zlib.crc32(got) != crc:
        return BAD_DATA, None
    return SUCCESS, got


def read(data, max_entries, out_avail=None, out_align=1, decode=True):
    """The archive `data` as libdeflate_amd_zip_decompress_batch reads it
    (decode=False: _index_batch) -> Result: the five words; rows (8 words per
    entry) and per-entry results, None where the call writes neither; plain:
    every entry's bytes (None for one that did not succeed), None where
    nothing was decoded."""
    data = bytes(data)
    if out_avail is None or not decode:
        out_avail = 1 << 64
    end = find_end(data)
    if end is None:
        return Result([BAD_DATA, 0, 0, 0, 0], None, None, None)
    if end.entries > max_entries:
        return Result([MORE_ENTRIES, end.entries, 0, 0, 0], None, None, None)
    cands = candidates(data, end)
    if len(cands) > min(max_entries + SLACK, len(data) // 4 + 1):
        return Result([MORE_CANDIDATES, len(cands), 0, 0, 0], None, None, None)
    rels = chain(data, end, cands)
    if rels is None or len(rels) != end.entries:
        return Result([BAD_DATA, 0, 0, 0, 0], None, None, None)
    rows, results, at = [], [], 0
    for rel in rels:
        row, r = resolve(data, end, rel)
        rows.append(row + [at])
        results.append(r)
        if r == SUCCESS:
            at += -(-row[6] // out_align) * out_align
    words = [SUCCESS, end.entries, end.cd_off, at, end.flags]
    if at > out_avail:
        words[0] = INSUFFICIENT_SPACE
        return Result(words, rows, results, None)
    plain = None
    if decode:
        plain = []
        for k, row in enumerate(rows):
            got = None
            if results[k] == SUCCESS:
                results[k], got = decode_entry(data, row)
            plain.append(got)
    words[0] = next((r for r in results if r != SUCCESS), SUCCESS)
    return Result(words, rows, results, plain)


def read_selection(data, rows, sel, out_align=1):
    """libdeflate_amd_zip_read_batch -> (offsets (len(sel) + 1), results,
    bytes per selection)"""
    data = bytes(data)
    offs, results, plain, at = [], [], [], 0
    for k in sel:
        row = [int(x) for x in rows[k]]
        method, flags = row[2] & 0xFFFF, row[2] >> 16
        offs.append(at)
        if (flags & FLAGS_REFUSED) or method not in (0, 8):
            r, got = UNSUPPORTED, None
        elif method == 0 and row[5] != row[6]:
            r, got = BAD_DATA, None
        else:
            at += -(-row[6] // out_align) * out_align
            r, got = decode_entry(data, row)
        results.append(r)
        plain.append(got)
    return offs + [at], results, plain
