"""CPU model of the tar reader (libdeflate_amd_tar_index_batch /
_extract_batch / _read_batch / _ranges): the whole rule of
include/libdeflate_amd.h in plain Python - the header rule, the serial walk,
the candidates the device scan lists, the names, the index rows, the per-entry
results and the verdict's precedence.  The kernels (csrc/tar_kernels.hip) are
checked against it word for word, and it is checked against Python's tarfile
(tests/test_tar_abi.py)."""
from collections import namedtuple

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
MORE_RECORDS, MORE_CANDIDATES, UNSUPPORTED = 16, 17, 18
RESULT_WORDS, WORDS, SLACK = 5, 8, 1024
EOF, HAS_L, HAS_PAX = 1, 2, 4
BLOCK = 512
SIZE_LIMIT = 1 << 36        # a size field of this or more is no header
EXT_MAX = 8                 # extension records in front of one entry
EXT_BYTES = 1 << 20         # the largest L or x record that is read
COPY_TILE = 65536           # bytes per tile of the gather copy
NAME_HEADER, NAME_L, NAME_PAX = 0, 1, 2
EXT_TYPES = b"LKxXg"
NO_DATA_TYPES = b"123456"   # links, devices, directories, FIFOs
REFUSED_TYPES = b"SMD"

Result = namedtuple("Result", "words rows results plain")
Walk = namedtuple("Walk", "ok records end eof")


def octal(field):
    """-> (value, digits) or None: leading spaces, octal digits, then the
    field's end, a NUL or a space"""
    i, n = 0, len(field)
    while i < n and field[i] == 0x20:
        i += 1
    v = d = 0
    while i < n and 0x30 <= field[i] <= 0x37:
        v = v * 8 + field[i] - 0x30
        i += 1
        d += 1
    if i < n and field[i] not in (0, 0x20):
        return None
    return v, d


def header_size(h):
    """the size field of the 512-byte block h, or None"""
    f = h[124:136]
    if f[0] == 0x80:
        return int.from_bytes(f[1:], "big")
    if f[0] & 0x80:
        return None
    r = octal(f)
    return None if r is None else r[0]


def header_blocks(h):
    """data blocks of the record whose header is the block h (rule 4 without
    the bound), or None where h is no header"""
    c = octal(h[148:156])
    if c is None or c[1] == 0:
        return None
    unsigned = sum(h[:148]) + 8 * 0x20 + sum(h[156:])
    signed = unsigned - 256 * sum(1 for b in h[:148] + h[156:] if b >= 0x80)
    if c[0] != unsigned and c[0] != signed:
        return None
    size = header_size(h)
    if size is None or size >= SIZE_LIMIT:
        return None
    if h[156] in NO_DATA_TYPES:
        return 0
    return (size + BLOCK - 1) // BLOCK


def record_at(data, nb, pos):
    """1 + d of the record at block pos, or 0"""
    d = header_blocks(data[BLOCK * pos:BLOCK * pos + BLOCK])
    return 0 if d is None or pos + 1 + d > nb else 1 + d


def walk(data):
    """the serial walk that defines the rule: records as block positions"""
    nb = len(data) // BLOCK
    zero = bytes(BLOCK)
    pos, recs = 0, []
    while pos < nb:
        if data[BLOCK * pos:BLOCK * pos + BLOCK] == zero:
            return Walk(True, recs, pos, True)
        size = record_at(data, nb, pos)
        if not size:
            return Walk(False, recs, pos, False)
        recs.append(pos)
        pos += size
    return Walk(nb > 0, recs, pos, False)


def candidates(data):
    """what the device scan lists: every block that passes rule 4"""
    nb = len(data) // BLOCK
    return [p for p in range(nb) if record_at(data, nb, p)]


def _strnlen(b):
    k = b.find(b"\0")
    return len(b) if k < 0 else k


def pax_parse(buf):
    """-> (ok, path (offset, length) or None, a size= key was seen)"""
    p, path, size_key = 0, None, False
    while p < len(buf):
        q, n = p, 0
        while q < len(buf) and q - p < 8 and 0x30 <= buf[q] <= 0x39:
            n = n * 10 + buf[q] - 0x30
            q += 1
        if q == p or q >= len(buf) or buf[q] != 0x20 or p + n > len(buf) or q + 1 >= p + n:
            return False, None, False
        if buf[p + n - 1] != 0x0A:
            return False, None, False
        eq = buf.find(b"=", q + 1, p + n - 1)
        if eq < 0:
            return False, None, False
        key = buf[q + 1:eq]
        if key == b"path":
            path = (eq + 1, p + n - 1 - (eq + 1))
        elif key == b"size":
            size_key = True
        p += n
    return True, path, size_key


def entries_of(data, recs):
    """-> (rows without out_off, results, flags): one row per entry record"""
    rows, results, flags = [], [], 0
    for k, pos in enumerate(recs):
        h = data[BLOCK * pos:BLOCK * pos + BLOCK]
        t = h[156]
        if t == 0x4C:
            flags |= HAS_L
        if t in b"xXg":
            flags |= HAS_PAX
        if t in EXT_TYPES:
            continue
        res = SUCCESS
        l_name = pax_name = None
        j = k
        while j > 0:
            q = recs[j - 1]
            e = data[BLOCK * q:BLOCK * q + BLOCK]
            if e[156] not in EXT_TYPES:
                break
            if k - j == EXT_MAX:
                res = UNSUPPORTED
                break
            j -= 1
            esize = header_size(e)
            d0 = BLOCK * (q + 1)
            if e[156] == 0x4C:
                if esize > EXT_BYTES:
                    res = UNSUPPORTED
                elif l_name is None:
                    l_name = (d0, _strnlen(data[d0:d0 + esize]))
            elif e[156] in b"xX":
                if esize > EXT_BYTES:
                    res = UNSUPPORTED
                else:
                    ok, path, size_key = pax_parse(data[d0:d0 + esize])
                    if not ok or size_key:
                        res = UNSUPPORTED
                    elif path is not None and pax_name is None:
                        pax_name = (d0 + path[0], path[1])
        if t in REFUSED_TYPES:
            res = UNSUPPORTED
        size = header_size(h)
        usize = 0 if t in NO_DATA_TYPES or res != SUCCESS else size
        src, name, prefix = NAME_HEADER, (BLOCK * pos, _strnlen(h[:100])), 0
        if res == SUCCESS and pax_name is not None:
            src, name = NAME_PAX, pax_name
        elif res == SUCCESS and l_name is not None:
            src, name = NAME_L, l_name
        elif h[257:263] == b"ustar\0":
            prefix = _strnlen(h[345:500])
        m = octal(h[136:148])
        rows.append([BLOCK * pos, name[0], name[1] | prefix << 32, t | src << 8,
                     BLOCK * (pos + 1), usize, m[0] if m else 0])
        results.append(res)
    return rows, results, flags


def read(data, max_records, out_avail=None, out_align=1, extract=True):
    """the device calls: -> Result(words, rows, results, plain); rows and
    results are None where the device writes none, plain is None unless the
    extract ran (per entry its bytes, None for an entry that failed)"""
    nb = len(data) // BLOCK
    bad = Result([BAD_DATA, 0, 0, 0, 0], None, None, None)
    if nb == 0:
        return bad
    k = len(candidates(data))
    if k > min(max_records + SLACK, nb):
        return Result([MORE_CANDIDATES, k, 0, 0, 0], None, None, None)
    w = walk(data)
    if not w.ok:
        return bad
    if len(w.records) > max_records:
        return Result([MORE_RECORDS, len(w.records), 0, 0, 0], None, None, None)
    rows, results, flags = entries_of(data, w.records)
    at = 0
    for row in rows:
        row.append(at)
        at += (row[5] + out_align - 1) // out_align * out_align
    words = [SUCCESS, len(rows), BLOCK * w.end, at, flags | (EOF if w.eof else 0)]
    if extract and out_avail is not None and at > out_avail:
        words[0] = INSUFFICIENT_SPACE
        return Result(words, rows, results, None)
    for r in results:
        if r != SUCCESS:
            words[0] = r
            break
    plain = None
    if extract:
        plain = [data[row[4]:row[4] + row[5]] if r == SUCCESS else None
                 for row, r in zip(rows, results)]
    return Result(words, rows, results, plain)


def name_of(data, row):
    """the entry's name as bytes: prefix, '/' and name"""
    n, p = row[2] & 0xFFFFFFFF, row[2] >> 32
    name = bytes(data[row[1]:row[1] + n])
    return bytes(data[row[0] + 345:row[0] + 345 + p]) + b"/" + name if p else name


def row_result(row):
    return UNSUPPORTED if (row[3] & 0xFF) in REFUSED_TYPES else SUCCESS


def read_selection(data, rows, sel, out_align=1):
    """libdeflate_amd_tar_read_batch: -> (out_offsets (len(sel) + 1), results,
    bytes per selection)"""
    offs, res, plain, at = [], [], [], 0
    for k in sel:
        row = rows[k]
        offs.append(at)
        r = row_result(row)
        res.append(r)
        if r == SUCCESS:
            plain.append(data[row[4]:row[4] + row[5]])
            at += (row[5] + out_align - 1) // out_align * out_align
        else:
            plain.append(None)
    return offs + [at], res, plain


def ranges(rows, sel):
    """libdeflate_amd_tar_ranges: -> ((data_off, usize) per selection, total)"""
    out = [(rows[k][4], rows[k][5] if row_result(rows[k]) == SUCCESS else 0) for k in sel]
    return out, sum(n for _, n in out)
