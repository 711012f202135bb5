"""The host side of the Parquet calls (libdeflate_amd_parquet_decode_batch and
its _ex form, which reads BYTE_ARRAY columns too):
parse() reads the footer of a host copy of a Parquet file, pages() walks the
page headers of the selected column chunks and makes the page rows the decode
call takes plus a layout of the columns, and read_columns() runs the call and
hands back tensors.

    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    cols = parquet.read_columns(dec, buf, d_in, ["price", "qty"])
    values, mask = cols["price"]        # float64 [rows], torch.bool [rows] or None

Flat columns of INT32, INT64, INT96, FLOAT, DOUBLE and FIXED_LEN_BYTE_ARRAY,
PLAIN or dictionary-coded, in V1 or V2 pages, GZIP or uncompressed; anything
else raises with the column's name and the reason.  BYTE_ARRAY columns -
`string` and `binary` - come back as ((offsets int64 [rows + 1], bytes uint8),
mask), Arrow's large layout.  Everything here is host
arithmetic on the footer and the page headers; no column byte is touched.  Pure
Python: a small Thrift compact-protocol reader, no Parquet library."""
import struct

import numpy as np

from . import binding

MAGIC = b"PAR1"
BOOLEAN, INT32, INT64, INT96, FLOAT, DOUBLE, BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY = range(8)
TYPE_NAMES = ["BOOLEAN", "INT32", "INT64", "INT96", "FLOAT", "DOUBLE", "BYTE_ARRAY",
              "FIXED_LEN_BYTE_ARRAY"]
TYPE_WIDTH = {INT32: 4, INT64: 8, INT96: 12, FLOAT: 4, DOUBLE: 8}
TYPE_DTYPE = {INT32: "int32", INT64: "int64", FLOAT: "float32", DOUBLE: "float64"}
UNCOMPRESSED, SNAPPY, GZIP = 0, 1, 2
CODEC_NAMES = ["UNCOMPRESSED", "SNAPPY", "GZIP", "LZO", "BROTLI", "LZ4", "ZSTD", "LZ4_RAW"]
REQUIRED, OPTIONAL, REPEATED = 0, 1, 2
DATA_PAGE, INDEX_PAGE, DICTIONARY_PAGE, DATA_PAGE_V2 = 0, 1, 2, 3
PLAIN, PLAIN_DICTIONARY, RLE, BIT_PACKED, RLE_DICTIONARY = 0, 2, 3, 4, 8
ALIGN = 64


# ---- Thrift's compact protocol: structs as {field id: value}, unknown fields kept ----

T_STOP, T_TRUE, T_FALSE, T_BYTE, T_I16, T_I32, T_I64, T_DOUBLE, T_BINARY, T_LIST, T_SET, T_MAP, \
    T_STRUCT = range(13)


class Thrift:
    def __init__(self, buf, at=0):
        self.buf, self.at = buf, at

    def byte(self):
        if self.at >= len(self.buf):
            raise ValueError("parquet: a Thrift structure leaves the buffer")
        self.at += 1
        return self.buf[self.at - 1]

    def varint(self):
        v = shift = 0
        while True:
            b = self.byte()
            v |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                return v
            if shift > 70:
                raise ValueError("parquet: a Thrift varint of more than 10 bytes")

    def zigzag(self):
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def value(self, t, depth):
        if depth > 32:
            raise ValueError("parquet: Thrift structures nested too deep")
        if t in (T_TRUE, T_FALSE):
            return t == T_TRUE
        if t == T_BYTE:
            return self.byte()
        if t in (T_I16, T_I32, T_I64):
            return self.zigzag()
        if t == T_DOUBLE:
            self.at += 8
            return struct.unpack("<d", bytes(self.buf[self.at - 8:self.at]))[0]
        if t == T_BINARY:
            n = self.varint()
            if n > len(self.buf) - self.at:
                raise ValueError("parquet: a Thrift string leaves the buffer")
            self.at += n
            return bytes(self.buf[self.at - n:self.at])
        if t in (T_LIST, T_SET):
            head = self.byte()
            n, et = head >> 4, head & 15
            if n == 15:
                n = self.varint()
            if et in (T_TRUE, T_FALSE):     # a bool element is a byte of its own
                return [self.byte() == T_TRUE for _ in range(n)]
            return [self.value(et, depth + 1) for _ in range(n)]
        if t == T_MAP:
            n = self.varint()
            if not n:
                return {}
            kv = self.byte()
            return dict((self.value(kv >> 4, depth + 1), self.value(kv & 15, depth + 1))
                        for _ in range(n))
        if t == T_STRUCT:
            return self.struct(depth + 1)
        raise ValueError("parquet: Thrift type %d" % t)

    def struct(self, depth=0):
        out, fid = {}, 0
        while True:
            head = self.byte()
            if head == T_STOP:
                return out
            fid = fid + (head >> 4) if head >> 4 else self.zigzag()
            out[fid] = self.value(head & 15, depth)


# ---- the footer ----

class Leaf:
    """a leaf of the schema: name (dotted path), type (physical), width (bytes
    of a value, None for BOOLEAN and BYTE_ARRAY), max_def, max_rep"""

    def __init__(self, name, ptype, width, max_def, max_rep):
        self.name, self.type, self.width = name, ptype, width
        self.max_def, self.max_rep = max_def, max_rep

    def __repr__(self):
        return "Leaf(%r, %s, width=%r, max_def=%d, max_rep=%d)" % (
            self.name, TYPE_NAMES[self.type], self.width, self.max_def, self.max_rep)


class Chunk:
    """a column chunk: its leaf's index, codec, num_values, where its pages
    start (the dictionary page if there is one) and their total compressed
    size"""

    def __init__(self, leaf, codec, num_values, start, nbytes):
        self.leaf, self.codec, self.num_values = leaf, codec, num_values
        self.start, self.nbytes = start, nbytes


class File:
    """a parsed footer: num_rows, leaves: [Leaf], row_groups: [(num_rows,
    [Chunk per leaf])]"""

    def __init__(self, num_rows, leaves, row_groups):
        self.num_rows, self.leaves, self.row_groups = num_rows, leaves, row_groups

    def leaf_index(self, name):
        for k, leaf in enumerate(self.leaves):
            if leaf.name == name:
                return k
        raise KeyError("parquet: no column %r" % (name,))


def parse(buf):
    """the footer of a Parquet file (bytes-like, the whole file) -> File"""
    buf = memoryview(buf).cast("B")
    if len(buf) < 12 or bytes(buf[:4]) != MAGIC or bytes(buf[-4:]) != MAGIC:
        raise ValueError("parquet: no PAR1 at both ends (an encrypted footer is PARE)")
    n = struct.unpack("<I", bytes(buf[-8:-4]))[0]
    if n > len(buf) - 12:
        raise ValueError("parquet: the footer length leaves the file")
    meta = Thrift(buf[len(buf) - 8 - n:len(buf) - 8]).struct()
    schema = meta.get(2, [])
    leaves, at = [], [1]

    def walk(prefix, max_def, max_rep, children):
        for _ in range(children):
            if at[0] >= len(schema):
                raise ValueError("parquet: the schema's children leave its list")
            el = schema[at[0]]
            at[0] += 1
            name = prefix + el.get(4, b"").decode("utf-8", "replace")
            rep = el.get(3, REQUIRED)
            d, r = max_def + (rep != REQUIRED), max_rep + (rep == REPEATED)
            if el.get(5):
                walk(name + ".", d, r, el[5])
            else:
                t = el.get(1)
                width = el.get(2) if t == FIXED_LEN_BYTE_ARRAY else TYPE_WIDTH.get(t)
                leaves.append(Leaf(name, t, width, d, r))
    if schema:
        walk("", 0, 0, schema[0].get(5, 0))
    groups = []
    for rg in meta.get(4, []):
        chunks = []
        for k, cc in enumerate(rg.get(1, [])):
            md = cc.get(3)
            if md is None or k >= len(leaves):
                raise ValueError("parquet: a column chunk without metadata")
            start = md.get(11) or md.get(9, 0)
            if md.get(11) and md.get(9, 0) < md[11]:    # some writers state a stale dictionary offset
                start = md[9]
            chunks.append(Chunk(k, md.get(4, 0), md.get(5, 0), start, md.get(7, 0)))
        groups.append((rg.get(3, 0), chunks))
    return File(meta.get(3, 0), leaves, groups)


# ---- the pages ----

class Column:
    """where a selected column lies: offset in d_out, valid_offset in d_valid
    (None for max_def 0), rows, width, type, dtype (numpy's name, or None for
    INT96 and FIXED_LEN_BYTE_ARRAY: uint8 [rows, width]).  byte_array: at
    offset lie rows + 1 int64 offsets into the call's d_bytes instead, and width
    is None"""

    def __init__(self, name, offset, valid_offset, rows, leaf):
        self.name, self.offset, self.valid_offset, self.rows = name, offset, valid_offset, rows
        self.width, self.type, self.dtype = leaf.width, leaf.type, TYPE_DTYPE.get(leaf.type)
        self.byte_array = leaf.type == BYTE_ARRAY


class Pages:
    """rows: numpy uint64 (pages, PARQUET_WORDS); format: "gzip", "zlib" or
    "deflate"; columns: {name: Column}; out_nbytes, valid_nbytes: what d_out
    and d_valid must hold; bytes_estimate: an estimate from the page headers of
    what d_bytes must hold, 0 without a BYTE_ARRAY column"""

    def __init__(self, rows, fmt, columns, out_nbytes, valid_nbytes, bytes_estimate=0):
        self.rows, self.format, self.columns = rows, fmt, columns
        self.out_nbytes, self.valid_nbytes = out_nbytes, valid_nbytes
        self.bytes_estimate = bytes_estimate


def _align(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


def _format_of(head):
    if len(head) >= 2 and head[0] == 0x1F and head[1] == 0x8B:
        return "gzip"
    if len(head) >= 2 and head[0] & 15 == 8 and (head[0] << 8 | head[1]) % 31 == 0:
        return "zlib"
    return "deflate"


def pages(buf, columns=None, row_groups=None, file=None, strings=False):
    """The page rows of the selected column chunks.  columns: names (None: every
    leaf); row_groups: indices in the order their rows shall lie in every
    column (None: all, in the file's order); file: parse(buf), if at hand.
    Every selected column is one contiguous array of (its rows) x width at a
    64-byte aligned offset of d_out, its validity bytes likewise in d_valid.
    strings: take BYTE_ARRAY columns too, as rows of
    libdeflate_amd_parquet_decode_batch_ex: such a column is (its rows + 1) x 8
    bytes of int64 offsets.  -> Pages.  Raises ValueError for what is out of scope, with the column's
    name and the reason."""
    buf = memoryview(buf).cast("B")
    f = file or parse(buf)
    names = [leaf.name for leaf in f.leaves] if columns is None else list(columns)
    groups = list(range(len(f.row_groups))) if row_groups is None else list(row_groups)
    total = sum(f.row_groups[g][0] for g in groups)
    rows, layout, fmt = [], {}, None
    out_at = valid_at = estimate = 0

    for name in names:
        leaf = f.leaves[f.leaf_index(name)]

        def no(why):
            return ValueError("parquet: column %r: %s" % (name, why))
        if leaf.max_rep or leaf.max_def > 1:
            raise no("nested or repeated (max_def %d, max_rep %d)" % (leaf.max_def, leaf.max_rep))
        is_str = bool(strings) and leaf.type == BYTE_ARRAY
        if not is_str and (leaf.type in (BOOLEAN, BYTE_ARRAY) or leaf.type not in range(8)):
            raise no("physical type %s" % (TYPE_NAMES[leaf.type] if leaf.type in range(8)
                                           else leaf.type))
        if not is_str and (not leaf.width or not 1 <= leaf.width <= 256):
            raise no("a value width of %r bytes (1 .. 256)" % (leaf.width,))
        out_at, valid_at = _align(out_at), _align(valid_at)
        col = Column(name, out_at, valid_at if leaf.max_def else None, total, leaf)
        layout[name] = col
        # what a slot takes of d_out: a value, or an int64 offset
        step = 8 if is_str else leaf.width
        base = binding.PARQUET_DATA_V1 | leaf.max_def << 13 | \
            (binding.PARQUET_BYTE_ARRAY if is_str else (leaf.width - 1) << 16)
        done = 0
        for g in groups:
            g_rows, chunks = f.row_groups[g]
            ch = chunks[f.leaf_index(name)]
            if ch.codec not in (UNCOMPRESSED, GZIP):
                raise no("codec %s" % (CODEC_NAMES[ch.codec] if ch.codec < len(CODEC_NAMES)
                                       else ch.codec))
            if ch.start < 4 or ch.start + ch.nbytes > len(buf) - 8:
                raise no("its pages leave the file")
            at, end, slots, dict_row, mean = ch.start, ch.start + ch.nbytes, 0, None, 0
            while at < end and slots < ch.num_values:
                th = Thrift(buf, at)
                ph = th.struct()
                body, kind = th.at, ph.get(1)
                usize, csize = ph.get(2, -1), ph.get(3, -1)
                if usize < 0 or csize < 0 or body + csize > end:
                    raise no("a page that leaves its chunk")
                at = body + csize
                packed = ch.codec == GZIP
                word4 = 0
                if kind == DICTIONARY_PAGE:
                    h = ph.get(7, {})
                    if h.get(2, PLAIN) not in (PLAIN, PLAIN_DICTIONARY):
                        raise no("a dictionary page with encoding %d" % h.get(2))
                    if dict_row is not None:
                        raise no("a second dictionary page in one chunk")
                    dict_row = len(rows)
                    word3 = (base & ~(1 << 13)) | binding.PARQUET_DICT
                    word4 = h.get(1, 0)
                    # the mean entry, rounded up: what an index is estimated to take
                    mean = -(-max(usize - 4 * word4, 0) // max(word4, 1))
                elif kind in (DATA_PAGE, DATA_PAGE_V2):
                    h = ph.get(5 if kind == DATA_PAGE else 8)
                    if h is None:
                        raise no("a data page without its header")
                    enc = h.get(2 if kind == DATA_PAGE else 4)
                    if enc not in (PLAIN, PLAIN_DICTIONARY, RLE_DICTIONARY):
                        raise no("encoding %r" % (enc,))
                    if enc != PLAIN and dict_row is None:
                        raise no("a dictionary-coded page without a dictionary page")
                    word3, word4 = base | enc << 4, h.get(1, 0)
                    if kind == DATA_PAGE:
                        if leaf.max_def and h.get(3, RLE) != RLE:
                            raise no("definition levels with encoding %d" % h.get(3))
                    else:
                        if h.get(6, 0):
                            raise no("repetition levels in a flat column")
                        if h.get(5, 0) and not leaf.max_def:
                            raise no("definition levels in a required column")
                        word3 = (word3 & ~15) | binding.PARQUET_DATA_V2
                        word4 |= h.get(5, 0) << 32
                        packed = packed and h.get(7, True)
                    n = word4 & 0xFFFFFFFF
                    if slots + n > g_rows:
                        raise no("more values than the row group has rows")
                elif kind == INDEX_PAGE:
                    continue
                else:
                    raise no("page type %r" % (kind,))
                if packed and fmt is None:
                    skip = word4 >> 32
                    fmt = _format_of(bytes(buf[body + skip:body + skip + 2]))
                row = [body, csize, usize, word3 | int(packed) << 12, word4, 0, 0, 0]
                if kind != DICTIONARY_PAGE:
                    row[5] = col.offset + (done + slots) * step
                    if is_str:
                        estimate += n * mean if (word3 >> 4 & 255) != PLAIN else usize
                    row[6] = col.valid_offset + done + slots if leaf.max_def else 0
                    row[7] = dict_row if (word3 >> 4 & 255) != PLAIN else 0
                    slots += n
                rows.append(row)
            if slots != g_rows:
                raise no("%d values in a row group of %d rows" % (slots, g_rows))
            done += g_rows
        out_at += (total + 1) * 8 if is_str else total * leaf.width
        valid_at += total if leaf.max_def else 0
    r = np.array(rows, dtype=np.uint64).reshape(-1, binding.PARQUET_WORDS)
    return Pages(r, fmt or "gzip", layout, _align(out_at), _align(valid_at), estimate)


def read_columns(dec, buf, d_in, columns=None, row_groups=None, stream=None, bytes_estimate=None):
    """The selected columns of the file `buf` (host bytes), whose copy in device
    memory is d_in (uint8 CUDA tensor), decoded by dec
    (libdeflate_amd.Decompressor).  -> {name: (values, mask)}: values a tensor
    of the column's type - INT96 and FIXED_LEN_BYTE_ARRAY as uint8 [rows,
    width] - with zeros where null, or for a BYTE_ARRAY column the pair
    (offsets int64 [rows + 1] from 0, bytes uint8); mask a torch.bool tensor,
    True where valid, or None for a required column.  The strings' room is
    estimated from the page headers (bytes_estimate: instead of that); only
    where a page then ends as INSUFFICIENT_SPACE the call is made again with
    the room it reported.  Waits for the device and raises if a page failed."""
    import torch
    f = parse(buf)
    names = [leaf.name for leaf in f.leaves] if columns is None else list(columns)
    strings = any(f.leaves[f.leaf_index(n)].type == BYTE_ARRAY for n in names)
    pg = pages(buf, names, row_groups, file=f, strings=strings)
    out = torch.empty(max(pg.out_nbytes, ALIGN), dtype=torch.uint8, device=d_in.device)
    valid = torch.empty(max(pg.valid_nbytes, ALIGN), dtype=torch.uint8, device=d_in.device)
    results = torch.empty(max(len(pg.rows), 1), dtype=torch.int32, device=d_in.device)
    data = None
    if not strings:
        dec.parquet_decode_batch(pg.format, pg.rows, d_in, out, valid, results, stream=stream)
        res = results[:len(pg.rows)].cpu().numpy()
    else:
        room = pg.bytes_estimate if bytes_estimate is None else int(bytes_estimate)
        total = torch.zeros(1, dtype=torch.int64, device=d_in.device)
        for _ in range(2):
            data = torch.empty(room, dtype=torch.uint8, device=d_in.device)
            dec.parquet_decode_batch_ex(pg.format, pg.rows, d_in, out, valid, data, total, results,
                                        stream=stream)
            res = results[:len(pg.rows)].cpu().numpy()
            if not (res == 3).any() or int(total.item()) <= room:    # INSUFFICIENT_SPACE
                break
            room = int(total.item())
    if res.any():
        k = int(np.flatnonzero(res)[0])
        raise ValueError("parquet: page row %d failed with libdeflate_result %d" % (k, res[k]))
    cols = {}
    for name, c in pg.columns.items():
        m = None
        if c.valid_offset is not None:
            m = valid[c.valid_offset:c.valid_offset + c.rows].view(torch.bool)
        if c.byte_array:
            o = out[c.offset:c.offset + (c.rows + 1) * 8].view(torch.int64)
            first, last = int(o[0].item()), int(o[-1].item())
            cols[name] = ((o - first, data[first:last]), m)
            continue
        v = out[c.offset:c.offset + c.rows * c.width]
        v = v.view(getattr(torch, c.dtype)) if c.dtype else v.view(c.rows, c.width)
        cols[name] = (v, m)
    return cols
