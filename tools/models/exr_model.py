"""The CPU model of OpenEXR's ZIP / ZIPS chunk coding and of the rows of the
OpenEXR calls (include/libdeflate_amd.h: libdeflate_amd_exr_decode_batch,
libdeflate_amd_exr_encode_batch; libdeflate_amd/csrc/exr_plan.h), in numpy and
plain Python.  The tests compare the device against it byte for byte.

A raw chunk holds its lines channel-planar: for every line, for every channel in
the file's order, the line's samples of that channel.  apply() codes it, undo()
is the inverse, expected() lays a raw chunk out as the reader must."""
import zlib

import numpy as np

WORDS, RESULT_WORDS, CHANNELS_MAX = 10, 4, 16
LINES, PIXELS = 0, 1
# exr_plan.h: the bytes a lane and a wave undo, the tiles of a workgroup
LANE, TILE, WG_TILES = 32, 2048, 4
# the row classes (exr_plan.h: EXR_C_*)
BAD, RAW_DIRECT, RAW_LAYOUT, ZLIB = 0, 1, 2, 3


def apply(raw):
    """raw chunk -> the coded bytes p that go into the zlib stream"""
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    n = len(a)
    if n == 0:
        return b""
    t = np.concatenate([a[0::2], a[1::2]])
    p = t.copy()
    p[1:] = t[1:] - t[:-1] + np.uint8(128)
    return p.tobytes()


def undo(coded):
    """the inverse of apply()"""
    p = np.frombuffer(bytes(coded), dtype=np.uint8)
    n = len(p)
    if n == 0:
        return b""
    t = np.cumsum(p, dtype=np.uint64) - np.uint64(128) * np.arange(n, dtype=np.uint64)
    t = (t & np.uint64(0xFF)).astype(np.uint8)
    h = (n + 1) // 2
    raw = np.empty(n, dtype=np.uint8)
    raw[0::2] = t[:h]
    raw[1::2] = t[h:]
    return raw.tobytes()


def data_of(raw, level=6):
    """what a file stores for a raw chunk: the zlib stream of the coded bytes
    where it is shorter than raw, else raw"""
    z = zlib.compress(apply(raw), level)
    return z if len(z) < len(raw) else bytes(raw)


def sizes_of(wide):
    return [4 if w else 2 for w in wide]


def row(data_off, data_n, pix_off, pitch, size, wide, layout=LINES, slots=None, head=()):
    """a row as api.exr_rows() makes it, as a list of ints"""
    c = len(wide)
    fmt = c | sum(1 << (8 + k) for k in range(c) if wide[k]) | layout << 32
    slot_word = 0
    if layout == PIXELS:
        for k, s in enumerate(range(c) if slots is None else slots):
            slot_word |= s << (4 * k)
    v = [x & 0xFFFFFFFF for x in head] + [0, 0, 0, 0]
    return [data_off, data_n, pix_off, pitch, size[0] | size[1] << 32, fmt, slot_word,
            4 * len(head) + 4 if head else 0, v[0] | v[1] << 32, v[2] | v[3] << 32]


def fields(r):
    """(width, lines, wide[], layout, slots[]) of a row"""
    r = [int(x) for x in r]
    c = r[5] & 0xFF
    wide = [bool(r[5] >> (8 + k) & 1) for k in range(c)]
    return r[4] & 0xFFFFFFFF, r[4] >> 32, wide, r[5] >> 32, [r[6] >> (4 * k) & 15 for k in range(c)]


def raw_size(r):
    w, lines, wide, _, _ = fields(r)
    return w * lines * sum(sizes_of(wide))


def row_why(r, reader, stored_avail, pix_avail, level=-1):
    """a word of the reason either call refuses the row with, or None
    (exr_plan.h: exr_row_why, in its order)"""
    r = [int(x) for x in r]
    c, mask, layout = r[5] & 0xFF, r[5] >> 8 & 0xFFFF, r[5] >> 32
    if r[5] >> 24 & 0xFF or r[5] >> 33:
        return "unknown bits"
    if not 1 <= c <= CHANNELS_MAX:
        return "channels"
    if mask >> c:
        return "wide-mask"
    w, lines = r[4] & 0xFFFFFFFF, r[4] >> 32
    if w == 0 or lines == 0:
        return "zero"
    if layout == LINES:
        if r[6]:
            return "word 6"
    elif sorted(r[6] >> (4 * k) & 15 for k in range(c)) != list(range(c)) or (c < 16 and r[6] >> (4 * c)):
        return "permutation"
    if r[7] not in (0, 8, 20):
        return "head length"
    lb = w * sum(4 if mask >> k & 1 else 2 for k in range(c))
    if lb * lines >= 1 << 32:
        return "2^32"
    if reader and r[0] + r[1] > stored_avail:
        return "in_nbytes"
    if lines > 1 and r[3] < lb:
        return "pitch"
    if r[2] + (lines - 1) * (r[3] if lines > 1 else 0) + lb > pix_avail:
        return "out_avail" if reader else "in_avail"
    if not reader and level == 0 and lb * lines > 0xFFFFFF00:
        return "level-0"
    return None


def bound(rows):
    if any(row_why(r, False, 0, (1 << 64) - 1) for r in rows):
        return 0
    return sum(int(r[7]) + raw_size(r) for r in rows)


def direct(r):
    w, lines, wide, layout, _ = fields(r)
    return layout == LINES and (lines == 1 or int(r[3]) == w * sum(sizes_of(wide)))


def classify(r):
    n = raw_size(r)
    if int(r[1]) > n:
        return BAD
    if int(r[1]) == n:
        return RAW_DIRECT if direct(r) else RAW_LAYOUT
    return ZLIB


def expected(r, raw):
    """the bytes of every line the reader writes for the raw chunk: line y
    stands at word 2 + y * word 3"""
    w, lines, wide, layout, slots = fields(r)
    sz = sizes_of(wide)
    px = sum(sz)
    a = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(lines, w * px)
    if layout == LINES:
        return [a[y].tobytes() for y in range(lines)]
    # where every channel stands in the pixel: behind the channels of lower slots
    by_slot = sorted(range(len(wide)), key=lambda k: slots[k])
    off, at = {}, 0
    for k in by_slot:
        off[k] = at
        at += sz[k]
    out = np.empty((lines, w, px), dtype=np.uint8)
    plane = 0
    for k in range(len(wide)):
        out[:, :, off[k]:off[k] + sz[k]] = a[:, plane:plane + w * sz[k]].reshape(lines, w, sz[k])
        plane += w * sz[k]
    return [out[y].tobytes() for y in range(lines)]


def gather(r, lines_bytes):
    """the inverse of expected(): the lines as the writer reads them -> raw"""
    w, lines, wide, layout, slots = fields(r)
    sz = sizes_of(wide)
    px = sum(sz)
    if layout == LINES:
        return b"".join(lines_bytes)
    by_slot = sorted(range(len(wide)), key=lambda k: slots[k])
    off, at = {}, 0
    for k in by_slot:
        off[k] = at
        at += sz[k]
    pix = np.frombuffer(b"".join(lines_bytes), dtype=np.uint8).reshape(lines, w, px)
    out = np.empty((lines, w * px), dtype=np.uint8)
    plane = 0
    for k in range(len(wide)):
        out[:, plane:plane + w * sz[k]] = pix[:, :, off[k]:off[k] + sz[k]].reshape(lines, w * sz[k])
        plane += w * sz[k]
    return out.tobytes()


def head_bytes(r, data_n):
    """the chunk head the writer puts in front of the data"""
    r = [int(x) for x in r]
    ints = [r[8] & 0xFFFFFFFF, r[8] >> 32, r[9] & 0xFFFFFFFF, r[9] >> 32]
    if r[7] == 0:
        return b""
    k = 1 if r[7] == 8 else 4
    return b"".join(v.to_bytes(4, "little") for v in ints[:k]) + int(data_n).to_bytes(4, "little")
