"""The PNG reader's rule on the CPU (libdeflate_amd_png_index_batch /
_png_out_sizes / _png_decode_batch, include/libdeflate_amd.h): the chunk walk
with its verdicts and its index row, the IDAT chain gathered against the row,
the zlib stream decoded with the exact-fill rule, and the five scanline filters
of the PNG specification undone in plain Python and numpy.  The GPU tests
compare every row word, result and pixel byte with this;
tests/test_png_model.py pins it against PIL."""
import struct
import zlib

import numpy as np

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
UNSUPPORTED = 18
WORDS = 8
LE16 = 1
SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_DIM = (1 << 31) - 1
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
# the 15 pairs of the specification, (depth, colour type)
COMBOS = [(d, c) for c in (0, 2, 3, 4, 6) for d in DEPTHS[c]]


def channels(colour):
    return CHANNELS[colour]


def bpp(depth, colour):
    """the filter unit: bytes per complete pixel, 1 below 8 bits"""
    return max(1, CHANNELS[colour] * depth // 8)


def rowbytes(width, depth, colour):
    return (width * CHANNELS[colour] * depth + 7) // 8


def index(buf, off=0, n=None):
    """The file buf[off : off + n] -> (result, row of 8 words)."""
    n = len(buf) - off if n is None else n
    f = bytes(buf[off:off + n])
    zero = [off, n, 0, 0, 0, 0, 0, 0]
    bad = (BAD_DATA, zero)
    if n < 33 + 12 or f[:8] != SIGNATURE:
        return bad
    length, ctype = struct.unpack(">I4s", f[8:16])
    if length != 13 or ctype != b"IHDR":
        return bad
    if zlib.crc32(f[12:29]) != struct.unpack(">I", f[29:33])[0]:
        return bad
    width, height, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", f[16:29])
    if not 1 <= width <= MAX_DIM or not 1 <= height <= MAX_DIM:
        return bad
    if colour not in DEPTHS or depth not in DEPTHS[colour] or comp or filt or interlace > 1:
        return bad
    pos, first, total, plte, trns = 33, 0, 0, 0, 0
    state, unknown = 0, False   # 0: in front of the IDAT run, 1: in it, 2: behind it
    while True:
        if n - pos < 12:
            return bad      # no IEND
        length, ctype = struct.unpack(">I4s", f[pos:pos + 8])
        if length > n - pos - 12:
            return bad
        if ctype == b"IEND":
            break
        if ctype == b"IDAT":
            if state == 2:
                return bad
            if state == 0:
                first = off + pos
            state = 1
            total += length
        else:
            if state == 1:
                state = 2
            if ctype == b"IHDR":
                return bad
            if ctype == b"PLTE":
                if length % 3 or length > 768 or plte:
                    return bad
                if state == 0:
                    plte = (off + pos + 8) | (length // 3) << 48
            elif ctype == b"tRNS":
                if state == 0 and not trns and length <= 0xFFFF:
                    trns = (off + pos + 8) | length << 48
            elif not ctype[0] & 0x20:
                unknown = True
        pos += 12 + length
    if state == 0 or (colour == 3 and not plte):
        return bad
    rb = rowbytes(width, depth, colour)
    if interlace or unknown or height * (1 + rb) >= 1 << 32:
        return UNSUPPORTED, zero
    return SUCCESS, [off, n, width | height << 32,
                     depth | colour << 8 | interlace << 16 | bpp(depth, colour) << 24 |
                     CHANNELS[colour] << 32, first, total, plte, trns]


def shape(row):
    """(height, width, channels, depth, colour) of a row, zeros for a zero row"""
    return (row[2] >> 32, row[2] & 0xFFFFFFFF, row[3] >> 32, row[3] & 0xFF, row[3] >> 8 & 0xFF)


def row_rowbytes(row):
    h, w, _, depth, colour = shape(row)
    return rowbytes(w, depth, colour)


def is_zero(row):
    return not any(row[2:])


def out_sizes(rows, sel, align=1):
    """-> the n_sel + 1 offsets of a selection in the output"""
    at, offs = 0, []
    for k in sel:
        offs.append(at)
        if not is_zero(rows[k]):
            size = (rows[k][2] >> 32) * row_rowbytes(rows[k])
            at += (size + align - 1) // align * align
    return offs + [at]


def gather(buf, row):
    """The IDAT run from the row's first IDAT on -> (the chain agrees with the
    row's sum, the bytes gathered)."""
    end, want = row[0] + row[1], row[5]
    pos, z = row[4], bytearray()
    while end - pos >= 12:
        length, ctype = struct.unpack(">I4s", bytes(buf[pos:pos + 8]))
        if ctype != b"IDAT":
            break
        if length > end - pos - 12 or length > want - len(z):
            return False, bytes(z)
        z += buf[pos + 8:pos + 8 + length]
        pos += 12 + length
    return len(z) == want, bytes(z)


def inflate_exact(z, size):
    """libdeflate_zlib_decompress into exactly `size` bytes -> (result, bytes)"""
    d = zlib.decompressobj()
    try:
        out = d.decompress(z, size + 1)
    except zlib.error:
        return BAD_DATA, None
    if len(out) > size:
        return INSUFFICIENT_SPACE, None
    if not d.eof:
        try:
            more = d.decompress(d.unconsumed_tail, 1)
        except zlib.error:
            return BAD_DATA, None
        if more:
            return INSUFFICIENT_SPACE, None
        if not d.eof:
            return BAD_DATA, None
    if len(out) < size:
        return SHORT_OUTPUT, None
    return SUCCESS, out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter(raw, height, rb, unit):
    """height scanlines of 1 + rb bytes -> (no filter byte above 4, height * rb
    bytes).  PNG specification 9.2; a row with a filter byte above 4 counts as
    type 0."""
    out = bytearray(height * rb)
    prev = bytes(rb)
    ok = True
    for y in range(height):
        ft = raw[y * (rb + 1)]
        line = raw[y * (rb + 1) + 1:(y + 1) * (rb + 1)]
        if ft > 4:
            ok, ft = False, 0
        if ft == 0:
            cur = bytes(line)
        elif ft == 1:
            a = np.frombuffer(line, dtype=np.uint8).reshape(-1, unit)
            cur = np.cumsum(a, axis=0, dtype=np.uint64).astype(np.uint8).tobytes()
        elif ft == 2:
            cur = (np.frombuffer(line, dtype=np.uint8) +
                   np.frombuffer(prev, dtype=np.uint8)).astype(np.uint8).tobytes()
        else:
            cur = bytearray(rb)
            for i in range(rb):
                a = cur[i - unit] if i >= unit else 0
                if ft == 3:
                    pred = (a + prev[i]) >> 1
                else:
                    pred = _paeth(a, prev[i], prev[i - unit] if i >= unit else 0)
                cur[i] = (line[i] + pred) & 0xFF
            cur = bytes(cur)
        out[y * rb:(y + 1) * rb] = cur
        prev = cur
    return ok, bytes(out)


def swap16(pixels):
    return np.frombuffer(pixels, dtype=">u2").astype("<u2").tobytes()


def decode(buf, row, flags=0):
    """One selection -> (result, the pixel bytes or None): the first of
    UNSUPPORTED (a zero row), the gather's BAD_DATA, the zlib decoder's result,
    BAD_DATA for a filter byte above 4, SUCCESS."""
    if is_zero(row):
        return UNSUPPORTED, None
    h, w, _, depth, colour = shape(row)
    rb = rowbytes(w, depth, colour)
    agrees, z = gather(buf, row)
    if not agrees:
        return BAD_DATA, None
    res, raw = inflate_exact(z, h * (1 + rb))
    if res != SUCCESS:
        return res, None
    ok, pixels = unfilter(raw, h, rb, bpp(depth, colour))
    if not ok:
        return BAD_DATA, None
    if flags & LE16 and depth == 16:
        pixels = swap16(pixels)
    return SUCCESS, pixels


def read(data, flags=0):
    """A whole file on its own -> (index result, row, decode result, pixels)"""
    res, row = index(data)
    if res != SUCCESS:
        return res, row, None, None
    dres, pixels = decode(data, row, flags)
    return res, row, dres, pixels
