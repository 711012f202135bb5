"""The rule of the PNG reader's calls that take Adam7-interlaced files
(libdeflate_amd_png_index_batch_ex / _png_out_sizes_ex / _png_decode_batch_ex,
include/libdeflate_amd.h) on the CPU, on top of png_model.py and
png_pixels_model.py: the geometry of the seven passes, the bytes an interlaced
stream inflates to, the weaving of pass images into an image and back, the
index with its flag, and the decode of one selection in either layout.  The
GPU tests compare every row word, result and pixel byte with this;
tests/test_png_adam7_model.py pins it against PIL."""
import struct
import zlib

import numpy as np

from tools.models import png_model as pm
from tools.models import png_pixels_model as px

SUCCESS, BAD_DATA, UNSUPPORTED = pm.SUCCESS, pm.BAD_DATA, pm.UNSUPPORTED
LE16, ADAM7 = pm.LE16, 2
# (x0, y0, dx, dy) of the passes, PNG specification 8.2
PASSES = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2),
          (0, 1, 1, 2))
TILE = 1024     # 16-byte pieces of a tile of the deinterlace kernel


def pass_sizes(width, height):
    """[(w_p, h_p)] of the seven passes; an absent pass is (0, 0)"""
    out = []
    for x0, y0, dx, dy in PASSES:
        w = -(-(width - x0) // dx) if width > x0 else 0
        h = -(-(height - y0) // dy) if height > y0 else 0
        out.append((w, h) if w and h else (0, 0))
    return out


def pass_geometry(width, height, depth, colour):
    """[(w_p, h_p, rb_p)], zeros for an absent pass"""
    return [(w, h, pm.rowbytes(w, depth, colour) if w else 0) for w, h in pass_sizes(width, height)]


def raw7(width, height, depth, colour):
    """the bytes the zlib stream of an interlaced image inflates to"""
    return sum(h * (1 + rb) for _, h, rb in pass_geometry(width, height, depth, colour))


def _unpack(pixels, width, height, depth, colour):
    """height * rowbytes bytes -> (height, width) of bits-per-pixel-wide units:
    a 2-d array of (height, width * bits) bits below 8 bits a pixel, of
    (height, width, bytes) bytes from there"""
    bits = depth * pm.CHANNELS[colour]
    rows = np.frombuffer(pixels, dtype=np.uint8).reshape(height, pm.rowbytes(width, depth, colour))
    if bits >= 8:
        return rows.reshape(height, width, bits // 8)
    return np.unpackbits(rows, axis=1)[:, :width * bits].reshape(height, width, bits)


def _pack(units, depth, colour):
    """the inverse of _unpack for an image of units.shape[:2]; spare bits zero"""
    h, w = units.shape[:2]
    if depth * pm.CHANNELS[colour] >= 8:
        return np.ascontiguousarray(units).tobytes()
    return np.packbits(units.reshape(h, -1), axis=1).tobytes()


def interlace(pixels, width, height, depth, colour):
    """an image's bytes (height * rowbytes) -> the seven pass images' bytes
    (h_p * rb_p each, b"" for an absent pass)"""
    units = _unpack(pixels, width, height, depth, colour)
    out = []
    for (x0, y0, dx, dy), (w, h) in zip(PASSES, pass_sizes(width, height)):
        out.append(_pack(units[y0::dy, x0::dx], depth, colour) if w else b"")
    return out


def deinterlace(passes, width, height, depth, colour):
    """the inverse of interlace(); the spare bits of a row's last byte are zero"""
    bits = depth * pm.CHANNELS[colour]
    units = np.zeros((height, width, bits // 8 if bits >= 8 else bits), dtype=np.uint8)
    for (x0, y0, dx, dy), (w, h), data in zip(PASSES, pass_sizes(width, height), passes):
        if w:
            units[y0::dy, x0::dx] = _unpack(data, w, h, depth, colour)
    return _pack(units, depth, colour)


def is_interlaced(row):
    return (row[3] >> 16 & 0xFF) != 0


def plain_twin(row):
    """the row with its interlace byte cleared"""
    return row[:3] + [row[3] & ~(0xFF << 16)] + row[4:]


def index(buf, off=0, n=None, flags=0):
    """The file buf[off : off + n] -> (result, row of 8 words): png_model's for
    flags 0 and for every file that is not interlaced; with ADAM7 an interlaced
    file is indexed as its twin, with bit 16 of word 3 set, and UNSUPPORTED only
    where the image or raw7 reaches 2^32."""
    n = len(buf) - off if n is None else n
    res, row = pm.index(buf, off, n)
    if not flags & ADAM7 or res != UNSUPPORTED or n < 33 or buf[off + 28] != 1:
        return res, row
    # (UNSUPPORTED: every BAD_DATA rule has passed) the same file, not interlaced
    head = bytearray(buf[off:off + n])
    head[28] = 0
    head[29:33] = struct.pack(">I", zlib.crc32(bytes(head[12:29])))
    res, row = pm.index(bytes(head), 0, n)
    if res != SUCCESS:
        return res, [off, n, 0, 0, 0, 0, 0, 0]
    h, w, _, depth, colour = pm.shape(row)
    if raw7(w, h, depth, colour) >= 1 << 32:
        return UNSUPPORTED, [off, n, 0, 0, 0, 0, 0, 0]
    row = [off, n, row[2], row[3] | 1 << 16, row[4] + off, row[5],
           row[6] + off if row[6] else 0, row[7] + off if row[7] else 0]
    return SUCCESS, row


def out_sizes(rows, sel, fmt=0, align=1):
    """-> the n_sel + 1 offsets: an interlaced row takes the room of its twin"""
    twins = [plain_twin(r) for r in rows]
    return px.out_sizes(twins, sel, fmt, align) if fmt else pm.out_sizes(twins, sel, align)


def decode_raw(buf, row, flags=0):
    """One selection in PNG's layout -> (result, height * rowbytes bytes or
    None).  A plain row: png_model.decode.  An interlaced one, the first of:
    UNSUPPORTED (a zero row), the gather's BAD_DATA, the zlib decoder's result
    against the exact fill of raw7, BAD_DATA for a filter byte above 4 in any
    pass, SUCCESS."""
    if pm.is_zero(row) or not is_interlaced(row):
        return pm.decode(buf, row, flags & LE16)
    h, w, _, depth, colour = pm.shape(row)
    geometry = pass_geometry(w, h, depth, colour)
    agrees, z = pm.gather(buf, row)
    if not agrees:
        return BAD_DATA, None
    res, raw = pm.inflate_exact(z, sum(hp * (1 + rb) for _, hp, rb in geometry))
    if res != SUCCESS:
        return res, None
    at, passes, good = 0, [], True
    for wp, hp, rb in geometry:
        ok, data = pm.unfilter(raw[at:at + hp * (1 + rb)], hp, rb, pm.bpp(depth, colour))
        good &= ok
        passes.append(data)
        at += hp * (1 + rb)
    if not good:
        return BAD_DATA, None
    pixels = deinterlace(passes, w, h, depth, colour)
    if flags & LE16 and depth == 16:
        pixels = pm.swap16(pixels)
    return SUCCESS, pixels


def decode(buf, row, flags=0, fmt=0):
    """One selection -> (result, bytes or None): fmt 0 is decode_raw, any other
    the pixel format of png_pixels_model (then BAD_DATA for a palette index out
    of range comes behind decode_raw's verdicts)."""
    if not fmt:
        return decode_raw(buf, row, flags)
    res, pixels = decode_raw(buf, row, 0)
    if res != SUCCESS:
        return res, None
    h, w, _, depth, colour = pm.shape(row)
    plte, trns = px.chunks_of(buf, row)
    return px.convert(pixels, w, h, depth, colour, fmt, plte, trns, flags & LE16)
