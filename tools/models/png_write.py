"""The PNG writer's rule on the CPU (libdeflate_amd_png_encode_bound /
_png_encode_batch, include/libdeflate_amd.h): the refusals, the bound, the
filtered scanlines of an image row - the five filters of the PNG specification
9.2 on whole images in numpy, and the adaptive choice by the least sum of
absolute values - and the files, result words and index rows assembled around
per-image zlib streams that the caller supplies (the GPU tests feed the
object's own libdeflate_zlib_compress() of scanlines(); tests/test_png_write_model.py
feeds zlib.compress and reads the files back with png_model and PIL)."""
import struct
import zlib

import numpy as np

from tools.models import png_model as pm

ADAPTIVE = 5
RESULT_WORDS = 4
INSUFFICIENT_SPACE = 3
LE16 = pm.LE16
MASK48 = (1 << 48) - 1


def zlib_bound(n):
    """libdeflate_zlib_compress_bound"""
    return 6 + 5 * max(1, (n + 4999) // 5000) + n


def geometry(row):
    """(width, height, depth, colour, rowbytes, unit) of an image row"""
    w, h = int(row[2]) & 0xFFFFFFFF, int(row[2]) >> 32
    depth, colour = int(row[3]) & 0xFF, int(row[3]) >> 8 & 0xFF
    return w, h, depth, colour, pm.rowbytes(w, depth, colour), pm.bpp(depth, colour)


def refusal(row, in_avail=None, level=6):
    """None, or why the call refuses the row (in_avail None: as the bound sees it)"""
    row = [int(x) for x in row]
    w, h = row[2] & 0xFFFFFFFF, row[2] >> 32
    depth, colour = row[3] & 0xFF, row[3] >> 8 & 0xFF
    if not 1 <= w <= pm.MAX_DIM or not 1 <= h <= pm.MAX_DIM:
        return "width"
    if colour not in pm.DEPTHS or depth not in pm.DEPTHS[colour]:
        return "bit depth"
    if row[3] >> 16 & 0xFF:
        return "interlaced"
    rb = pm.rowbytes(w, depth, colour)
    scan = h * (1 + rb)
    if scan >= 1 << 32:
        return "2^32"
    if row[1] != h * rb:
        return "word 1"
    if level == 0 and scan > 0xFFFFFF00:
        return "level-0"
    if zlib_bound(scan) > (1 << 31) - 1:
        return "zlib bound"
    if in_avail is not None and (row[0] > in_avail or in_avail - row[0] < h * rb):
        return "pixels"
    entries = 0
    if row[6]:
        off, entries = row[6] & MASK48, row[6] >> 48
        if colour in (0, 4):
            return "PLTE"
        if not 1 <= entries <= 256 or (colour == 3 and entries > 1 << depth):
            return "PLTE"
        if in_avail is not None and (off > in_avail or in_avail - off < 3 * entries):
            return "PLTE"
    elif colour == 3:
        return "PLTE"
    if row[7]:
        off, length = row[7] & MASK48, row[7] >> 48
        if colour in (4, 6):
            return "tRNS"
        if (colour == 0 and length != 2) or (colour == 2 and length != 6) or \
                (colour == 3 and not 1 <= length <= entries):
            return "tRNS"
        if in_avail is not None and (off > in_avail or in_avail - off < length):
            return "tRNS"
    return None


def head_size(row):
    """bytes of the file in front of the IDAT payload"""
    e, t = int(row[6]) >> 48, int(row[7]) >> 48
    return 8 + 25 + (12 + 3 * e if e else 0) + (12 + t if t else 0) + 8


def bound(rows, level=6):
    """libdeflate_amd_png_encode_bound: 0 for rows the call refuses"""
    total = 0
    for row in rows:
        if refusal(row, None, level):
            return 0
        w, h, depth, colour, rb, unit = geometry(row)
        total += head_size(row) + zlib_bound(h * (1 + rb)) + 4 + 12
    return total


def _shift(a, unit):
    """every row's bytes `unit` to the right, zeros in front"""
    out = np.zeros_like(a)
    if unit < a.shape[1]:
        out[:, unit:] = a[:, :-unit]
    return out


def filtered(pixels, height, rb, unit):
    """the five filtered forms of an image: uint8 (5, height, rb)"""
    cur = np.frombuffer(pixels, dtype=np.uint8).reshape(height, rb).astype(np.int32)
    up = np.zeros_like(cur)
    up[1:] = cur[:-1]
    a, c = _shift(cur, unit), _shift(up, unit)
    p = a + up - c
    pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
    preds = [np.zeros_like(cur), a, up, (a + up) >> 1, paeth]
    return np.stack([((cur - q) & 0xFF).astype(np.uint8) for q in preds])


def choose(cand):
    """per row the type with the least sum of |signed byte|, the lowest on ties"""
    sums = np.abs(cand.view(np.int8).astype(np.int64)).sum(axis=2)
    return np.argmin(sums, axis=0)


def scanlines(pixels, height, rb, unit, filt):
    """-> (the filtered scanlines with their filter bytes, the types chosen)"""
    cand = filtered(pixels, height, rb, unit)
    types = choose(cand) if filt == ADAPTIVE else np.full(height, filt, dtype=np.int64)
    raw = np.empty((height, rb + 1), dtype=np.uint8)
    raw[:, 0] = types
    raw[:, 1:] = cand[types, np.arange(height)]
    return raw.tobytes(), types.tolist()


def image_pixels(row, data, flags=0):
    """the image's pixel bytes in PNG order"""
    w, h, depth, colour, rb, unit = geometry(row)
    pixels = bytes(data[int(row[0]):int(row[0]) + h * rb])
    return pm.swap16(pixels) if flags & LE16 and depth == 16 else pixels


def image_scanlines(row, data, filt=ADAPTIVE, flags=0):
    """what the image's zlib stream holds -> (bytes, types)"""
    w, h, depth, colour, rb, unit = geometry(row)
    return scanlines(image_pixels(row, data, flags), h, rb, unit, filt)


def _chunk(ctype, body):
    return struct.pack(">I", len(body)) + ctype + body + \
        struct.pack(">I", zlib.crc32(ctype + body))


def encode(rows, data, streams, out_avail=None):
    """rows, the input buffer and every image's zlib stream -> (files, result
    words, index rows).  The files stand back to back from offset 0; under
    INSUFFICIENT_SPACE (the total above out_avail) files and index are None."""
    files, index, at, pixel_bytes = [], [], 0, 0
    for row, z in zip(rows, streams):
        row = [int(x) for x in row]
        w, h, depth, colour, rb, unit = geometry(row)
        e, t = row[6] >> 48, row[7] >> 48
        parts = [pm.SIGNATURE,
                 _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, 0))]
        plte_at = trns_at = 0
        if e:
            plte_at = at + sum(map(len, parts)) + 8
            off = row[6] & MASK48
            parts.append(_chunk(b"PLTE", bytes(data[off:off + 3 * e])))
        if t:
            trns_at = at + sum(map(len, parts)) + 8
            off = row[7] & MASK48
            parts.append(_chunk(b"tRNS", bytes(data[off:off + t])))
        idat_at = at + sum(map(len, parts))
        parts += [_chunk(b"IDAT", z), _chunk(b"IEND", b"")]
        f = b"".join(parts)
        assert idat_at - at + 8 == head_size(row)
        index.append([at, len(f), row[2],
                      depth | colour << 8 | unit << 24 | pm.channels(colour) << 32,
                      idat_at, len(z), plte_at | e << 48 if e else 0,
                      trns_at | t << 48 if t else 0])
        files.append(f)
        at += len(f)
        pixel_bytes += h * rb
    ok = out_avail is None or at <= out_avail
    result = [0 if ok else INSUFFICIENT_SPACE, at, pixel_bytes, len(files)]
    return (files, result, index) if ok else (None, result, None)
