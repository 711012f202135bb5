"""PNG files built by hand (struct, zlib, zlib.crc32) for the PNG reader's
tests and benchmark: any valid depth and colour type, a chosen filter type per
row or the minimum-sum-of-absolute-differences choice, a chosen split of the
zlib stream into IDAT chunks, extra ancillary chunks, and every defect the
reader has a verdict for."""
import collections
import random
import struct
import zlib

import numpy as np

from tools.models import png_model as pm

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE, UNSUPPORTED = 0, 1, 2, 3, 18

# a built file: its bytes, the pixel bytes it holds (height * rowbytes, PNG
# order; None where it is not meant to decode) and the IHDR fields
Png = collections.namedtuple("Png", "data pixels width height depth colour")


def chunk(ctype, data=b"", crc=None):
    body = ctype + data
    return struct.pack(">I", len(data)) + body + \
        struct.pack(">I", zlib.crc32(body) if crc is None else crc)


def ihdr(width, height, depth, colour, comp=0, filt=0, interlace=0, crc=None):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour, comp, filt,
                                      interlace), crc)


def pixels_random(width, height, depth, colour, seed):
    """uniform random bytes (the unused low bits of a last byte are zero)"""
    rb = pm.rowbytes(width, depth, colour)
    a = np.random.RandomState(seed).randint(0, 256, (height, rb)).astype(np.uint8)
    spare = rb * 8 - width * pm.channels(colour) * depth
    if spare:
        a[:, -1] &= (0xFF << spare) & 0xFF
    return a.tobytes()


def pixels_constant(width, height, depth, colour, value=0x5A):
    rb = pm.rowbytes(width, depth, colour)
    a = np.full((height, rb), value, dtype=np.uint8)
    spare = rb * 8 - width * pm.channels(colour) * depth
    if spare:
        a[:, -1] &= (0xFF << spare) & 0xFF
    return a.tobytes()


def pixels_smooth(width, height, depth, colour, seed):
    """a gradient with a little noise: what adaptive filters are chosen for"""
    rb = pm.rowbytes(width, depth, colour)
    y, x = np.mgrid[0:height, 0:rb]
    noise = np.random.RandomState(seed).randint(0, 4, (height, rb))
    a = ((x * 3 + y * 5) // 2 + noise).astype(np.uint8)
    spare = rb * 8 - width * pm.channels(colour) * depth
    if spare:
        a[:, -1] &= (0xFF << spare) & 0xFF
    return a.tobytes()


def _filter_row(ft, cur, prev, unit):
    """the filtered bytes of a scanline (numpy uint8 in, PNG specification 9.2)"""
    a = np.zeros_like(cur)
    a[unit:] = cur[:-unit] if unit < len(cur) else cur[:0]
    c = np.zeros_like(cur)
    c[unit:] = prev[:-unit] if unit < len(cur) else prev[:0]
    if ft == 1:
        pred = a
    elif ft == 2:
        pred = prev
    elif ft == 3:
        pred = ((a.astype(np.int32) + prev) >> 1).astype(np.uint8)
    elif ft == 4:
        ai, bi, ci = a.astype(np.int32), prev.astype(np.int32), c.astype(np.int32)
        p = ai + bi - ci
        pa, pb, pc = abs(p - ai), abs(p - bi), abs(p - ci)
        pred = np.where((pa <= pb) & (pa <= pc), ai, np.where(pb <= pc, bi, ci)).astype(np.uint8)
    else:
        return cur.copy()       # type 0, and a type there is not
    return (cur - pred).astype(np.uint8)


def scanlines(pixels, height, rb, unit, filters):
    """The filtered scanlines with their filter bytes.  filters: an int (every
    row), a sequence (one per row; a value above 4 is written as it is in front
    of unfiltered bytes), "random:<seed>" or "adaptive" (per row the type whose
    filtered bytes, as signed, have the least sum of absolute values)."""
    img = np.frombuffer(pixels, dtype=np.uint8).reshape(height, rb)
    if isinstance(filters, int):
        filters = [filters] * height
    elif isinstance(filters, str) and filters.startswith("random"):
        rng = random.Random(int(filters.split(":")[1]) if ":" in filters else 0)
        filters = [rng.randrange(5) for _ in range(height)]
    prev = np.zeros(rb, dtype=np.uint8)
    raw = bytearray()
    for y in range(height):
        cur = img[y]
        if filters == "adaptive":
            cand = [_filter_row(t, cur, prev, unit) for t in range(5)]
            ft = int(np.argmin([np.abs(f.view(np.int8).astype(np.int32)).sum() for f in cand]))
            line = cand[ft]
        else:
            ft = filters[y]
            line = _filter_row(ft, cur, prev, unit)
        raw.append(ft)
        raw += line.tobytes()
        prev = cur
    return bytes(raw)


def split(z, how):
    """the zlib stream in IDAT chunks: None (one chunk), an int (chunks of that
    many bytes) or a list of lengths (a last chunk takes what is left; zeros
    make empty chunks)"""
    if how is None:
        return [z]
    if isinstance(how, int):
        return [z[i:i + how] for i in range(0, len(z), how)] or [b""]
    parts, at = [], 0
    for n in how:
        parts.append(z[at:at + n])
        at += n
    if at < len(z):
        parts.append(z[at:])
    return parts


def palette(entries=256):
    return bytes((i * 7 + k * 85) & 0xFF for i in range(entries) for k in range(3))


def make(width, height, depth=8, colour=2, pixels=None, filters="adaptive", idat=None,
         before=(), after=(), level=6, seed=1, plte=None, trns=None, interlace=0,
         rows_delta=0, damage=None, tail=b""):
    """A PNG file.  pixels: height * rowbytes bytes (default: random).  before /
    after: (type, data) chunks in front of and behind the IDAT run.  plte: the
    PLTE data (default: 256 entries for colour type 3, none otherwise).
    rows_delta: scanlines dropped (-1) or repeated (+1) at the stream's end.
    damage(z) -> z: applied to the zlib stream before it is split.  tail: bytes
    behind IEND."""
    rb, unit = pm.rowbytes(width, depth, colour), pm.bpp(depth, colour)
    if pixels is None:
        pixels = pixels_random(width, height, depth, colour, seed)
    raw = scanlines(pixels, height, rb, unit, filters)
    if rows_delta < 0:
        raw = raw[:(height + rows_delta) * (rb + 1)]
    elif rows_delta > 0:
        raw += raw[-(rb + 1):] * rows_delta
    z = zlib.compress(raw, level)
    if damage:
        z = damage(z)
    if plte is None and colour == 3:
        plte = palette(min(256, 1 << depth))
    out = [pm.SIGNATURE, ihdr(width, height, depth, colour, interlace=interlace)]
    if plte is not None:
        out.append(chunk(b"PLTE", plte))
    if trns is not None:
        out.append(chunk(b"tRNS", trns))
    out += [chunk(t, d) for t, d in before]
    out += [chunk(b"IDAT", p) for p in split(z, idat)]
    out += [chunk(t, d) for t, d in after]
    out += [chunk(b"IEND"), tail]
    return Png(b"".join(out), pixels, width, height, depth, colour)


# ---- the defects: name -> (file bytes, the index call's verdict) ----

def _parts(width=5, height=3, depth=8, colour=2):
    """(ihdr, idat chunks joined, iend) of a small good file"""
    g = make(width, height, depth, colour, seed=9, filters=0)
    return g.data[8:33], g.data[33:-12], g.data[-12:]


def defects():
    sig = pm.SIGNATURE
    head, body, iend = _parts()
    idat = body
    text = chunk(b"tEXt", b"k\0v")
    pal = make(4, 4, 8, 3, seed=3)
    pal_body = pal.data[33:]
    pal_plte_len = 12 + 768
    out = collections.OrderedDict()

    def add(name, data, verdict):
        out[name] = (data, verdict)
    add("signature", b"\x89PNG\r\n\x1a\r" + head + body + iend, BAD_DATA)
    add("first_not_ihdr", sig + text + head + body + iend, BAD_DATA)
    add("ihdr_length", sig + chunk(b"IHDR", struct.pack(">IIBBBBBB", 5, 3, 8, 2, 0, 0, 0, 0)) +
        body + iend, BAD_DATA)
    add("ihdr_crc", sig + ihdr(5, 3, 8, 2, crc=0x12345678) + body + iend, BAD_DATA)
    add("width_0", sig + ihdr(0, 3, 8, 2) + body + iend, BAD_DATA)
    add("height_0", sig + ihdr(5, 0, 8, 2) + body + iend, BAD_DATA)
    add("width_2_31", sig + ihdr(1 << 31, 3, 8, 2) + body + iend, BAD_DATA)
    add("height_2_31", sig + ihdr(5, 1 << 31, 8, 2) + body + iend, BAD_DATA)
    add("depth_3", sig + ihdr(5, 3, 3, 0) + body + iend, BAD_DATA)
    add("rgb_depth_4", sig + ihdr(5, 3, 4, 2) + body + iend, BAD_DATA)
    add("palette_depth_16", sig + ihdr(5, 3, 16, 3) + chunk(b"PLTE", palette(4)) + body + iend,
        BAD_DATA)
    add("colour_5", sig + ihdr(5, 3, 8, 5) + body + iend, BAD_DATA)
    add("compression_1", sig + ihdr(5, 3, 8, 2, comp=1) + body + iend, BAD_DATA)
    add("filter_method_1", sig + ihdr(5, 3, 8, 2, filt=1) + body + iend, BAD_DATA)
    add("interlace_2", sig + ihdr(5, 3, 8, 2, interlace=2) + body + iend, BAD_DATA)
    add("chunk_past_end", sig + head + body[:-6], BAD_DATA)
    add("length_huge", sig + head + struct.pack(">I", 0xFFFFFFF0) + body[4:] + iend, BAD_DATA)
    add("no_idat", sig + head + text + iend, BAD_DATA)
    add("idat_after_run", sig + head + idat + text + idat + iend, BAD_DATA)
    add("second_ihdr", sig + head + head + body + iend, BAD_DATA)
    add("palette_without_plte", pal.data[:33] + pal_body[pal_plte_len:], BAD_DATA)
    add("plte_behind_idat", pal.data[:33] + pal_body[pal_plte_len:-12] +
        pal_body[:pal_plte_len] + iend, BAD_DATA)
    add("plte_length_4", sig + head + chunk(b"PLTE", bytes(4)) + body + iend, BAD_DATA)
    add("plte_length_771", sig + head + chunk(b"PLTE", bytes(771)) + body + iend, BAD_DATA)
    add("second_plte", sig + head + chunk(b"PLTE", bytes(3)) + chunk(b"PLTE", bytes(3)) + body +
        iend, BAD_DATA)
    add("no_iend", sig + head + body, BAD_DATA)
    add("no_iend_text", sig + head + body + text, BAD_DATA)
    add("short", sig + head, BAD_DATA)
    add("empty", b"", BAD_DATA)
    add("adam7", sig + ihdr(5, 3, 8, 2, interlace=1) + body + iend, UNSUPPORTED)
    add("critical_unknown", sig + head + chunk(b"ABCD", b"xyz") + body + iend, UNSUPPORTED)
    add("critical_behind_idat", sig + head + body + chunk(b"QxYz") + iend, UNSUPPORTED)
    add("raw_2_32", sig + ihdr(65536, 16384, 8, 6) + body + iend, UNSUPPORTED)
    add("raw_2_32_wide", sig + ihdr((1 << 31) - 1, 1, 16, 6) + body + iend, UNSUPPORTED)
    # BAD_DATA comes first where both apply
    add("adam7_no_iend", sig + ihdr(5, 3, 8, 2, interlace=1) + body, BAD_DATA)
    return out
