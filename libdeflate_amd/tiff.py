"""The host side of the TIFF calls (libdeflate_amd_tiff_decode_batch,
libdeflate_amd_tiff_encode_batch): parse() walks the IFDs of a host copy of a
little-endian classic TIFF or BigTIFF and makes the segment rows the decode
call takes; build() assembles a classic little-endian TIFF from finished zlib
streams.  Pure Python and numpy: no device work, no other library.

    images = tiff.parse(buf)
    im = images[0]                     # width, height, spp, bps, predictor, ...
    rows = im.rows(offset=0)           # numpy uint64 (segments, 8): H x W x C at offset
    dec.decode_tiff_batch(rows, d_file, d_pixels, d_results)

Not covered, a plain ValueError: big-endian (MM) files, compressions other
than deflate (8, 32946) - LZW, JPEG, ZSTD, LERC, uncompressed -, sample sizes
that are not 8, 16, 32 or 64 bits or differ between the samples,
PlanarConfiguration = 2 with more than one sample per pixel, more than 16
samples per pixel, predictor 3 on 8-bit samples."""
import struct

import numpy as np

WORDS = 8
# tag numbers
WIDTH, HEIGHT, BITS, COMPRESSION, PHOTOMETRIC, STRIP_OFFSETS, SPP, ROWS_PER_STRIP, \
    STRIP_COUNTS, PLANAR, PREDICTOR, EXTRA_SAMPLES, TILE_WIDTH, TILE_LENGTH, TILE_OFFSETS, \
    TILE_COUNTS, SAMPLE_FORMAT = 256, 257, 258, 259, 262, 273, 277, 278, 279, 284, 317, 338, \
    322, 323, 324, 325, 339
DEFLATE = (8, 32946)
# field type -> (struct code, size)
_TYPES = {1: ("B", 1), 2: ("c", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8), 6: ("b", 1),
          7: ("B", 1), 8: ("h", 2), 9: ("i", 4), 10: ("ii", 8), 11: ("f", 4), 12: ("d", 8),
          13: ("I", 4), 16: ("Q", 8), 17: ("q", 8), 18: ("Q", 8)}


class Image:
    """One IFD: width, height, spp, bps (bytes per sample), sample_format,
    predictor, compression; the segments' geometry - tiled, seg_width,
    seg_rows (TileWidth x TileLength, or the image's width x RowsPerStrip),
    across, down - and where they are stored: offsets, counts."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def nbytes(self):
        return self.height * self.width * self.spp * self.bps

    def rows(self, offset=0, pitch=None):
        """the rows of libdeflate_amd_tiff_decode_batch for a height x width x
        spp image at `offset` of the raw buffer, `pitch` bytes between its
        rows (None: packed).  Edge tiles are cropped, the last strip is short."""
        px = self.spp * self.bps
        pitch = self.width * px if pitch is None else int(pitch)
        out = np.zeros((len(self.offsets), WORDS), dtype=np.uint64)
        for k in range(len(self.offsets)):
            ty, tx = divmod(k, self.across)
            x0, y0 = tx * self.seg_width, ty * self.seg_rows
            kw, kr = min(self.seg_width, self.width - x0), min(self.seg_rows, self.height - y0)
            # a strip is coded with the rows it has; a tile always whole
            cw, cr = (self.seg_width, self.seg_rows) if self.tiled else (self.width, kr)
            out[k] = [self.offsets[k], self.counts[k], offset + y0 * pitch + x0 * px, pitch,
                      cw | cr << 32, kw | kr << 32, self.spp | self.bps << 8 | self.predictor << 16, 0]
        return out


def _ifd(buf, at, big):
    """the entries of the IFD at `at` -> ({tag: tuple of values}, next IFD)"""
    cnt_fmt, ent, off_fmt = ("<Q", 20, "<Q") if big else ("<H", 12, "<I")
    csz, osz = struct.calcsize(cnt_fmt), struct.calcsize(off_fmt)
    if at + csz > len(buf):
        raise ValueError("tiff: an IFD outside the file")
    n = struct.unpack_from(cnt_fmt, buf, at)[0]
    if at + csz + n * ent + osz > len(buf):
        raise ValueError("tiff: an IFD outside the file")
    tags = {}
    for k in range(n):
        e = at + csz + k * ent
        tag, typ = struct.unpack_from("<HH", buf, e)
        count = struct.unpack_from(off_fmt, buf, e + 4)[0]
        if typ not in _TYPES:
            continue
        code, size = _TYPES[typ]
        where = e + 4 + osz
        if count * size > osz:
            where = struct.unpack_from(off_fmt, buf, where)[0]
        if where + count * size > len(buf):
            raise ValueError("tiff: tag %d outside the file" % tag)
        if typ == 2:
            tags[tag] = (bytes(buf[where:where + count]),)
        else:
            tags[tag] = struct.unpack_from("<%d%s" % (count * len(code), code[0]), buf, where)
    return tags, struct.unpack_from(off_fmt, buf, at + csz + n * ent)[0]


def _image(tags):
    def one(tag, default=None):
        v = tags.get(tag)
        if v is None:
            if default is None:
                raise ValueError("tiff: tag %d is missing" % tag)
            return default
        return int(v[0])
    width, height, spp = one(WIDTH), one(HEIGHT), one(SPP, 1)
    comp, pred, planar = one(COMPRESSION, 1), one(PREDICTOR, 1), one(PLANAR, 1)
    if comp not in DEFLATE:
        raise ValueError("tiff: compression %d is not deflate (8, 32946)" % comp)
    if width < 1 or height < 1:
        raise ValueError("tiff: an empty image")
    if spp < 1 or spp > 16:
        raise ValueError("tiff: %d samples per pixel (1 .. 16)" % spp)
    if planar != 1 and spp > 1:
        raise ValueError("tiff: PlanarConfiguration 2 with %d samples per pixel" % spp)
    bits = tuple(int(b) for b in tags.get(BITS, (1,)))
    if len(set(bits)) != 1 or bits[0] not in (8, 16, 32, 64):
        raise ValueError("tiff: bits per sample %r (8, 16, 32 or 64, all equal)" % (bits,))
    bps = bits[0] // 8
    if pred not in (1, 2, 3) or (pred == 3 and bps == 1):
        raise ValueError("tiff: predictor %d on %d-bit samples" % (pred, bits[0]))
    fmt = tuple(int(f) for f in tags.get(SAMPLE_FORMAT, (1,)))
    tiled = TILE_WIDTH in tags
    if tiled:
        sw, sr = one(TILE_WIDTH), one(TILE_LENGTH)
        offsets, counts = tags.get(TILE_OFFSETS), tags.get(TILE_COUNTS)
    else:
        sw, sr = width, min(one(ROWS_PER_STRIP, height), height)
        offsets, counts = tags.get(STRIP_OFFSETS), tags.get(STRIP_COUNTS)
    if sw < 1 or sr < 1 or offsets is None or counts is None:
        raise ValueError("tiff: no strips or tiles")
    across, down = (width + sw - 1) // sw, (height + sr - 1) // sr
    if len(offsets) != across * down or len(counts) != across * down:
        raise ValueError("tiff: %d offsets and %d counts for %d segments" %
                         (len(offsets), len(counts), across * down))
    return Image(width=width, height=height, spp=spp, bps=bps, sample_format=fmt[0],
                 predictor=pred, compression=comp, tiled=tiled, seg_width=sw, seg_rows=sr,
                 across=across, down=down, offsets=[int(o) for o in offsets],
                 counts=[int(c) for c in counts])


def parse(buf):
    """a little-endian classic TIFF or BigTIFF (bytes-like, on the host) -> a
    list of Image, one per IFD.  ValueError for what is not covered."""
    buf = bytes(buf) if not isinstance(buf, (bytes, bytearray)) else buf
    if len(buf) < 8:
        raise ValueError("tiff: too short")
    if buf[:2] == b"MM":
        raise ValueError("tiff: big-endian (MM) files are not covered")
    if buf[:2] != b"II":
        raise ValueError("tiff: no TIFF header")
    magic = struct.unpack_from("<H", buf, 2)[0]
    if magic == 42:
        big, at = False, struct.unpack_from("<I", buf, 4)[0]
    elif magic == 43 and len(buf) >= 16 and struct.unpack_from("<HH", buf, 4) == (8, 0):
        big, at = True, struct.unpack_from("<Q", buf, 8)[0]
    else:
        raise ValueError("tiff: no TIFF header")
    images, seen = [], set()
    while at:
        if at in seen:
            raise ValueError("tiff: the IFDs form a loop")
        seen.add(at)
        tags, at = _ifd(buf, at, big)
        im = _image(tags)
        for o, c in zip(im.offsets, im.counts):
            if o + c > len(buf):
                raise ValueError("tiff: a segment outside the file")
        images.append(im)
    return images


def build(width, height, spp, bps, sample_format, predictor, streams, rows_per_strip=None,
          tile=None):
    """a classic little-endian TIFF of one image from finished zlib streams,
    one per strip (rows_per_strip; None: one strip) or per tile (tile = (width,
    length)), in TIFF's order: rows of tiles, left to right.  -> bytes"""
    if tile is not None:
        tw, tl = tile
        n = ((width + tw - 1) // tw) * ((height + tl - 1) // tl)
    else:
        rps = height if rows_per_strip is None else min(int(rows_per_strip), height)
        n = (height + rps - 1) // rps
    if len(streams) != n:
        raise ValueError("tiff.build: %d streams for %d segments" % (len(streams), n))
    body, offsets = bytearray(b"II*\0\0\0\0\0"), []
    for s in streams:
        offsets.append(len(body))
        body += bytes(s)
        body += b"\0" * (len(body) & 1)
    extra = spp - (3 if spp >= 3 else 1)
    entries = [(WIDTH, 4, [width]), (HEIGHT, 4, [height]), (BITS, 3, [8 * bps] * spp),
               (COMPRESSION, 3, [8]), (PHOTOMETRIC, 3, [2 if spp >= 3 else 1]),
               (SPP, 3, [spp]), (PLANAR, 3, [1]), (PREDICTOR, 3, [predictor]),
               (SAMPLE_FORMAT, 3, [sample_format] * spp)]
    if extra > 0:
        entries.append((EXTRA_SAMPLES, 3, [2] + [0] * (extra - 1)))
    if tile is not None:
        entries += [(TILE_WIDTH, 4, [tw]), (TILE_LENGTH, 4, [tl]), (TILE_OFFSETS, 4, offsets),
                    (TILE_COUNTS, 4, [len(s) for s in streams])]
    else:
        entries += [(STRIP_OFFSETS, 4, offsets), (ROWS_PER_STRIP, 4, [rps]),
                    (STRIP_COUNTS, 4, [len(s) for s in streams])]
    entries.sort()
    # values that do not fit an entry's four bytes stand in front of the IFD
    fields = []
    for tag, typ, vals in entries:
        data = struct.pack("<%d%s" % (len(vals), "H" if typ == 3 else "I"), *vals)
        if len(data) > 4:
            where = len(body)
            body += data
            body += b"\0" * (len(body) & 1)
            data = struct.pack("<I", where)
        fields.append(struct.pack("<HHI", tag, typ, len(vals)) + data.ljust(4, b"\0"))
    struct.pack_into("<I", body, 4, len(body))
    body += struct.pack("<H", len(fields)) + b"".join(fields) + struct.pack("<I", 0)
    return bytes(body)
