"""The PNG writer's CPU model (tools/models/png_write.py) against what the
repository already trusts: its scanlines against the row-by-row filters of
tests/png_files.py for all 15 depth and colour pairs, the five types and the
adaptive choice; the files it assembles around zlib.compress streams read back
by the reader's model (rows and pixels) and by PIL."""
import io
import zlib

import numpy as np
import pytest

from tests import png_files as pf
from tools.models import png_model as pm
from tools.models import png_write as pw

SHAPES = [(1, 1), (2, 3), (5, 2), (17, 3), (67, 9)]


def _builders(w, h, d, c, seed):
    return (pf.pixels_random(w, h, d, c, seed), pf.pixels_smooth(w, h, d, c, seed),
            pf.pixels_constant(w, h, d, c))


@pytest.mark.parametrize("depth,colour", pm.COMBOS)
def test_scanlines_are_png_files(depth, colour):
    for w, h in SHAPES:
        rb, unit = pm.rowbytes(w, depth, colour), pm.bpp(depth, colour)
        for pixels in _builders(w, h, depth, colour, w * 31 + h):
            for filt in range(5):
                raw, types = pw.scanlines(pixels, h, rb, unit, filt)
                assert raw == pf.scanlines(pixels, h, rb, unit, filt)
                assert types == [filt] * h
            raw, types = pw.scanlines(pixels, h, rb, unit, pw.ADAPTIVE)
            assert raw == pf.scanlines(pixels, h, rb, unit, "adaptive")
            assert types == [raw[y * (rb + 1)] for y in range(h)]


def test_the_ties_the_issue_names():
    # 1 x 1 RGB16: the row is shorter than the unit, Sub ties with None
    raw, types = pw.scanlines(bytes([9, 8, 7, 6, 5, 4]), 1, 6, 6, pw.ADAPTIVE)
    assert types == [0]
    # constant rows below the first: Up ties with Paeth (and Average loses)
    px = pf.pixels_constant(8, 4, 8, 0)
    raw, types = pw.scanlines(px, 4, 8, 1, pw.ADAPTIVE)
    assert types[1:] == [2, 2, 2]
    # a smooth image uses mixed types
    px = pf.pixels_smooth(64, 64, 8, 2, 3)
    raw, types = pw.scanlines(px, 64, 192, 3, pw.ADAPTIVE)
    assert len(set(types)) >= 3


def _batch():
    """a buffer of pixels, palettes and tRNS data and its rows: every pair,
    with PLTE and tRNS where they may stand"""
    buf, rows = bytearray(b"xyz"), []
    for i, (d, c) in enumerate(pm.COMBOS):
        w, h = 5 + 3 * i, 2 + i % 4
        px = pf.pixels_smooth(w, h, d, c, i)
        row = [len(buf), len(px), w | h << 32, d | c << 8 | 0xAB << 24, 77, 88, 0, 0]
        buf += px
        if c == 3:
            entries = min(1 << d, 7)
            row[6] = len(buf) | entries << 48
            buf += pf.palette(entries)
            row[7] = len(buf) | entries - 1 << 48 if entries > 1 else 0
            buf += bytes(range(entries))
        elif c == 2 and d == 8:
            row[6] = len(buf) | 256 << 48   # a suggested palette
            buf += pf.palette(256)
            row[7] = len(buf) | 6 << 48
            buf += bytes(6)
        elif c == 0 and d == 16:
            row[7] = len(buf) | 2 << 48
            buf += b"\x01\x02"
        rows.append(row)
    return bytes(buf), rows


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4, pw.ADAPTIVE])
def test_files_read_back(filt):
    buf, rows = _batch()
    assert all(pw.refusal(r, len(buf)) is None for r in rows)
    streams = [zlib.compress(pw.image_scanlines(r, buf, filt)[0], 6) for r in rows]
    files, result, index = pw.encode(rows, buf, streams)
    out = b"".join(files)
    assert result == [0, len(out), sum(r[1] for r in rows), len(rows)]
    assert len(out) <= pw.bound(rows)
    for row, f, ix in zip(rows, files, index):
        assert out[ix[0]:ix[0] + ix[1]] == f
        # the reader's model finds the row the writer's model states
        assert pm.index(out, ix[0], ix[1]) == (0, ix)
        res, pixels = pm.decode(out, ix)
        assert res == 0 and pixels == buf[row[0]:row[0] + row[1]]
        e, t = row[6] >> 48, row[7] >> 48
        if e:
            assert out[ix[6] & pw.MASK48:][:3 * e] == buf[row[6] & pw.MASK48:][:3 * e]
        if t:
            assert out[ix[7] & pw.MASK48:][:t] == buf[row[7] & pw.MASK48:][:t]
    # one byte short: nothing but the result
    assert pw.encode(rows, buf, streams, len(out) - 1) == (None, [3] + result[1:], None)
    assert pw.encode(rows, buf, streams, len(out))[1][0] == 0


def test_le16_swaps_on_load():
    px = pf.pixels_random(7, 3, 16, 2, 5)
    row = [0, len(px), 7 | 3 << 32, 16 | 2 << 8, 0, 0, 0, 0]
    assert pw.image_scanlines(row, pm.swap16(px), 4, pw.LE16) == pw.image_scanlines(row, px, 4)
    row8 = [0, 63, 7 | 3 << 32, 8 | 2 << 8, 0, 0, 0, 0]
    assert pw.image_pixels(row8, px, pw.LE16) == px[:63]


def test_pil_reads_the_files():
    Image = pytest.importorskip("PIL.Image")
    buf, rows = _batch()
    streams = [zlib.compress(pw.image_scanlines(r, buf)[0], 6) for r in rows]
    files, _, _ = pw.encode(rows, buf, streams)
    modes = {(8, 0): "L", (8, 2): "RGB", (8, 6): "RGBA", (8, 4): "LA", (8, 3): "P"}
    for row, f in zip(rows, files):
        w, h, d, c, rb, unit = pw.geometry(row)
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.size == (w, h)
        if (d, c) in modes:
            assert im.mode == modes[d, c]
            assert im.tobytes() == buf[row[0]:row[0] + row[1]]
        elif d < 8 and c == 3:
            idx = np.frombuffer(im.tobytes(), dtype=np.uint8).reshape(h, w)
            packed = np.frombuffer(buf[row[0]:row[0] + row[1]], dtype=np.uint8).reshape(h, rb)
            bits = np.unpackbits(packed, axis=1)[:, :w * d].reshape(h, w, d)
            assert (idx == (bits * (1 << np.arange(d - 1, -1, -1))).sum(axis=2)).all()
        if row[6] and c == 3:
            e = row[6] >> 48
            assert bytes(im.getpalette()[:3 * e]) == buf[row[6] & pw.MASK48:][:3 * e]


def test_refusals_and_bound():
    ok = [0, 45, 5 | 3 << 32, 8 | 2 << 8, 0, 0, 0, 0]
    assert pw.refusal(ok, 45) is None and pw.refusal(ok, 44) == "pixels"
    assert pw.bound([ok]) == 8 + 25 + 12 + pw.zlib_bound(3 * 16) + 12
    for col, value, word in ((1, 44, "word 1"), (2, 5, "width"), (2, 3 << 32, "width"),
                             (3, 4 | 2 << 8, "bit depth"), (3, 8 | 2 << 8 | 1 << 16, "interlaced"),
                             (7, 10 | 2 << 48, "tRNS"), (6, 10 | 257 << 48, "PLTE")):
        bad = list(ok)
        bad[col] = value
        assert pw.refusal(bad, 1 << 20) == word and pw.bound([ok, bad]) == 0
    grey = [0, 15, 5 | 3 << 32, 8, 0, 0, 1 | 1 << 48, 0]
    assert pw.refusal(grey, 100) == "PLTE"
    pal = [0, 15, 5 | 3 << 32, 8 | 3 << 8, 0, 0, 0, 0]
    assert pw.refusal(pal, 100) == "PLTE"
    pal[6] = 20 | 2 << 48
    assert pw.refusal(pal, 100) is None
    pal[7] = 30 | 3 << 48
    assert pw.refusal(pal, 100) == "tRNS"
    big = [0, 65536 * 65536 * 4, 65536 | 65536 << 32, 8 | 6 << 8, 0, 0, 0, 0]
    assert pw.refusal(big) == "2^32"
    idat = [0, 46341 * 46340, 46340 | 46341 << 32, 8, 0, 0, 0, 0]
    assert pw.refusal(idat) == "zlib bound"
