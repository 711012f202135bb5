"""The CPU model of the PNG reader (tools/models/png_model.py) and the file
builder (tests/png_files.py) pinned against PIL where PIL imports: files PIL
writes, with its own adaptive filters, decode through the model to PIL's
pixels, and files the builder writes decode through PIL to the model's pixels,
for all 15 depth and colour pairs - so the GPU tests may rest on the model
alone where PIL is absent.  And, without PIL, the model against the builder on
every filter type and the model's verdicts on the defect files.  No GPU."""
import io

import numpy as np
import pytest

from tests import png_files as pf
from tools.models import png_model as pm

W, H = 67, 65


def _pil_pixels(im, depth, colour):
    """PIL's pixels as the bytes PNG stores: height * rowbytes, packed, 16-bit
    big-endian"""
    w, h = im.size
    if colour == 3 or (colour == 0 and depth < 8):
        idx = np.asarray(im.convert("L") if im.mode == "1" else im, dtype=np.uint8)
        if im.mode == "1":
            idx = idx // 255
        bits = np.unpackbits(idx.reshape(h, w, 1), axis=2)[:, :, 8 - depth:].reshape(h, -1)
        return np.packbits(bits, axis=1).tobytes()
    a = np.asarray(im)
    if depth == 16:
        return a.astype(">u2").tobytes()
    return a.astype(np.uint8).tobytes()


# what PIL writes itself: mode -> (depth, colour)
PIL_WRITES = {"1": (1, 0), "L": (8, 0), "I;16": (16, 0), "RGB": (8, 2), "P": (8, 3),
              "LA": (8, 4), "RGBA": (8, 6)}


@pytest.mark.parametrize("mode", sorted(PIL_WRITES))
def test_pil_written_files_decode_through_the_model(mode):
    Image = pytest.importorskip("PIL.Image")
    depth, colour = PIL_WRITES[mode]
    rng = np.random.RandomState(len(mode) + depth)
    y, x = np.mgrid[0:H, 0:W]
    if mode == "1":
        im = Image.fromarray(((x + y + rng.randint(0, 2, (H, W))) % 3 == 0))
    elif mode == "I;16":
        im = Image.fromarray((x * 700 + y * 300 + rng.randint(0, 50, (H, W))).astype(np.uint16))
    else:
        ch = pm.channels(colour)
        a = (x[:, :, None] * 3 + y[:, :, None] * 2 + np.arange(ch) * 40 +
             rng.randint(0, 6, (H, W, ch))).astype(np.uint8)
        im = Image.fromarray(a[:, :, 0] if ch == 1 else a, mode="P" if mode == "P" else None)
        if mode == "P":
            im.putpalette(pf.palette(256))
    for opts in ({}, {"optimize": True}, {"compress_level": 1}):
        f = io.BytesIO()
        im.save(f, "PNG", **opts)
        data = f.getvalue()
        res, row, dres, pixels = pm.read(data)
        assert (res, dres) == (0, 0)
        back = Image.open(io.BytesIO(data))
        got = pm.shape(row)
        assert got[:2] == (H, W) and (got[3], got[4]) in ((depth, colour), (8, 3), (1, 3),
                                                         (2, 3), (4, 3))
        assert pixels == _pil_pixels(back, got[3], got[4]), (mode, opts)


@pytest.mark.parametrize("depth,colour", pm.COMBOS)
def test_builder_files_decode_through_pil(depth, colour):
    Image = pytest.importorskip("PIL.Image")
    for filters in ("adaptive", "random:3", 4):
        g = pf.make(W, H, depth, colour, filters=filters, seed=depth * 8 + colour,
                    pixels=pf.pixels_smooth(W, H, depth, colour, 5) if filters == "adaptive"
                    else None, idat=1000)
        res, row, dres, pixels = pm.read(g.data)
        assert (res, dres) == (0, 0) and pixels == g.pixels
        assert pm.shape(row) == (H, W, pm.channels(colour), depth, colour)
        im = Image.open(io.BytesIO(g.data))
        im.load()
        assert im.size == (W, H)
        if colour == 4 and depth == 16 or colour in (2, 6) and depth == 16:
            # PIL reduces these to 8 bits: the high byte of every sample
            # (grey with alpha comes back as RGBA, the grey three times)
            want = np.frombuffer(pixels, dtype=np.uint8)[0::2].reshape(H, W, -1)
            if colour == 4:
                want = want[:, :, [0, 0, 0, 1]]
            assert np.array_equal(np.asarray(im), want)
        else:
            assert _pil_pixels(im, depth, colour) == pixels, (depth, colour, filters)


@pytest.mark.parametrize("depth,colour", pm.COMBOS)
def test_model_undoes_what_the_builder_filters(depth, colour):
    for w, h in ((W, H), (1, 65), (65, 1)):
        for filters in (0, 1, 2, 3, 4, "random:1", "adaptive"):
            g = pf.make(w, h, depth, colour, filters=filters, seed=w + h)
            res, row, dres, pixels = pm.read(g.data)
            assert (res, dres) == (0, 0) and pixels == g.pixels
            if depth == 16:
                assert pm.read(g.data, pm.LE16)[3] == \
                    np.frombuffer(g.pixels, dtype=">u2").astype("<u2").tobytes()


def test_model_verdicts_on_the_defect_files():
    for name, (data, verdict) in pf.defects().items():
        res, row = pm.index(b"xyz" + data + b"tail", 3, len(data))
        assert res == verdict, name
        assert row == [3, len(data), 0, 0, 0, 0, 0, 0], name


def test_model_decode_time_verdicts():
    g = pf.make(9, 70, 8, 2, filters=[1] * 63 + [5] + [2] * 6)
    assert pm.read(g.data)[2] == pm.BAD_DATA
    g = pf.make(9, 70, 8, 2, damage=lambda z: z[:40] + bytes([z[40] ^ 0x10]) + z[41:])
    assert pm.read(g.data)[2] == pm.BAD_DATA
    assert pm.read(pf.make(9, 70, 8, 2, rows_delta=-1).data)[2] == pm.SHORT_OUTPUT
    assert pm.read(pf.make(9, 70, 8, 2, rows_delta=1).data)[2] == pm.INSUFFICIENT_SPACE
    g = pf.make(9, 70, 8, 2, idat=[10, 0, 20])
    res, row, dres, pixels = pm.read(g.data)
    assert dres == 0 and pixels == g.pixels
    for delta in (-1, 1):
        stale = list(row)
        stale[5] += delta
        assert pm.decode(g.data, stale) == (pm.BAD_DATA, None)
    assert pm.decode(g.data, row[:2] + [0] * 6) == (pm.UNSUPPORTED, None)
    assert pm.out_sizes([row, row[:2] + [0] * 6], [0, 1, 0], 64) == [0, 1920, 1920, 3840]
