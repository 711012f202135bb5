"""The CPU model of the Adam7 calls (tools/models/png_adam7.py) and the builder
of interlaced files (tests/png_adam7_files.py), pinned against each other, the
builder's own pixels and PIL: weaving and taking apart are inverses for every
depth and colour pair and every width and height in 1 .. 17, the model decodes
what the builder built - in PNG's layout and to a pixel format -, PIL reads the
same pixels out of the same files, and without the flag the index is
png_model's.  No GPU."""
import io

import numpy as np
import pytest

from tests import png_adam7_files as p7
from tests import png_files as pf
from tools.models import png_adam7 as m7
from tools.models import png_model as pm
from tools.models import png_pixels_model as px

SIZES = [(1, 1), (2, 1), (1, 2), (3, 3), (4, 5), (5, 4), (8, 8), (9, 9), (17, 31), (31, 17)]


def test_pass_geometry_is_the_grid_walked():
    for w in range(1, 18):
        for h in range(1, 18):
            sizes = m7.pass_sizes(w, h)
            grid = np.zeros((h, w), dtype=np.int32)
            for p, (x0, y0, dx, dy) in enumerate(p7.PASSES):
                part = grid[y0::dy, x0::dx]
                part += 1
                want = part.shape if part.size else (0, 0)
                assert (sizes[p][1], sizes[p][0]) == want
            assert (grid == 1).all()        # every pixel in exactly one pass
    assert m7.PASSES == p7.PASSES
    assert m7.raw7(9, 10, 8, 2) == 290 and m7.raw7(1, 1, 1, 0) == 2
    assert m7.raw7(2, 1300000000, 8, 0) >= 1 << 32 > 3 * 1300000000


def test_deinterlace_inverts_interlace():
    for depth, colour in pm.COMBOS:
        for w in range(1, 18):
            for h in range(1, 18):
                pixels = pf.pixels_random(w, h, depth, colour, w * 31 + h)
                passes = m7.interlace(pixels, w, h, depth, colour)
                geo = m7.pass_geometry(w, h, depth, colour)
                assert [len(p) for p in passes] == [hp * rb for _, hp, rb in geo]
                assert m7.deinterlace(passes, w, h, depth, colour) == pixels
    # the model's passes are the builder's
    pixels = pf.pixels_random(13, 11, 2, 3, 5)
    built = {p: data for p, _, _, data in p7.pass_images(pixels, 13, 11, 2, 3)}
    assert [built.get(p, b"") for p in range(7)] == m7.interlace(pixels, 13, 11, 2, 3)


def _files():
    for depth, colour in pm.COMBOS:
        for k, (w, h) in enumerate(SIZES):
            yield p7.make7(w, h, depth, colour, seed=depth + colour + k,
                           filters="random:%d" % (k + depth), idat=None if k % 2 else 7)


def test_model_decodes_what_the_builder_built():
    for g in _files():
        assert pm.index(g.data)[0] == pm.UNSUPPORTED
        res, row = m7.index(g.data, flags=m7.ADAM7)
        assert res == m7.SUCCESS and row[3] >> 16 & 0xFF == 1
        twin = pf.make(g.width, g.height, g.depth, g.colour, pixels=g.pixels)
        trow = pm.index(twin.data)[1]
        assert m7.plain_twin(row)[2:4] == trow[2:4]
        assert m7.decode(g.data, row) == (m7.SUCCESS, g.pixels)
        if g.depth == 16:
            assert m7.decode(g.data, row, m7.LE16) == (m7.SUCCESS, pm.swap16(g.pixels))
        for fmt in (px.RGB, px.GRAY_ALPHA | px.OUT16):
            assert m7.decode(g.data, row, m7.LE16, fmt) == px.decode(twin.data, trow, fmt, pm.LE16)
        assert m7.out_sizes([row, row], [1, 0], 0, 16) == pm.out_sizes([trow, trow], [1, 0], 16)
        assert m7.out_sizes([row], [0], px.RGBA, 4) == px.out_sizes([trow], [0], px.RGBA, 4)


def test_pil_reads_the_same_pixels():
    Image = pytest.importorskip("PIL.Image")
    for g in _files():
        twin = pf.make(g.width, g.height, g.depth, g.colour, pixels=g.pixels)
        a = Image.open(io.BytesIO(g.data))
        b = Image.open(io.BytesIO(twin.data))
        assert a.info.get("interlace") == 1 and not b.info.get("interlace")
        a.load()
        b.load()
        assert a.mode == b.mode and a.size == b.size and a.tobytes() == b.tobytes()


def test_index_without_the_flag_is_png_model():
    files = [data for data, _ in pf.defects().values()]
    files += [data for data, _, _ in p7.defects7().values()]
    files += [g.data for g in list(_files())[::7]]
    files += [pf.make(5, 4, d, c, seed=d).data for d, c in pm.COMBOS]
    buf = b"xyz" + b"".join(files)
    at = 3
    for f in files:
        assert m7.index(buf, at, len(f), 0) == pm.index(buf, at, len(f))
        res, row = m7.index(buf, at, len(f), m7.ADAM7)
        old = pm.index(buf, at, len(f))
        if len(f) > 28 and f[28] == 1 and old[0] == pm.UNSUPPORTED:
            assert res in (m7.SUCCESS, m7.UNSUPPORTED)
        else:
            assert (res, row) == old
        at += len(f)
    for name, (data, verdict, decoded) in p7.defects7().items():
        res, row = m7.index(data, flags=m7.ADAM7)
        assert res == verdict, name
        if decoded is not None:
            assert m7.decode(data, row)[0] == decoded, name
            assert m7.decode(data, row, 0, px.RGB)[0] == decoded, name
    # an interlaced file with an unknown critical chunk stays refused
    g = p7.make7(5, 5, before=[(b"ABCD", b"x")])
    assert m7.index(g.data, flags=m7.ADAM7)[0] == m7.UNSUPPORTED
