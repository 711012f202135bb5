"""The CPU model of the PNG reader's decode to one pixel format
(tools/models/png_pixels_model.py) against hand-written vectors for each of its
five steps, and against PIL's convert() where PIL imports and follows the same
rule.  No GPU."""
import io

import numpy as np
import pytest

from tests import png_files as pf
from tools.models import png_model as pm
from tools.models import png_pixels_model as px

V16 = [0, 127, 128, 129, 255, 256, 257, 383, 384, 385, 65407, 65408, 65535]
W16 = [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 255, 255, 255]     # round(v / 257)


def _be16(values):
    return np.array(values, dtype=">u2").tobytes()


def test_formats():
    assert px.FORMATS == [1, 2, 3, 4, 0x11, 0x12, 0x13, 0x14]
    assert all(px.format_ok(f) for f in px.FORMATS)
    assert not any(px.format_ok(f) for f in (0, 5, 0x20, 0x13 | 0x40, 0x10, 0x15))
    assert (px.GRAY, px.GRAY_ALPHA, px.RGB, px.RGBA, px.OUT16, px.LE16) == (1, 2, 3, 4, 16, 1)
    direct = {(d, c, f) for d, c in pm.COMBOS for f in px.FORMATS if px.is_direct(d, c, f)}
    assert direct == {(8, 0, 1), (8, 4, 2), (8, 2, 3), (8, 6, 4),
                      (16, 0, 0x11), (16, 4, 0x12), (16, 2, 0x13), (16, 6, 0x14)}


def test_samples_are_unpacked_most_significant_bit_first():
    # two rows of 5 pixels at 2 bits: 10 bits of two bytes, 6 spare bits set
    s = px.samples(bytes([0b00011011, 0b11111111, 0b11100100, 0b00111111]), 5, 2, 2, 0)
    assert s[:, :, 0].tolist() == [[0, 1, 2, 3, 3], [3, 2, 1, 0, 0]]
    s = px.samples(bytes([0b10100000]), 3, 1, 1, 0)
    assert s[:, :, 0].tolist() == [[1, 0, 1]]
    s = px.samples(bytes([0x12, 0x3F]), 3, 1, 4, 3)
    assert s[:, :, 0].tolist() == [[1, 2, 3]]
    s = px.samples(_be16([0x0102, 0xFFFE, 3, 4, 5, 6]), 1, 2, 16, 2)
    assert s.tolist() == [[[0x0102, 0xFFFE, 3]], [[4, 5, 6]]]


def test_sixteen_to_eight_rounds_to_nearest():
    got = px.scale(np.array(V16), 16, 8).tolist()
    assert got == W16
    # as one image, to GRAY and RGB
    res, out = px.convert(_be16(V16), 13, 1, 16, 0, px.GRAY)
    assert res == 0 and list(out) == W16
    res, out = px.convert(_be16(V16), 13, 1, 16, 0, px.RGB)
    assert list(out) == [v for v in W16 for _ in range(3)]
    # every value against the rational it rounds: v / 257, halves upwards
    v = np.arange(65536)
    assert np.array_equal(px.scale(v, 16, 8), (2 * v + 257) // 514)


def test_bit_replication_of_every_small_value():
    assert px.scale(np.arange(2), 1, 8).tolist() == [0, 255]
    assert px.scale(np.arange(4), 2, 8).tolist() == [0, 85, 170, 255]
    assert px.scale(np.arange(16), 4, 8).tolist() == [17 * i for i in range(16)]
    assert px.scale(np.arange(2), 1, 16).tolist() == [0, 65535]
    assert px.scale(np.arange(4), 2, 16).tolist() == [0, 0x5555, 0xAAAA, 0xFFFF]
    assert px.scale(np.arange(16), 4, 16).tolist() == [0x1111 * i for i in range(16)]
    assert px.scale(np.arange(256), 8, 16).tolist() == [257 * i for i in range(256)]
    assert px.scale(np.arange(256), 8, 8).tolist() == list(range(256))


def test_grey_formula():
    def grey(r, g, b):
        return int(px.gray_of(np.array([r]), np.array([g]), np.array([b]))[0])
    assert grey(255, 255, 255) == 255
    assert grey(255, 0, 0) == (19595 * 255 + 32768) >> 16 == 76
    assert grey(0, 255, 0) == (38470 * 255 + 32768) >> 16 == 150
    assert grey(0, 0, 255) == (7471 * 255 + 32768) >> 16 == 29
    assert grey(65535, 65535, 65535) == 65535       # fits in 32 bits
    assert all(grey(v, v, v) == v for v in (0, 1, 127, 128, 254, 65534))
    res, out = px.convert(bytes([255, 0, 0, 0, 255, 0, 0, 0, 255, 9, 9, 9]), 4, 1, 8, 2, px.GRAY)
    assert list(out) == [76, 150, 29, 9]
    res, out = px.convert(bytes([255, 0, 0, 0, 255, 0]), 2, 1, 8, 2, px.GRAY_ALPHA | px.OUT16)
    assert out == _be16([grey(65535, 0, 0), 65535, grey(0, 65535, 0), 65535])


def test_palette_and_its_alphas():
    plte = bytes([10, 20, 30, 40, 50, 60, 70, 80, 90])
    idx = bytes([0b00011000])       # 2 bits: 0, 1, 2, (0)
    res, out = px.convert(idx, 3, 1, 2, 3, px.RGBA, plte, bytes([1, 2]))
    assert res == 0 and list(out) == [10, 20, 30, 1, 40, 50, 60, 2, 70, 80, 90, 255]
    res, out = px.convert(idx, 3, 1, 2, 3, px.RGB, plte, None)
    assert list(out) == list(plte)
    # a tRNS longer than the palette: its first `entries` bytes
    res, out = px.convert(idx, 3, 1, 2, 3, px.GRAY_ALPHA, plte, bytes([5, 6, 7, 8]))
    assert list(out)[1::2] == [5, 6, 7]
    res, out = px.convert(idx, 3, 1, 2, 3, px.RGBA | px.OUT16, plte, bytes([1]), px.LE16)
    assert np.frombuffer(out, "<u2").tolist() == [2570, 5140, 7710, 257, 40 * 257, 50 * 257,
                                                  60 * 257, 65535, 70 * 257, 80 * 257, 90 * 257,
                                                  65535]
    # index 3 of 3 entries
    assert px.convert(bytes([0b11000000]), 1, 1, 2, 3, px.RGB, plte, None) == (px.BAD_DATA, None)
    # the spare bits of a row are no index
    res, out = px.convert(bytes([0b00111111]), 1, 1, 2, 3, px.RGB, plte, None)
    assert res == 0 and list(out) == [10, 20, 30]


def test_colour_key_match_and_near_miss():
    # grey, 4 bits: the key's low 4 bits count
    res, out = px.convert(bytes([0x56, 0x40]), 3, 1, 4, 0, px.GRAY_ALPHA, None, bytes([0xFF, 0xF5]))
    assert list(out) == [0x55, 0, 0x66, 255, 0x44, 255]
    # grey 16: equal, the lowest bit differs
    res, out = px.convert(_be16([0x1234, 0x1235]), 2, 1, 16, 0, px.GRAY_ALPHA | px.OUT16, None,
                          _be16([0x1234]))
    assert out == _be16([0x1234, 0, 0x1235, 65535])
    # compared before the scaling: 0x1234 and 0x1235 are both 0x12 at 8 bits
    res, out = px.convert(_be16([0x1234, 0x1235]), 2, 1, 16, 0, px.GRAY_ALPHA, None, _be16([0x1234]))
    assert list(out) == [0x12, 0, 0x12, 255]
    # RGB 8: the key words' low bytes; one channel differs
    key = bytes([0xAB, 1, 0xCD, 2, 0xEF, 3])
    res, out = px.convert(bytes([1, 2, 3, 1, 2, 4, 0, 2, 3]), 3, 1, 8, 2, px.RGBA, None, key)
    assert list(out) == [1, 2, 3, 0, 1, 2, 4, 255, 0, 2, 3, 255]
    # a tRNS of another length, or none: opaque
    for trns in (None, b"", bytes([0]), bytes([0, 1, 0]), bytes(7)):
        res, out = px.convert(bytes([1, 2, 3]), 1, 1, 8, 2, px.RGBA, None, trns)
        assert list(out) == [1, 2, 3, 255]
        res, out = px.convert(bytes([0]), 1, 1, 8, 0, px.GRAY_ALPHA, None,
                              None if trns is None else trns[:1] + trns[3:])
        assert list(out) == [0, 255]
    # colour types 4 and 6 keep their own alpha
    res, out = px.convert(bytes([7, 9]), 1, 1, 8, 4, px.RGBA, None, bytes([0, 7]))
    assert list(out) == [7, 7, 7, 9]
    res, out = px.convert(bytes([1, 2, 3, 4]), 1, 1, 8, 6, px.GRAY_ALPHA, None, bytes(6))
    assert list(out)[1] == 4
    # dropped where the format has none
    res, out = px.convert(bytes([7, 9]), 1, 1, 8, 4, px.RGB)
    assert list(out) == [7, 7, 7]


def test_decode_reads_the_chunks_the_row_names():
    g = pf.make(9, 4, 4, 3, seed=2, plte=pf.palette(16), trns=bytes(range(5)))
    buf = b"xyz" + g.data
    res, row = pm.index(buf, 3, len(g.data))
    assert res == 0
    plte, trns = px.chunks_of(buf, row)
    assert plte == pf.palette(16) and trns == bytes(range(5))
    res, out = px.decode(buf, row, px.RGBA)
    want = px.convert(g.pixels, 9, 4, 4, 3, px.RGBA, plte, trns)
    assert res == 0 and (res, out) == want and len(out) == 9 * 4 * 4
    assert px.out_sizes([row], [0, 0], px.RGBA, 64) == [0, 192, 384]
    assert px.shapes([row], px.RGB | px.OUT16) == ([(4, 9, 3)], "uint16")
    zero = [row[0], row[1], 0, 0, 0, 0, 0, 0]
    assert px.decode(buf, zero, px.RGB) == (px.UNSUPPORTED, None)
    assert px.out_sizes([row, zero], [1, 0, 1], px.GRAY) == [0, 0, 36, 36]


def test_against_pil_convert():
    """where PIL follows the same rule, 8 bits only: palette (+ tRNS) -> RGB /
    RGBA, grey -> RGB, RGBA -> RGB"""
    Image = pytest.importorskip("PIL.Image")
    cases = [pf.make(33, 7, 8, 3, seed=1), pf.make(33, 7, 4, 3, seed=2),
             pf.make(9, 5, 2, 3, seed=3), pf.make(17, 3, 1, 3, seed=4),
             pf.make(33, 7, 8, 3, seed=5, trns=bytes(range(0, 200, 2))),
             pf.make(9, 5, 4, 3, seed=6, trns=bytes([0, 128, 255])),
             pf.make(33, 7, 8, 0, seed=7), pf.make(33, 7, 8, 6, seed=8)]
    modes = [("RGB", px.RGB), ("RGBA", px.RGBA)]
    for g in cases:
        res, row = pm.index(g.data)
        assert res == 0
        for mode, fmt in modes:
            if g.colour != 3 and mode == "RGBA":
                continue
            im = Image.open(io.BytesIO(g.data))
            want = np.asarray(im.convert(mode))
            res, out = px.decode(g.data, row, fmt)
            got = np.frombuffer(out, dtype=np.uint8).reshape(want.shape)
            assert res == 0 and np.array_equal(got, want), (g.depth, g.colour, mode)
