"""The CPU side of the OpenEXR calls: the model of the ZIP / ZIPS chunk coding
(tools/models/exr_model.py) against the format's worked example and against
itself, the host parser and builder (libdeflate_amd/exr.py) round trip for
scanline ZIP, ZIPS, NONE and tiled files, every refusal of parse() with its
reason, and the fixture files of tests/golden/exr (written by
tools/gen_exr_fixtures.py with exr.assemble() and Python's zlib: they pin the
parser and the model against regressions, not the format against the OpenEXR
library).  No GPU."""
import struct
import zlib

import numpy as np
import pytest

from libdeflate_amd import binding, exr
from tests import exr_chunks as ec
from tools.models import exr_model as em

RGBA = [("A", exr.HALF), ("B", exr.HALF), ("G", exr.HALF), ("R", exr.HALF)]
RGBAZ = RGBA + [("Z", exr.FLOAT)]


def test_the_worked_example_byte_for_byte():
    raw = bytes.fromhex("103c123c153c193c1e")
    coded = bytes.fromhex("10828384859e808080")
    assert em.apply(raw) == coded
    assert em.undo(coded) == raw


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 2047, 2048, 2049, 4097, 10001])
def test_undo_inverts_apply(n):
    for seed in range(3):
        x = ec.random_bytes([n, seed], n)
        assert len(em.apply(x)) == n
        assert em.undo(em.apply(x)) == x
        assert em.apply(em.undo(x)) == x


def test_apply_is_the_formula():
    raw = ec.random_bytes(5, 77)
    n, h = 77, 39
    t = [raw[2 * k] for k in range(h)] + [raw[2 * k + 1] for k in range(n - h)]
    p = [t[0]] + [(t[i] - t[i - 1] + 128) % 256 for i in range(1, n)]
    assert em.apply(raw) == bytes(p)


def test_the_store_decision():
    rnd = ec.random_bytes(1, 4096)
    assert len(zlib.compress(em.apply(rnd), 6)) >= 4096 and em.data_of(rnd) == rnd
    flat = b"\x07" * 4096
    assert len(em.data_of(flat)) < 4096 and em.undo(zlib.decompress(em.data_of(flat))) == flat
    tiny = ec.random_bytes(2, 16)
    assert em.data_of(tiny) == tiny         # 16 random bytes: the stream is longer


def test_rows_and_classes():
    r = em.row(100, 50, 7, 64, (8, 2), [False, True], em.PIXELS, [1, 0], head=(-3,))
    assert r == [100, 50, 7, 64, 8 | 2 << 32, 2 | 2 << 8 | 1 << 32, 1, 8, 0xFFFFFFFD, 0]
    assert em.raw_size(r) == 8 * 2 * 6 and em.classify(r) == em.ZLIB
    assert em.classify(em.row(0, 96, 0, 64, (8, 2), [False, True], em.PIXELS, [1, 0])) == em.RAW_LAYOUT
    assert em.classify(em.row(0, 96, 0, 48, (8, 2), [False, True])) == em.RAW_DIRECT
    assert em.classify(em.row(0, 96, 0, 49, (8, 2), [False, True])) == em.RAW_LAYOUT
    assert em.classify(em.row(0, 48, 0, 49, (8, 1), [False, True])) == em.RAW_DIRECT
    assert em.classify(em.row(0, 97, 0, 48, (8, 2), [False, True])) == em.BAD
    tile = em.row(0, 0, 0, 0, (1, 1), [False], head=(1, 2, 0, 0))
    assert tile[7:] == [20, 1 | 2 << 32, 0]
    from libdeflate_amd import api
    got = api.exr_rows([7], 64, (8, 2), [False, True], binding.EXR_PIXELS, [1, 0], [100], [50], [(-3,)])
    assert got.tolist() == [r]


def test_expected_and_gather_are_inverses():
    for wide, slots in [([False] * 4, [3, 2, 1, 0]), ([False, True, False], [1, 2, 0]), ([True], [0])]:
        r = em.row(0, 0, 0, 0, (5, 3), wide, em.PIXELS, slots)
        raw = ec.random_bytes(9, em.raw_size(r))
        lines = em.expected(r, raw)
        assert em.gather(r, lines) == raw
    # A, B, G, R in the file -> R, G, B, A in the pixel
    r = em.row(0, 0, 0, 0, (2, 1), [False] * 4, em.PIXELS, [3, 2, 1, 0])
    raw = bytes.fromhex("a0a0a1a1" "b0b0b1b1" "c0c0c1c1" "d0d0d1d1")
    assert em.expected(r, raw) == [bytes.fromhex("d0d0c0c0b0b0a0a0" "d1d1c1c1b1b1a1a1")]


@pytest.mark.parametrize("compression,tile,channels", [
    (exr.ZIP, None, RGBA), (exr.ZIPS, None, RGBAZ), (exr.NONE, None, RGBA),
    (exr.ZIP, (32, 32), RGBA), (exr.ZIP, (16, 8), [("Y", exr.FLOAT)])])
def test_build_and_parse_round_trip(compression, tile, channels):
    width, height = 70, 37
    data, planes = ec.image_file(width, height, channels, compression, tile, seed=3)
    im = exr.parse(data)
    assert (im.width, im.height, im.channels, im.compression, im.tile) == \
        (width, height, channels, compression, tile)
    per = exr.LINES_PER_CHUNK[compression]
    n = -(-width // tile[0]) * -(-height // tile[1]) if tile else -(-height // per)
    assert len(im.chunks) == n
    # every chunk decodes, on the host, to its region of the image
    rows = im.rows(layout=binding.EXR_PIXELS, order=None)
    assert rows.shape == (n, binding.EXR_WORDS)
    px = im.pixel_bytes
    want = ec.interleaved(planes)
    got = np.zeros((height, width * px), dtype=np.uint8)
    flat = got.reshape(-1)
    kinds = set()
    for r, t in zip(rows.tolist(), im.chunks.tolist()):
        assert r[0] == t[exr.T_DATA_OFF] and r[1] == t[exr.T_DATA_N]
        assert r[7] == (20 if tile else 8) and r[0] - r[7] == t[exr.T_HEAD_OFF]
        stored = data[r[0]:r[0] + r[1]]
        assert em.head_bytes(r, r[1]) == data[r[0] - r[7]:r[0]]
        kinds.add(em.classify(r))
        raw = stored if r[1] == em.raw_size(r) else em.undo(zlib.decompress(stored))
        for y, line in enumerate(em.expected(r, raw)):
            flat[r[2] + y * r[3]:r[2] + y * r[3] + len(line)] = np.frombuffer(line, dtype=np.uint8)
    assert got.tobytes() == want.tobytes()
    assert kinds == ({em.RAW_LAYOUT} if compression == exr.NONE else {em.ZLIB})


def test_rows_orders_and_layouts():
    data, _ = ec.image_file(9, 5, RGBA, exr.ZIPS, seed=1)
    im = exr.parse(data)
    assert im.slots("RGBA") == [3, 2, 1, 0] and im.slots(None) == [0, 1, 2, 3]
    assert im.slots(["A", "R", "G", "B"]) == [0, 3, 2, 1]
    assert [int(r[6]) for r in im.rows(layout=binding.EXR_PIXELS, order="RGBA")] == [0x0123] * 5
    lines = im.rows(offset=11)
    assert [int(r[6]) for r in lines] == [0] * 5 and [int(r[5]) >> 32 for r in lines] == [0] * 5
    assert [int(r[2]) for r in lines] == [11 + 72 * y for y in range(5)]
    with pytest.raises(ValueError, match="order"):
        im.slots("RGB")
    with pytest.raises(ValueError, match="PIXELS"):
        im.rows(order="RGBA")


def _patched(data, name, value):
    """the file with attribute `name`'s value replaced (same length)"""
    at = data.index(name.encode() + b"\0")
    at = data.index(b"\0", at + len(name) + 1) + 1 + 4
    return data[:at] + value + data[at + len(value):]


def test_parse_refusals():
    data, _ = ec.image_file(20, 20, RGBA, exr.ZIP, seed=2)
    tiled, _ = ec.image_file(20, 20, RGBA, exr.ZIP, (8, 8), seed=2)
    exr.parse(data), exr.parse(tiled)
    with pytest.raises(ValueError, match="magic"):
        exr.parse(b"\x00" + data[1:])
    for comp, name in [(1, "RLE"), (4, "PIZ"), (5, "PXR24"), (6, "B44"), (7, "B44A"), (8, "DWAA"),
                       (9, "DWAB")]:
        with pytest.raises(ValueError, match="compression %s is not covered" % name):
            exr.parse(_patched(data, "compression", bytes([comp])))
    with pytest.raises(ValueError, match="deep"):
        exr.parse(data[:4] + struct.pack("<i", 2 | exr.DEEP) + data[8:])
    with pytest.raises(ValueError, match="multi-part"):
        exr.parse(data[:4] + struct.pack("<i", 2 | exr.MULTIPART) + data[8:])
    for mode, name in [(1, "MIPMAP"), (2, "RIPMAP"), (0x11, "MIPMAP")]:
        with pytest.raises(ValueError, match=name):
            exr.parse(_patched(tiled, "tiles", struct.pack("<IIB", 8, 8, mode)))
    # channel A with xSampling 2
    chl = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", t, 0, 2 if n == "A" else 1, 1)
                   for n, t in RGBA) + b"\0"
    with pytest.raises(ValueError, match="subsampled"):
        exr.parse(_patched(data, "channels", chl))
    im = exr.parse(data)
    table_at = int(im.chunks[0, exr.T_HEAD_OFF]) - 8 * len(im.chunks)
    with pytest.raises(ValueError, match="offset .* outside the file"):
        exr.parse(data[:table_at] + struct.pack("<Q", len(data) - 3) + data[table_at + 8:])
    size_at = int(im.chunks[1, exr.T_HEAD_OFF]) + 4
    with pytest.raises(ValueError, match="size .* outside the file"):
        exr.parse(data[:size_at] + struct.pack("<i", len(data)) + data[size_at + 4:])
    with pytest.raises(ValueError, match="size .* outside the file"):
        exr.parse(data[:-1])
    with pytest.raises(ValueError, match="offset table"):
        exr.parse(data[:table_at + 5])


def test_fixture_files_parse_to_their_pixels():
    files = ec.fixtures()
    assert len(files) >= 6
    seen = set()
    for name, data, pixels in files:
        im = exr.parse(data)
        seen.add((im.compression, im.tile is not None))
        assert pixels.shape == (im.height, im.width, im.pixel_bytes), name
        flat = np.zeros(im.nbytes, dtype=np.uint8)
        for r in im.rows(layout=binding.EXR_PIXELS).tolist():
            stored = data[r[0]:r[0] + r[1]]
            raw = stored if r[1] == em.raw_size(r) else em.undo(zlib.decompress(stored))
            for y, line in enumerate(em.expected(r, raw)):
                flat[r[2] + y * r[3]:r[2] + y * r[3] + len(line)] = np.frombuffer(line, dtype=np.uint8)
        assert flat.tobytes() == pixels.tobytes(), name
    assert seen >= {(exr.ZIP, False), (exr.ZIPS, False), (exr.NONE, False), (exr.ZIP, True)}
