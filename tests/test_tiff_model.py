"""The CPU model of the TIFF predictors (tools/models/tiff_model.py) and the
host-side parser and builder (libdeflate_amd/tiff.py), pinned to libtiff: the
files of tests/golden/tiff were written by Pillow with libtiff, and
tiff.parse() plus Python's zlib plus the model's undo() reproduce their pixels
exactly.  apply() and undo() are inverses on random shapes; where Pillow is
importable, files made by tiff.build() open in it with equal pixels, and
freshly generated files agree with the committed ones.  No GPU."""
import os
import zlib

import numpy as np
import pytest

from libdeflate_amd import tiff
from tests import tiff_segments as ts
from tools import gen_tiff_fixtures as gen
from tools.models import tiff_model as tm


def _decode(data, offset=0, pitch=None):
    """the file's first image through parse(), zlib and the model -> its bytes"""
    (im,) = tiff.parse(data)
    px = im.spp * im.bps
    pitch_ = im.width * px if pitch is None else pitch
    out = bytearray(b"\xA5" * (offset + (im.height - 1) * pitch_ + im.width * px))
    for r in im.rows(offset=offset, pitch=pitch):
        d = tm.unpack(r)
        assert tm.row_why(r, True, len(data), len(out)) is None
        raw = zlib.decompress(data[d["stored_off"]:d["stored_off"] + d["stored_n"]])
        assert len(raw) == d["coded"]
        pix = tm.undo(raw, d["cr"], d["cw"], d["spp"], d["bps"], d["pred"])
        for y, line in enumerate(tm.expected(r, pix)):
            at = d["raw_off"] + y * d["pitch"]
            out[at:at + len(line)] = line
    return im, bytes(out)


def test_fixtures_cover_the_modes():
    names = [n for n, _, _ in ts.fixtures()]
    assert len(names) == len(list(gen.cases())) == 45
    assert sorted(names) == sorted(gen.name(m, p, w, h, r, c) for m, _, _, p, w, h, r, c in gen.cases())
    for f in os.listdir(ts.GOLDEN):
        assert os.path.getsize(os.path.join(ts.GOLDEN, f)) <= 65536, f


@pytest.mark.parametrize("name,data,pixels", ts.fixtures(), ids=[n for n, _, _ in ts.fixtures()])
def test_parse_zlib_and_the_model_reproduce_libtiff(name, data, pixels):
    im, got = _decode(data)
    assert got == pixels
    mode, pred, w, h, rps = name.split("_")[:5]
    assert (im.predictor, im.width, im.height) == (int(pred[1:]), int(w[1:]), int(h[1:]))
    assert not im.tiled and im.seg_rows == min(int(rps[3:]), im.height) and im.across == 1
    assert (im.spp, im.bps, im.sample_format) == {"l": (1, 1, 1), "rgb": (3, 1, 1), "rgba": (4, 1, 1),
                                                  "i16": (1, 2, 1), "f": (1, 4, 3)}[mode]
    assert im.compression in tiff.DEFLATE
    # the last strip is short, and every strip is kept whole
    rows = im.rows()
    assert sum(int(r[5]) >> 32 for r in rows) == im.height
    assert all(r[4] == r[5] for r in rows)
    # at an offset and a pitch of its own: the same pixels, nothing in the gaps
    px = im.spp * im.bps
    _, wide = _decode(data, offset=7, pitch=im.width * px + 5)
    for y in range(im.height):
        a = 7 + y * (im.width * px + 5)
        assert wide[a:a + im.width * px] == pixels[y * im.width * px:(y + 1) * im.width * px]
        assert y + 1 == im.height or wide[a + im.width * px:a + im.width * px + 5] == b"\xA5" * 5


def test_apply_then_undo_is_the_identity():
    rng = np.random.default_rng(317)
    for k in range(300):
        spp, bps = int(rng.integers(1, 17)), int(rng.choice([1, 2, 4, 8]))
        rows, width = int(rng.integers(1, 6)), int(rng.integers(1, 40))
        raw = rng.integers(0, 256, size=rows * width * spp * bps, dtype=np.uint8).tobytes()
        for pred in (1, 2, 3) if bps > 1 else (1, 2):
            coded = tm.apply(raw, rows, width, spp, bps, pred)
            assert len(coded) == len(raw) and (pred != 1 or coded == raw)
            assert tm.undo(coded, rows, width, spp, bps, pred) == raw
            assert tm.apply(tm.undo(raw, rows, width, spp, bps, pred), rows, width, spp, bps, pred) == raw


def test_the_predictors_by_hand():
    # predictor 2, two channels of one byte: differences per channel, modulo 256
    assert tm.apply(bytes([10, 200, 13, 190, 3, 201]), 1, 3, 2, 1, 2) == bytes([10, 200, 3, 246, 246, 11])
    # 16-bit samples: the carry stays inside the sample
    a = np.array([0x00FF, 0x0100, 0x0000], dtype="<u2").tobytes()
    assert tm.apply(a, 1, 3, 1, 2, 2) == np.array([0x00FF, 0x0001, 0xFF00], dtype="<u2").tobytes()
    # predictor 3, two float32 of one channel: planes most significant first, then byte differences
    b = bytes([0x11, 0x22, 0x33, 0x44, 0x15, 0x26, 0x37, 0x48])
    planes = bytes([0x44, 0x48, 0x33, 0x37, 0x22, 0x26, 0x11, 0x15])
    want = bytes([planes[0]] + [(planes[i] - planes[i - 1]) & 0xFF for i in range(1, 8)])
    assert tm.apply(b, 1, 2, 1, 4, 3) == want and tm.undo(want, 1, 2, 1, 4, 3) == b


def test_pad_crop_rows_and_classes():
    kept = bytes(range(12))
    seg = tm.pad(kept, (2, 2), (3, 3), 3, 1)
    assert seg == bytes([0, 1, 2, 3, 4, 5, 0, 0, 0, 6, 7, 8, 9, 10, 11, 0, 0, 0] + [0] * 9)
    assert tm.crop(seg, (2, 2), (3, 3), 3, 1) == kept
    r = tm.row(5, 6, 7, 8, (3, 3), (2, 2), 3, 1, 2)
    assert r == [5, 6, 7, 8, 3 | 3 << 32, 2 | 2 << 32, 3 | 1 << 8 | 2 << 16, 0]
    assert tm.unpack(r)["coded"] == 27 and tm.classify(r) == tm.SCAN
    assert tm.classify(tm.row(0, 0, 0, 9, (3, 3), (3, 3), 3, 1, 1)) == tm.DIRECT
    assert tm.classify(tm.row(0, 0, 0, 10, (3, 3), (3, 3), 3, 1, 1)) == tm.SCAN      # a pitch of its own
    assert tm.classify(tm.row(0, 0, 0, 10, (3, 1), (3, 1), 3, 1, 1)) == tm.DIRECT    # ... of a single row
    assert tm.classify(tm.row(0, 0, 0, 9, (3, 3), (3, 2), 3, 1, 1)) == tm.SCAN
    assert tm.classify(tm.row(0, 0, 0, 12, (3, 3), (3, 3), 1, 4, 3)) == tm.SCAN_GATHER
    from libdeflate_amd import api
    assert api.tiff_rows([7], [8], (3, 3), (2, 2), 3, 1, 2, [5], [6]).tolist() == [r]
    assert api.tiff_rows([7, 9], 8, [(3, 3), (4, 1)], None, 3, [1, 2], 2).tolist() == \
        tm.rows([7, 9], 8, [(3, 3), (4, 1)], None, 3, [1, 2], 2).tolist()


def test_parse_refuses_what_is_not_covered():
    name, data, _ = ts.fixtures()[0]
    with pytest.raises(ValueError, match="big-endian"):
        tiff.parse(b"MM\x00*" + data[4:])
    with pytest.raises(ValueError):
        tiff.parse(b"II")
    with pytest.raises(ValueError, match="header"):
        tiff.parse(b"PK\x03\x04" + data[4:])

    def with_tag(tag, value):
        streams = [zlib.compress(bytes(4 * 3))]
        f = bytearray(tiff.build(4, 1, 3, 1, 1, 1, streams))
        at = int.from_bytes(f[4:8], "little")
        for k in range(int.from_bytes(f[at:at + 2], "little")):
            e = at + 2 + 12 * k
            if int.from_bytes(f[e:e + 2], "little") == tag:
                f[e + 8:e + 12] = value.to_bytes(4, "little")
                return bytes(f)
        raise AssertionError(tag)
    assert len(tiff.parse(with_tag(tiff.COMPRESSION, 8))) == 1
    assert tiff.parse(with_tag(tiff.COMPRESSION, 32946))[0].compression == 32946
    for comp in (1, 5, 7, 50000, 34887):           # none, LZW, JPEG, ZSTD, LERC
        with pytest.raises(ValueError, match="compression"):
            tiff.parse(with_tag(tiff.COMPRESSION, comp))
    with pytest.raises(ValueError, match="Planar"):
        tiff.parse(with_tag(tiff.PLANAR, 2))
    with pytest.raises(ValueError, match="predictor"):
        tiff.parse(with_tag(tiff.PREDICTOR, 3))     # on 8-bit samples
    with pytest.raises(ValueError, match="predictor"):
        tiff.parse(with_tag(tiff.PREDICTOR, 4))
    with pytest.raises(ValueError, match="outside"):
        tiff.parse(with_tag(tiff.STRIP_COUNTS, 1 << 20))


def test_parse_reads_bigtiff():
    """the same image as a hand-made BigTIFF: 8-byte offsets and counts"""
    import struct
    pixels = ts.random_bytes(43, 5 * 3 * 2)
    stream = zlib.compress(tm.apply(pixels, 3, 5, 1, 2, 2))
    body = bytearray(b"II+\x00\x08\x00\x00\x00" + bytes(8)) + stream
    entries = [(256, 4, 5), (257, 4, 3), (258, 3, 16), (259, 3, 8), (273, 16, 16), (277, 3, 1),
               (278, 4, 3), (279, 16, len(stream)), (317, 3, 2)]
    struct.pack_into("<Q", body, 8, len(body))
    body += struct.pack("<Q", len(entries))
    for tag, typ, val in entries:
        body += struct.pack("<HHQQ", tag, typ, 1, val)
    body += struct.pack("<Q", 0)
    im, got = _decode(bytes(body))
    assert got == pixels and (im.width, im.height, im.bps, im.predictor) == (5, 3, 2, 2)


def _build(width, height, spp, dtype, pred, seed, rows_per_strip=None, tile=None):
    """an image through apply(), Python's zlib and tiff.build() -> (file, array)"""
    bps = np.dtype(dtype).itemsize
    px = spp * bps
    raw = np.frombuffer(ts.random_bytes(seed, width * height * px), dtype=np.uint8).copy()
    if dtype == np.float32:     # (no NaNs: they need not compare equal)
        bits = raw.view(np.uint32)
        bits[(bits & 0x7F800000) == 0x7F800000] &= 0xBFFFFFFF
    img = raw.reshape(height, width * px)
    streams = []
    if tile:
        tw, tl = tile
        for y0 in range(0, height, tl):
            for x0 in range(0, width, tw):
                kept = img[y0:y0 + tl, x0 * px:(x0 + tw) * px]
                seg = tm.pad(kept.tobytes(), (kept.shape[1] // px, kept.shape[0]), tile, spp, bps)
                streams.append(zlib.compress(tm.apply(seg, tl, tw, spp, bps, pred)))
    else:
        rps = height if rows_per_strip is None else rows_per_strip
        for y0 in range(0, height, rps):
            strip = img[y0:y0 + rps]
            streams.append(zlib.compress(tm.apply(strip.tobytes(), strip.shape[0], width, spp, bps, pred)))
    fmt = 3 if dtype == np.float32 else 1
    data = tiff.build(width, height, spp, bps, fmt, pred, streams, rows_per_strip=rows_per_strip,
                      tile=tile)
    arr = raw.view(dtype).reshape((height, width, spp) if spp > 1 else (height, width))
    return data, arr


BUILT = [(40, 23, 3, np.uint8, 2, None, (16, 16)), (40, 23, 1, np.uint16, 2, None, (16, 16)),
         (33, 17, 1, np.float32, 3, None, (16, 32)), (53, 23, 4, np.uint8, 2, 5, None),
         (1, 9, 1, np.uint8, 1, 4, None), (300, 7, 3, np.uint8, 1, None, None),
         (19, 21, 1, np.float32, 2, 8, None), (64, 32, 1, np.float32, 3, None, (32, 16))]


@pytest.mark.parametrize("case", BUILT, ids=[str(k) for k in range(len(BUILT))])
def test_build_round_trips_through_parse(case):
    width, height, spp, dtype, pred, rps, tile = case
    data, arr = _build(width, height, spp, dtype, pred, [1] + list(case[:3]), rps, tile)
    im, got = _decode(data)
    assert got == arr.tobytes()
    assert im.tiled == (tile is not None)
    if tile:
        assert (im.seg_width, im.seg_rows) == tile
        rows = im.rows()
        assert all((int(r[4]) & 0xFFFFFFFF, int(r[4]) >> 32) == tile for r in rows)
        assert int(rows[-1][5]) & 0xFFFFFFFF == width - (im.across - 1) * tile[0]
        assert int(rows[-1][5]) >> 32 == height - (im.down - 1) * tile[1]
    with pytest.raises(ValueError, match="streams"):
        tiff.build(width, height, spp, np.dtype(dtype).itemsize, 1, pred, [], rows_per_strip=rps,
                   tile=tile)


@pytest.mark.parametrize("case", BUILT, ids=[str(k) for k in range(len(BUILT))])
def test_built_files_open_in_pillow(case, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    width, height, spp, dtype, pred, rps, tile = case
    data, arr = _build(width, height, spp, dtype, pred, [2] + list(case[:3]), rps, tile)
    path = tmp_path / "built.tif"
    path.write_bytes(data)
    with Image.open(path) as im:
        got = np.asarray(im)
    assert got.shape == arr.shape and got.tobytes() == arr.tobytes()


def test_fresh_pillow_files_agree_with_the_fixtures(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    for mode, c, dtype, pred, w, h, rps, content in list(gen.cases())[::4]:
        name = gen.name(mode, pred, w, h, rps, content)
        a = gen.pixels(mode, c, dtype, pred, w, h, rps, content)
        assert a.tobytes() == np.load(os.path.join(ts.GOLDEN, name + ".npy")).tobytes()
        path = str(tmp_path / (name + ".tif"))
        Image.fromarray(a).save(path, compression="tiff_adobe_deflate", tiffinfo={317: pred, 278: rps})
        im, got = _decode(open(path, "rb").read())
        assert got == a.tobytes() and im.predictor == pred, name
