"""Predictor-coded deflate strips and tiles (TIFF, GeoTIFF) read on the GPU
(libdeflate_amd_tiff_decode_batch).  No tolerance anywhere: every result and
every byte of every kept rectangle equal what Python's zlib and the CPU model
(tools/models/tiff_model.py) state - and, for the files of tests/golden/tiff,
what Pillow and libtiff wrote -, and the canary bytes in front of d_out, in
every pitch gap, between the rectangles and behind out_avail stay untouched.
The stored segments are packed at unaligned offsets with junk between them, the
rectangles at unaligned offsets too, and out_avail is exactly the end of the
last kept byte."""
import random
import zlib

import numpy as np
import pytest

from tests import tiff_segments as ts
from tools.models import tiff_model as tm

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
CANARY = 0xA5
UNSET = -7      # d_results where nothing was written
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec():
    from libdeflate_amd import api
    d = api.Decompressor()
    yield d
    d.close()


class Seg:
    """pixels: the coded segment's pixels (the padding holds pixels too, as an
    edge tile's does); stored: the zlib stream of the predicted segment; want:
    the result; room: 'pixels' (the kept rectangle holds them) or 'any'"""

    def __init__(self, spp, bps, pred, coded, kept=None, extra=0, seed=0, level=1):
        self.spp, self.bps, self.pred, self.coded = spp, bps, pred, coded
        self.kept, self.extra = kept or coded, extra
        n = coded[0] * coded[1] * spp * bps
        self.pixels = ts.random_bytes([seed, spp, bps, pred, coded[0], coded[1]], n)
        self.predicted = tm.apply(self.pixels, coded[1], coded[0], spp, bps, pred)
        self.stored = zlib.compress(self.predicted, level)
        self.want, self.room = SUCCESS, "pixels"

    @property
    def kept_rb(self):
        return self.kept[0] * self.spp * self.bps

    def row(self, stored_off, raw_off):
        return tm.row(stored_off, len(self.stored), raw_off, self.kept_rb + self.extra, self.coded,
                      self.kept, self.spp, self.bps, self.pred)


def run(torch, dec, segs, seed=0, stream=None, sync=True):
    """one call over the segments -> a closure that checks everything (called
    at once unless sync is False)"""
    rng = random.Random(seed)
    buf, rows, at = bytearray(), [], 0
    for s in segs:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 8)))
        at += rng.randrange(0, 4)       # a gap of canary bytes in front of the rectangle
        rows.append(s.row(len(buf), at))
        buf += s.stored
        at += (s.kept[1] - 1) * (s.kept_rb + s.extra) + s.kept_rb
    buf += b"\x78\x9c" * 5              # behind the last segment: never read as part of it
    total = at
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((len(segs) + 1,), UNSET, dtype=torch.int32, device="cuda")
    if stream is not None:      # the uploads are the current stream's work
        stream.wait_stream(torch.cuda.current_stream())
    got_rows = dec.decode_tiff_batch(rows, d_in, whole[GUARD:], per, stream=stream, out_avail=total)
    assert got_rows.tolist() == rows

    def check():
        host = whole.cpu().numpy()
        assert not (host[:GUARD] != CANARY).any(), "bytes written in front of d_out"
        assert not (host[GUARD + total:] != CANARY).any(), "bytes written past out_avail"
        host = host[GUARD:GUARD + total]
        res = per.cpu().numpy()
        assert res[len(segs)] == UNSET
        want = np.full(total, CANARY, dtype=np.uint8)
        defined = np.ones(total, dtype=bool)
        for s, r in zip(segs, rows):
            for y, line in enumerate(tm.expected(r, s.pixels)):
                a = r[2] + y * r[3]
                if s.room == "pixels":
                    want[a:a + len(line)] = np.frombuffer(line, dtype=np.uint8)
                else:
                    defined[a:a + len(line)] = False
        assert res[:len(segs)].tolist() == [s.want for s in segs]
        bad = np.nonzero((host != want) & defined)[0]
        if bad.size:
            k = max(i for i, r in enumerate(rows) if r[2] <= bad[0])
            s = segs[k]
            raise AssertionError("first wrong byte at %d of %d: segment %d (spp %d, bps %d, predictor "
                                 "%d, coded %r, kept %r, pitch +%d) byte %d; %d wrong in all" %
                                 (bad[0], total, k, s.spp, s.bps, s.pred, s.coded, s.kept, s.extra,
                                  bad[0] - rows[k][2], bad.size))
        return host, rows, bytes(buf)
    if not sync:
        return check
    torch.cuda.synchronize()
    return check()


@pytest.fixture(scope="module")
def edge_segs():
    segs = [Seg(*shape, seed=k) for k, shape in enumerate(ts.shapes())]
    assert sum(len(s.pixels) for s in segs) < 8 << 20
    classes = {tm.classify(s.row(0, 0)) for s in segs}
    assert classes == {tm.SCAN, tm.SCAN_GATHER}
    return segs


def test_fixture_files_decode_to_their_pixels(torch, dec):
    """every file of tests/golden/tiff (Pillow, libtiff), all in one batch:
    tiff.parse()'s rows, the pixels at H x W x C"""
    from libdeflate_amd import tiff
    files = ts.fixtures()
    assert len(files) >= 40
    blob, rows, at, spans = bytearray(), [], 0, []
    for name, data, pixels in files:
        (im,) = tiff.parse(data)
        assert im.nbytes == len(pixels)
        at += 3                                 # (unaligned images, canary between them)
        r = im.rows(offset=at)
        r[:, 0] += np.uint64(len(blob) + 1)
        rows.append(r)
        spans.append((at, pixels))
        blob += b"\x00" + data
        at += len(pixels)
    rows = np.concatenate(rows)
    preds = {int(r[6]) >> 16 for r in rows}
    assert preds == {1, 2, 3}
    d_in = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    whole = torch.full((GUARD + at + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((len(rows) + 1,), UNSET, dtype=torch.int32, device="cuda")
    dec.decode_tiff_batch(rows, d_in, whole[GUARD:], per, out_avail=at)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [SUCCESS] * len(rows) + [UNSET]
    want = np.full(GUARD + at + GUARD, CANARY, dtype=np.uint8)
    for (a, pixels), (name, _, _) in zip(spans, files):
        want[GUARD + a:GUARD + a + len(pixels)] = np.frombuffer(pixels, dtype=np.uint8)
    host = whole.cpu().numpy()
    for (a, pixels), (name, _, _) in zip(spans, files):
        got = host[GUARD + a:GUARD + a + len(pixels)]
        assert got.tobytes() == pixels, name
    assert (host == want).all()


def test_all_shapes_mixed_in_one_batch(torch, dec, edge_segs):
    segs = list(edge_segs)
    random.Random(3).shuffle(segs)
    run(torch, dec, segs, seed=1)


def test_shapes_in_their_own_order_and_small_batches(torch, dec, edge_segs):
    """the same segments unshuffled - runs of one format - and, one group size
    at a time, in batches of their own"""
    run(torch, dec, edge_segs, seed=2)
    for g in (4, 16, 64):
        part = [s for s in edge_segs
                if tm.group(s.kept_rb if s.pred != 3 else s.coded[0] * s.spp * s.bps,
                            s.spp if s.pred == 3 else s.spp * s.bps if s.pred == 2 else 0) == g][::7]
        assert part
        run(torch, dec, part, seed=g)


def _tiled(width, height, spp, bps, pred, tile, seed):
    """a TIFF of one tiled image through tiff.build() -> (file, pixels)"""
    from libdeflate_amd import tiff
    px = spp * bps
    pixels = np.frombuffer(ts.random_bytes(seed, width * height * px), dtype=np.uint8)
    img = pixels.reshape(height, width * px)
    tw, tl = tile
    streams = []
    for y0 in range(0, height, tl):
        for x0 in range(0, width, tw):
            kept = img[y0:y0 + tl, x0 * px:(x0 + tw) * px]
            seg = tm.pad(kept.tobytes(), (kept.shape[1] // px, kept.shape[0]), tile, spp, bps)
            streams.append(zlib.compress(tm.apply(seg, tl, tw, spp, bps, pred), 6))
    return tiff.build(width, height, spp, bps, 1, pred, streams, tile=tile), pixels.tobytes()


@pytest.mark.parametrize("spp,bps,pred", [(3, 1, 2), (1, 2, 2), (1, 4, 3), (3, 1, 1)])
def test_tiles_land_in_one_image(torch, dec, spp, bps, pred):
    """a 40 x 23 image as six 16 x 16 tiles, the right and bottom ones cropped:
    the output is the image, the canaries around it are intact"""
    from libdeflate_amd import tiff
    data, pixels = _tiled(40, 23, spp, bps, pred, (16, 16), [40, spp, bps, pred])
    (im,) = tiff.parse(data)
    assert im.tiled and (im.across, im.down) == (3, 2) and im.nbytes == len(pixels)
    rows = im.rows(offset=5)
    assert [int(r[5]) & 0xFFFFFFFF for r in rows] == [16, 16, 8] * 2
    assert [int(r[5]) >> 32 for r in rows] == [16] * 3 + [7] * 3
    total = 5 + len(pixels)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((7,), UNSET, dtype=torch.int32, device="cuda")
    dec.decode_tiff_batch(rows, d_in, whole[GUARD:], per, out_avail=total)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [SUCCESS] * 6 + [UNSET]
    host = whole.cpu().numpy()
    assert host[GUARD + 5:GUARD + total].tobytes() == pixels
    assert (host[:GUARD + 5] == CANARY).all() and (host[GUARD + total:] == CANARY).all()


def test_direct_batch_is_decompress_batch(torch, dec):
    """a batch that is direct throughout - predictor 1, kept whole, at the
    row's own pitch or a single row -, byte for byte against
    libdeflate_amd_decompress_batch on the same streams and rooms"""
    segs = [Seg(spp, bps, 1, coded, extra=extra, seed=90 + k) for k, (spp, bps, coded, extra) in
            enumerate([(1, 1, (1, 1), 0), (3, 1, (300, 40), 0), (4, 2, (17, 1), 9), (1, 4, (256, 256), 0),
                       (16, 8, (3, 2), 0), (5, 1, (1000, 1), 3)])]
    for s in segs:
        assert tm.classify(s.row(0, 0)) == tm.DIRECT
    host, rows, buf = run(torch, dec, segs, seed=5)
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    r = np.array(rows, dtype=np.int64)
    sizes = [len(s.pixels) for s in segs]
    cols = [torch.tensor(c, dtype=torch.int64, device="cuda")
            for c in (r[:, 0].tolist(), r[:, 1].tolist(), r[:, 2].tolist(), sizes)]
    total = int(r[-1, 2]) + sizes[-1]
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((len(segs),), UNSET, dtype=torch.int32, device="cuda")
    dec.decompress_batch("zlib", d_in, cols[0], cols[1], out, cols[2], cols[3], per)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [SUCCESS] * len(segs)
    assert (out.cpu().numpy() == host).all()


def _defects():
    """(name, segment) of every failure, on a cropped RGB tile at a pitch"""
    def base(seed):
        return Seg(3, 1, 2, (70, 9), (61, 8), 5, seed=seed, level=6)
    out = []
    s = base(1)
    s.stored, s.want, s.room = s.stored[:-7], BAD_DATA, "any"
    out.append(("truncated", s))
    s = base(2)
    s.stored, s.want, s.room = zlib.compress(s.predicted[:-1], 6), SHORT_OUTPUT, "any"
    out.append(("short", s))
    s = base(3)
    s.stored, s.want, s.room = zlib.compress(s.predicted + b"\x00", 6), INSUFFICIENT_SPACE, "any"
    out.append(("long", s))
    s = base(4)
    z = bytearray(s.stored)
    z[-1] ^= 0x10
    s.stored, s.want, s.room = bytes(z), BAD_DATA, "any"
    out.append(("adler", s))
    s = Seg(1, 4, 3, (33, 5), (30, 5), 0, seed=5, level=6)     # ... and a float one
    z = bytearray(s.stored)
    z[-2] ^= 0x01
    s.stored, s.want, s.room = bytes(z), BAD_DATA, "any"
    out.append(("adler-float", s))
    return out


def test_failures_leave_their_neighbours_intact(torch, dec):
    good = [Seg(3, 1, 2, (64, 16), (50, 11), 3, seed=20), Seg(1, 2, 2, (301, 3), seed=21),
            Seg(1, 4, 3, (53, 7), (53, 6), 1, seed=22), Seg(4, 1, 1, (9, 9), seed=23),
            Seg(5, 1, 2, (77, 2), (70, 2), 0, seed=24), Seg(1, 8, 3, (16, 16), (9, 9), 2, seed=25)]
    segs = []
    for k, (name, s) in enumerate(_defects()):
        segs += [good[k % len(good)], s, good[(k + 3) % len(good)]]
    run(torch, dec, segs, seed=6)
    # each alone between two neighbours, and first and last of a batch
    for name, s in _defects():
        run(torch, dec, [s, good[0], s], seed=7)


def test_two_calls_queued_on_a_side_stream(torch, dec, edge_segs):
    """a non-default stream, and two calls on one object without a
    synchronisation between them: the second call's plan and scratch follow the
    first's in stream order"""
    st = torch.cuda.Stream()
    check_a = run(torch, dec, edge_segs[::5], seed=9, stream=st, sync=False)
    check_b = run(torch, dec, edge_segs[2::7], seed=10, stream=st, sync=False)
    st.synchronize()
    check_a()
    check_b()


def test_nothing_to_do(torch, dec):
    from libdeflate_amd import binding
    out = torch.full((16,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((1,), UNSET, dtype=torch.int32, device="cuda")
    dec.decode_tiff_batch(np.zeros((0, binding.TIFF_WORDS), dtype=np.uint64), out, out, per)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [UNSET] and (out.cpu().numpy() == CANARY).all()
