"""Predictor-coded deflate strips and tiles (TIFF, GeoTIFF) written on the GPU
(libdeflate_amd_tiff_encode_batch).  No tolerance anywhere: every stream equals
the single-buffer zlib Compressor call of this build on the model's predicted,
zero-padded segment (tools/models/tiff_model.py), Python's zlib and the model's
undo give the pixels back, d_result and d_index equal the model's rows, the
reader takes d_out and the rows as they are, and the canary bytes in front of
d_out and behind out_avail stay untouched.  The raw rectangles are packed at
unaligned offsets with junk between them and in every pitch gap, and out_avail
is exactly the streams' size."""
import os
import random
import re
import zlib

import numpy as np
import pytest

from tests import tiff_segments as ts
from tools.models import tiff_model as tm

pytestmark = pytest.mark.gpu

SUCCESS, INSUFFICIENT_SPACE = 0, 3
CANARY = 0xA5
UNSET = -7
GUARD = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


_COMP = {}


def _compressor(level):
    from libdeflate_amd import api
    if level not in _COMP:
        _COMP[level] = api.Compressor(level)
    return _COMP[level]


class Case:
    """kept: the kept rectangle's pixels; predicted: the model's predicted,
    zero-padded segment"""

    def __init__(self, spp, bps, pred, coded, kept, extra, seed=0, smooth=False):
        self.spp, self.bps, self.pred, self.coded, self.kept, self.extra = spp, bps, pred, coded, kept, extra
        self.kept_rb = kept[0] * spp * bps
        self.pixels = ts.random_bytes([7, seed, spp, bps, pred, kept[0], kept[1]], self.kept_rb * kept[1])
        if smooth:      # bytes that compress: a slow walk
            steps = np.frombuffer(self.pixels, dtype=np.uint8) % 3
            self.pixels = np.cumsum(steps, dtype=np.uint8).tobytes()
        self.padded = tm.pad(self.pixels, kept, coded, spp, bps)
        self.predicted = tm.apply(self.padded, coded[1], coded[0], spp, bps, pred)
        self._streams = {}

    def stream(self, level):
        """the single-buffer call of this build on the predicted segment; once per level"""
        if level not in self._streams:
            self._streams[level] = _compressor(level).compress("zlib", self.predicted)
            assert self._streams[level] is not None
        return self._streams[level]


@pytest.fixture(scope="module")
def cases():
    return [Case(*shape, seed=k) for k, shape in enumerate(ts.shapes())]


def _segment_min():
    """the size from which a segment is compressed as primed segments: the plan's"""
    text = open(os.path.join(ROOT, "libdeflate_amd", "csrc", "large_plan.h")).read()
    seg = int(re.search(r"#define LDA_SEG_BYTES (\d+)u", text).group(1))
    assert re.search(r"#define LDA_LARGE_MIN \(2 \* LDA_SEG_BYTES\)", text)
    return 2 * seg


def write(torch, level, cs, seed=0, short=0, read_back=True):
    """one call over the cases into exactly the room the streams need (less
    `short` bytes); everything checked -> the output bytes"""
    from libdeflate_amd import api
    comp = _compressor(level)
    rng = random.Random(seed)
    buf, offs = bytearray(), []
    for c in cs:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 8)))
        offs.append(len(buf))
        for y in range(c.kept[1]):      # the rows at their pitch, junk in the gaps
            buf += c.pixels[y * c.kept_rb:(y + 1) * c.kept_rb]
            if y + 1 < c.kept[1]:
                buf += bytes(rng.randrange(256) for _ in range(c.extra))
    buf += b"tail"
    n = len(cs)
    rows = api.tiff_rows(offs, [c.kept_rb + c.extra for c in cs], [c.coded for c in cs],
                         [c.kept for c in cs], [c.spp for c in cs], [c.bps for c in cs],
                         [c.pred for c in cs])
    assert rows.tolist() == [tm.row(0, 0, offs[k], c.kept_rb + c.extra, c.coded, c.kept, c.spp, c.bps,
                                    c.pred) for k, c in enumerate(cs)]
    bound = comp.tiff_encode_bound(rows) if n else 0
    assert bound == tm.bound(rows)
    want = [c.stream(level) for c in cs]
    total = sum(len(w) for w in want)
    assert total <= bound
    avail = total - short
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    result = torch.full((tm.RESULT_WORDS + 1,), UNSET, dtype=torch.int64, device="cuda")
    index = torch.full((tm.WORDS * n + 1,), UNSET, dtype=torch.int64, device="cuda")
    comp.encode_tiff_batch(rows, d_in, whole[GUARD:], result, index, in_avail=len(buf) - 4,
                           out_avail=avail)
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    res = result.cpu().tolist()
    idx = index.cpu().numpy()
    assert not (host[:GUARD] != CANARY).any(), "bytes written in front of d_out"
    assert not (host[GUARD + avail:] != CANARY).any(), "bytes written past out_avail"
    assert res[tm.RESULT_WORDS] == UNSET and idx[tm.WORDS * n] == UNSET
    if n == 0:
        assert res[:4] == [UNSET] * 4   # nothing to do: nothing is queued
        return b""
    raw_total = sum(len(c.pixels) for c in cs)
    if short:
        assert res[:4] == [INSUFFICIENT_SPACE, total, raw_total, n]
        assert not (host != CANARY).any(), "bytes written though the streams do not fit"
        assert (idx == UNSET).all()
        return None
    assert res[0] == SUCCESS
    out = host[GUARD:GUARD + total].tobytes()
    at, want_rows = 0, []
    for k, (w, c) in enumerate(zip(want, cs)):
        got = out[at:at + len(w)]
        assert got == w, "segment %d (spp %d, bps %d, predictor %d, coded %r, kept %r): stream " \
            "differs at byte %d" % (k, c.spp, c.bps, c.pred, c.coded, c.kept,
                                    next((i for i in range(len(w)) if got[i] != w[i]), -1))
        body = zlib.decompress(got)
        assert body == c.predicted
        assert tm.crop(tm.undo(body, c.coded[1], c.coded[0], c.spp, c.bps, c.pred), c.kept, c.coded,
                       c.spp, c.bps) == c.pixels
        want_rows.append([at, len(w)] + [int(x) for x in rows[k][2:]])
        at += len(w)
    assert res[:4] == [SUCCESS, total, raw_total, n]
    assert idx[:tm.WORDS * n].reshape(n, tm.WORDS).tolist() == want_rows
    if read_back:
        # d_out and the rows straight to the reader, the rectangles where the input was
        dec = api.Decompressor()
        back = torch.full((len(buf),), CANARY, dtype=torch.uint8, device="cuda")
        per = torch.full((n,), UNSET, dtype=torch.int32, device="cuda")
        dec.decode_tiff_batch(idx[:tm.WORDS * n].view(np.uint64), whole[GUARD:], back, per,
                              in_nbytes=total, out_avail=len(buf) - 4)
        torch.cuda.synchronize()
        assert per.cpu().tolist() == [SUCCESS] * n
        got = back.cpu().numpy()
        want_back = np.full(len(buf), CANARY, dtype=np.uint8)
        for k, c in enumerate(cs):
            for y in range(c.kept[1]):
                a = offs[k] + y * (c.kept_rb + c.extra)
                want_back[a:a + c.kept_rb] = np.frombuffer(c.pixels[y * c.kept_rb:(y + 1) * c.kept_rb],
                                                           dtype=np.uint8)
        assert (got == want_back).all()
        dec.close()
    return out


@pytest.mark.parametrize("level", [1, 6, 9])
def test_shapes_mixed_in_one_batch(torch, cases, level):
    cs = cases[level % 4::4]
    random.Random(level).shuffle(cs)
    write(torch, level, cs, seed=level)


@pytest.mark.parametrize("level", [0, 12])
def test_levels_0_and_12_on_a_smaller_set(torch, cases, level):
    write(torch, level, cases[3::12], seed=20 + level)


def test_a_segment_above_the_segmentation_threshold(torch):
    """the primed-segment path: segments of the threshold's size and more
    between small ones, and one just below it, which is one piece"""
    edge = _segment_min()
    assert edge == 131072
    cs = [Case(3, 1, 2, (16, 16), (9, 7), 3, seed=1),
          Case(3, 1, 2, (256, 171), (250, 170), 0, seed=2, smooth=True),    # 131 328 bytes
          Case(1, 4, 3, (256, 128), (256, 128), 0, seed=3, smooth=True),    # exactly the threshold
          Case(1, 2, 2, (65535, 1), (65535, 1), 0, seed=4, smooth=True),    # two bytes below it
          Case(4, 2, 2, (300, 100), (300, 99), 8, seed=5)]                  # 240 000 bytes
    assert [len(c.predicted) >= edge for c in cs] == [False, True, True, False, True]
    out = write(torch, 6, cs, seed=30)
    # the segmented streams are segmented: they hold the empty stored blocks
    # that end a segment on a byte boundary
    assert out.count(b"\x00\x00\xff\xff") >= 3


def test_out_avail_one_byte_short_and_exact(torch, cases):
    cs = cases[5::29]
    write(torch, 6, cs, seed=40, short=1)
    write(torch, 6, cs, seed=40, read_back=False)


def test_no_segments_does_nothing(torch):
    assert write(torch, 6, [], seed=50) == b""
