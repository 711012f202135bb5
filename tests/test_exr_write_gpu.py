"""OpenEXR ZIP / ZIPS chunks written on the GPU (libdeflate_amd_exr_encode_batch).
No tolerance anywhere: every chunk's stream equals the single-buffer zlib
Compressor call of this build on the model's coded bytes
(tools/models/exr_model.py), the choice between stream and raw chunk equals
len(stream) < n, head ints, dataSize, offsets, d_result and d_index equal the
model's, Python's zlib and the model's undo give the pixels back, the reader
takes d_out and the index as they are, exr.build() puts a header in front that
exr.parse() reads, and the canary bytes in front of d_out and behind out_avail
stay untouched.  The pixels are packed at unaligned offsets with junk between
the chunks and in every pitch gap, and out_avail is exactly what is written."""
import os
import random
import re
import zlib

import numpy as np
import pytest

from tests import exr_chunks as ec
from tools.models import exr_model as em

pytestmark = pytest.mark.gpu

SUCCESS, INSUFFICIENT_SPACE = 0, 3
CANARY = 0xA5
UNSET = -7
GUARD = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, F = ec.H, ec.F


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


def stream_of(c, level):
    """the single-buffer call of this build on the chunk's coded bytes; once per level"""
    cache = c.__dict__.setdefault("streams", {})
    if level not in cache:
        cache[level] = _compressor(level).compress("zlib", em.apply(c.raw))
        assert cache[level] is not None
    return cache[level]


@pytest.fixture(scope="module")
def cases():
    """the reader's shapes, each with a head: scanline chunks and tiles by turns"""
    cs = ec.edge_chunks()
    for k, c in enumerate(cs):
        c.head = ((k * 16 - 40,), (k % 7, k // 7, 0, 0), ())[k % 3]
    return cs


def _segment_min():
    """the size from which a chunk is compressed as primed segments: the plan's"""
    text = open(os.path.join(ROOT, "libdeflate_amd", "csrc", "large_plan.h")).read()
    seg = int(re.search(r"#define LDA_SEG_BYTES (\d+)u", text).group(1))
    assert re.search(r"#define LDA_LARGE_MIN \(2 \* LDA_SEG_BYTES\)", text)
    return 2 * seg


def write(torch, level, cs, seed=0, short=0, read_back=True, both=False):
    """one call over the chunks into exactly the room they need (less `short`
    bytes); everything checked -> (the output bytes, the index)"""
    from libdeflate_amd import api
    comp = _compressor(level)
    rng = random.Random(seed)
    buf, offs = bytearray(), []
    for c in cs:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 8)))
        offs.append(len(buf))
        lines = c.lines()
        for y, line in enumerate(lines):        # the lines at their pitch, junk in the gaps
            buf += line
            if y + 1 < len(lines):
                buf += bytes(rng.randrange(256) for _ in range(c.extra))
    buf += b"tail"
    n = len(cs)
    rows = np.array([c.row(0, offs[k], 0) for k, c in enumerate(cs)], dtype=np.uint64).reshape(
        n, em.WORDS)
    bound = comp.exr_encode_bound(rows) if n else 0
    assert bound == em.bound(rows.tolist()) == sum(int(r[7]) + c.n for r, c in zip(rows.tolist(), cs))
    want, kinds = [], []
    for c, r in zip(cs, rows.tolist()):
        z = stream_of(c, level)
        data = z if len(z) < c.n else c.raw
        kinds.append(len(z) < c.n)
        want.append(em.head_bytes(r, len(data)) + data)
    if both:
        assert set(kinds) == {False, True}, "both branches in one batch"
    if level == 0:
        assert not any(kinds)
    total = sum(len(w) for w in want)
    assert total <= bound
    avail = total - short
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    result = torch.full((em.RESULT_WORDS + 1,), UNSET, dtype=torch.int64, device="cuda")
    index = torch.full((em.WORDS * n + 1,), UNSET, dtype=torch.int64, device="cuda")
    comp.encode_exr_batch(rows, d_in, whole[GUARD:], result, index, in_avail=len(buf) - 4,
                          out_avail=avail)
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    res = result.cpu().tolist()
    idx = index.cpu().numpy()
    assert not (host[:GUARD] != CANARY).any(), "bytes written in front of d_out"
    assert not (host[GUARD + avail:] != CANARY).any(), "bytes written past out_avail"
    assert res[em.RESULT_WORDS] == UNSET and idx[em.WORDS * n] == UNSET
    if n == 0:
        assert res[:4] == [UNSET] * 4   # nothing to do: nothing is queued
        return b"", idx
    raw_total = sum(c.n for c in cs)
    if short:
        assert res[:4] == [INSUFFICIENT_SPACE, total, raw_total, n]
        assert not (host != CANARY).any(), "bytes written though the chunks do not fit"
        assert (idx == UNSET).all()
        return None, None
    assert res[0] == SUCCESS
    out = host[GUARD:GUARD + total].tobytes()
    at, want_rows = 0, []
    for k, (w, c) in enumerate(zip(want, cs)):
        got = out[at:at + len(w)]
        r = rows[k].tolist()
        head = int(r[7])
        assert got[:head] == w[:head], "chunk %d: head %r, not %r" % (k, got[:head], w[:head])
        assert got == w, "chunk %d (channels %r, size %r, layout %d, n %d, %s): data differs at byte " \
            "%d" % (k, c.wide, c.size, c.layout, c.n, "stream" if kinds[k] else "raw",
                    next((i for i in range(len(w)) if got[i] != w[i]), -1) - head)
        body = got[head:]
        raw = em.undo(zlib.decompress(body)) if kinds[k] else body
        assert raw == c.raw and em.expected(r, raw) == c.lines()
        want_rows.append([at + head, len(body)] + [int(x) for x in r[2:]])
        at += len(w)
    assert res[:4] == [SUCCESS, total, raw_total, n]
    assert idx[:em.WORDS * n].view(np.uint64).reshape(n, em.WORDS).tolist() == want_rows
    if read_back:
        # d_out and the index straight to the reader, the lines where the input was
        dec = api.Decompressor()
        back = torch.full((len(buf),), CANARY, dtype=torch.uint8, device="cuda")
        per = torch.full((n,), UNSET, dtype=torch.int32, device="cuda")
        dec.decode_exr_batch(idx[:em.WORDS * n].view(np.uint64), whole[GUARD:], back, per,
                             in_nbytes=total, out_avail=len(buf) - 4)
        torch.cuda.synchronize()
        assert per.cpu().tolist() == [SUCCESS] * n
        got = back.cpu().numpy()
        want_back = np.full(len(buf), CANARY, dtype=np.uint8)
        for k, c in enumerate(cs):
            for y, line in enumerate(c.lines()):
                a = offs[k] + y * c.pitch
                want_back[a:a + len(line)] = np.frombuffer(line, dtype=np.uint8)
        assert (got == want_back).all()
        dec.close()
    return out, idx[:em.WORDS * n].reshape(n, em.WORDS)


@pytest.mark.parametrize("level", [1, 6, 9])
def test_shapes_mixed_in_one_batch(torch, cases, level):
    cs = cases[level % 3::3]
    random.Random(level).shuffle(cs)
    write(torch, level, cs, seed=level, both=True)


def test_every_shape_at_level_6(torch, cases):
    write(torch, 6, cases, seed=11, both=True)


@pytest.mark.parametrize("level", [0, 12])
def test_levels_0_and_12_on_a_smaller_set(torch, cases, level):
    """at level 0 every chunk is raw: its stored blocks are longer than it"""
    write(torch, level, cases[3::6], seed=20 + level)


def test_a_chunk_above_the_segmentation_threshold(torch):
    """the primed-segment path: chunks of the threshold's size and more between
    small ones, one just below it, which is one piece, and a large one of random
    samples, which is stored raw from its pieces' ranges"""
    edge = _segment_min()
    assert edge == 131072
    cs = [ec.Chunk([H] * 4, (9, 7), em.PIXELS, [3, 2, 1, 0], extra=3, few=True, seed=1, head=(0,)),
          ec.Chunk([H] * 4, (1026, 16), em.PIXELS, [3, 2, 1, 0], few=True, seed=2, head=(16,)),
          ec.Chunk([F], (2048, 16), few=True, seed=3, head=(32,)),              # exactly the threshold
          ec.Chunk([H], (65535, 1), few=True, seed=4, head=(48,)),              # two bytes below it
          ec.Chunk([H] * 4, (2048, 16), em.PIXELS, None, extra=8, seed=5, head=(49,)),  # random: raw
          ec.Chunk([H] * 3, (300, 100), em.LINES, extra=8, few=True, seed=6, head=(1, 2, 0, 0))]
    assert [c.n >= edge for c in cs] == [False, True, True, False, True, True]
    out, _ = write(torch, 6, cs, seed=30, both=True)
    # the segmented streams are segmented: they hold the empty stored blocks
    # that end a segment on a byte boundary
    assert out.count(b"\x00\x00\xff\xff") >= 3


def test_out_avail_one_byte_short_and_exact(torch, cases):
    """an all-raw batch at out_avail = bound - 1 writes nothing"""
    cs = [c for c in cases if not c.few][5::4]
    comp = _compressor(6)
    rows = [c.row(0, 0, 0) for c in cs]
    assert all(len(stream_of(c, 6)) >= c.n for c in cs)
    assert comp.exr_encode_bound(np.array(rows, dtype=np.uint64)) == \
        sum(r[7] + c.n for r, c in zip(rows, cs))
    write(torch, 6, cs, seed=40, short=1)
    write(torch, 6, cs, seed=40, read_back=False)
    mixed = cases[5::9]
    write(torch, 6, mixed, seed=41, short=1)


@pytest.mark.parametrize("tile", [None, (32, 32)])
def test_a_written_file_parses(torch, tile):
    """an image's chunks encoded from an H x W x 4 RGBA half tensor, exr.build()'s
    header in front: exr.parse() finds every chunk, Python's zlib and the model
    give back the planes, and the reader the tensor"""
    from libdeflate_amd import api, binding, exr
    channels = [("A", exr.HALF), ("B", exr.HALF), ("G", exr.HALF), ("R", exr.HALF)]
    width, height = 75, 37
    planes = ec.image(width, height, channels, seed=9)
    pixels = ec.interleaved(planes, [3, 2, 1, 0])       # R, G, B, A
    px, comp = 8, _compressor(6)
    if tile:
        regions = [(x0, y0, min(tile[0], width - x0), min(tile[1], height - y0))
                   for y0 in range(0, height, tile[1]) for x0 in range(0, width, tile[0])]
        heads = [(x0 // tile[0], y0 // tile[1], 0, 0) for x0, y0, _, _ in regions]
    else:
        regions = [(0, y0, width, min(16, height - y0)) for y0 in range(0, height, 16)]
        heads = [(y0,) for _, y0, _, _ in regions]
    rows = api.exr_rows([y0 * width * px + x0 * px for x0, y0, _, _ in regions], width * px,
                        [(w, l) for _, _, w, l in regions], [False] * 4, binding.EXR_PIXELS,
                        [3, 2, 1, 0], None, None, heads)
    n = len(rows)
    bound = comp.exr_encode_bound(rows)
    d_in = torch.frombuffer(bytearray(pixels.tobytes()), dtype=torch.uint8).cuda()
    out = torch.full((bound,), CANARY, dtype=torch.uint8, device="cuda")
    result = torch.full((4,), UNSET, dtype=torch.int64, device="cuda")
    index = torch.full((n * em.WORDS,), UNSET, dtype=torch.int64, device="cuda")
    comp.encode_exr_batch(rows, d_in, out, result, index)
    torch.cuda.synchronize()
    res = result.cpu().tolist()
    assert res[0] == SUCCESS and res[2] == pixels.size and res[3] == n and res[1] < pixels.size
    idx = index.cpu().numpy().view(np.uint64).reshape(n, em.WORDS)
    head = exr.build(width, height, channels, exr.ZIP, idx, tile)
    data = head + out.cpu().numpy()[:res[1]].tobytes()
    im = exr.parse(data)
    assert (im.width, im.height, im.channels, im.compression, im.tile) == \
        (width, height, channels, exr.ZIP, tile)
    assert im.chunks[:, exr.T_DATA_N].tolist() == idx[:, 1].tolist()
    assert [(int(t[exr.T_X0]), int(t[exr.T_Y0]), int(t[exr.T_W]), int(t[exr.T_LINES]))
            for t in im.chunks] == regions
    for t, (x0, y0, w, l) in zip(im.chunks.tolist(), regions):
        stored = data[t[exr.T_DATA_OFF]:t[exr.T_DATA_OFF] + t[exr.T_DATA_N]]
        raw = stored if len(stored) == w * l * px else em.undo(zlib.decompress(stored))
        assert raw == ec.raw_chunk(planes, x0, y0, w, l)
    # ... and the file back through the reader into the same tensor
    dec = api.Decompressor()
    d_file = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    back = torch.full((pixels.size,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((n,), UNSET, dtype=torch.int32, device="cuda")
    dec.decode_exr_batch(im.rows(layout=binding.EXR_PIXELS, order="RGBA"), d_file, back, per)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [SUCCESS] * n
    assert back.cpu().numpy().tobytes() == pixels.tobytes()
    dec.close()


def test_no_chunks_does_nothing(torch):
    assert write(torch, 6, [], seed=50)[0] == b""
