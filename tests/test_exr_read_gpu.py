"""OpenEXR ZIP / ZIPS chunks read on the GPU (libdeflate_amd_exr_decode_batch).
No tolerance anywhere: every result and every byte of every line equal what
Python's zlib and the CPU model (tools/models/exr_model.py) state, and the
canary bytes in front of d_out, in every pitch gap, between the chunks and
behind out_avail stay untouched.  The stored chunks are packed at unaligned
offsets with junk between them, the lines at unaligned offsets too, and
out_avail is exactly the end of the last written byte.

Every sample has 2 or 4 bytes, so no row can describe a chunk of an odd number
of bytes: the sizes are the even ones around the undo kernels' edges
(tests/exr_chunks.py), those of 2 (mod 4) with a second half that starts at an
odd place; odd sizes are the CPU model's (tests/test_exr_model.py)."""
import random
import zlib

import numpy as np
import pytest

from tests import exr_chunks as ec
from tests import oracle_util
from tools.models import exr_model as em

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
CANARY = 0xA5
UNSET = -7      # d_results where nothing was written
GUARD = 64
H, F = ec.H, ec.F


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


def run(torch, dec, chunks, seed=0, stream=None, sync=True):
    """one call over the chunks -> a closure that checks everything (called at
    once unless sync is False)"""
    rng = random.Random(seed)
    buf, rows, at = bytearray(), [], 0
    for c in chunks:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 8)))
        at += rng.randrange(0, 4)       # a gap of canary bytes in front of the lines
        rows.append(c.row(len(buf), at))
        buf += c.stored
        at += (c.size[1] - 1) * c.pitch + c.lb
    buf += b"\x78\x9c" * 5              # behind the last chunk: never read as part of it
    total = at
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((len(chunks) + 1,), UNSET, dtype=torch.int32, device="cuda")
    if stream is not None:      # the uploads are the current stream's work
        stream.wait_stream(torch.cuda.current_stream())
    got_rows = dec.decode_exr_batch(rows, d_in, whole[GUARD:], per, stream=stream, out_avail=total)
    assert got_rows.tolist() == rows

    def check():
        # (d_in lives until the check: freed at the return of run(), its memory
        # could become the next call's input while this call is still queued)
        assert d_in.numel() == len(buf)
        host = whole.cpu().numpy()
        assert not (host[:GUARD] != CANARY).any(), "bytes written in front of d_out"
        assert not (host[GUARD + total:] != CANARY).any(), "bytes written past out_avail"
        host = host[GUARD:GUARD + total]
        res = per.cpu().numpy()
        assert res[len(chunks)] == UNSET
        want = np.full(total, CANARY, dtype=np.uint8)
        defined = np.ones(total, dtype=bool)
        for c, r in zip(chunks, rows):
            for y, line in enumerate(c.lines()):
                a = r[2] + y * r[3]
                if c.room == "pixels":
                    want[a:a + len(line)] = np.frombuffer(line, dtype=np.uint8)
                elif c.room == "any":
                    defined[a:a + len(line)] = False
                # ("canary": the call writes nothing there)
        assert res[:len(chunks)].tolist() == [c.want for c in chunks]
        bad = np.nonzero((host != want) & defined)[0]
        if bad.size:
            k = max(i for i, r in enumerate(rows) if r[2] <= bad[0])
            c = chunks[k]
            raise AssertionError("first wrong byte at %d of %d: chunk %d (channels %r, size %r, layout "
                                 "%d, slots %r, pitch +%d, n %d, stored %d) byte %d; %d wrong in all" %
                                 (bad[0], total, k, c.wide, c.size, c.layout, c.slots, c.extra, c.n,
                                  len(c.stored), bad[0] - rows[k][2], bad.size))
        return host, rows, bytes(buf)
    if not sync:
        return check
    torch.cuda.synchronize()
    return check()


@pytest.fixture(scope="module")
def edge_chunks():
    chunks = ec.edge_chunks()
    assert sum(c.n for c in chunks) < 8 << 20
    # the model's decision is len(stream) < n: every edge size of 16 bytes and
    # more occurs as a zlib chunk and raw, the smaller ones raw
    kinds = {}
    for c in chunks:
        assert (len(c.stored) < c.n) == (len(zlib.compress(em.apply(c.raw), 6)) < c.n)
        kinds.setdefault(c.n, set()).add(em.classify(c.row(0, 0)) == em.ZLIB)
    for n in ec.EDGE_SIZES:
        assert kinds[n] == {False, True} if n >= 16 else False in kinds[n], n
    classes = {em.classify(c.row(0, 0)) for c in chunks}
    assert classes == {em.RAW_DIRECT, em.RAW_LAYOUT, em.ZLIB}
    assert {len(c.wide) for c in chunks} >= {1, 3, 4, 5, 16}
    assert {c.size[1] for c in chunks} >= {1, 2, 15, 16, 17, 32, 64}
    assert {c.layout for c in chunks} == {em.LINES, em.PIXELS}
    return chunks


def test_all_shapes_mixed_in_one_batch(torch, dec, edge_chunks):
    chunks = list(edge_chunks)
    random.Random(3).shuffle(chunks)
    run(torch, dec, chunks, seed=1)


def test_shapes_in_their_own_order_and_by_class(torch, dec, edge_chunks):
    """the same chunks unshuffled and, one class at a time, in batches of their
    own - a batch of direct raw rows is a copy kernel and the verdicts"""
    run(torch, dec, edge_chunks, seed=2)
    for cls in (em.RAW_DIRECT, em.RAW_LAYOUT, em.ZLIB):
        part = [c for c in edge_chunks if em.classify(c.row(0, 0)) == cls]
        assert part
        run(torch, dec, part, seed=10 + cls)


def test_one_chunk_alone_at_every_edge_size(torch, dec, edge_chunks):
    """a batch of one zlib chunk: the carries restart at its first tile"""
    for c in edge_chunks[:2 * len(ec.EDGE_SIZES)]:
        if c.few:
            run(torch, dec, [c], seed=c.n)


def test_a_large_chunk_of_many_tiles(torch, dec):
    """2 MiB as one chunk - 1024 tiles, the carry kernel's wave takes 32 passes -
    next to 512 chunks of 512 bytes"""
    big = ec.Chunk([H] * 4, (2048, 128), em.PIXELS, [3, 2, 1, 0], few=True, seed=5)
    assert big.n == 2 << 20 and len(big.stored) < big.n
    small = [ec.Chunk([H], (256, 1), few=True, seed=600 + k) for k in range(512)]
    run(torch, dec, [small[0], big] + small[1:], seed=4)


@pytest.mark.parametrize("tile,order", [((32, 32), "RGBA"), ((64, 64), None), (None, "RGBA")])
def test_one_image_into_one_buffer(torch, dec, tile, order):
    """3 x 3 tiles with narrower edge tiles, and scanline chunks with a short
    last one, through exr.parse().rows() into one H x W x C buffer"""
    from libdeflate_amd import binding, exr
    channels = [("A", exr.HALF), ("B", exr.HALF), ("G", exr.HALF), ("R", exr.HALF)]
    width, height = (3 * tile[0] - 11, 2 * tile[1] + 5) if tile else (75, 37)
    data, planes = ec.image_file(width, height, channels, exr.ZIP, tile, seed=[8, width])
    im = exr.parse(data)
    assert len(im.chunks) == (9 if tile else 3)
    rows = im.rows(offset=5, layout=binding.EXR_PIXELS, order=order)
    pixels = ec.interleaved(planes, [3, 2, 1, 0] if order else None).tobytes()
    total = 5 + len(pixels)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((len(rows) + 1,), UNSET, dtype=torch.int32, device="cuda")
    dec.decode_exr_batch(rows, d_in, whole[GUARD:], per, out_avail=total)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [SUCCESS] * len(rows) + [UNSET]
    host = whole.cpu().numpy()
    assert host[GUARD + 5:GUARD + total].tobytes() == pixels
    assert (host[:GUARD + 5] == CANARY).all() and (host[GUARD + total:] == CANARY).all()


def test_fixture_files_decode_to_their_pixels(torch, dec):
    """every file of tests/golden/exr in one batch (files of this project's own
    builder: they pin parser, model and kernels against each other)"""
    from libdeflate_amd import binding, exr
    files = ec.fixtures()
    assert len(files) >= 6
    blob, rows, at, spans = bytearray(), [], 0, []
    for name, data, pixels in files:
        im = exr.parse(data)
        at += 3
        r = im.rows(offset=at, layout=binding.EXR_PIXELS)
        r[:, 0] += np.uint64(len(blob) + 1)
        rows.append(r)
        spans.append((at, pixels.tobytes()))
        blob += b"\x00" + data
        at += pixels.size
    rows = np.concatenate(rows)
    d_in = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    whole = torch.full((GUARD + at + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((len(rows) + 1,), UNSET, dtype=torch.int32, device="cuda")
    dec.decode_exr_batch(rows, d_in, whole[GUARD:], per, out_avail=at)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [SUCCESS] * len(rows) + [UNSET]
    want = np.full(GUARD + at + GUARD, CANARY, dtype=np.uint8)
    for a, pixels in spans:
        want[GUARD + a:GUARD + a + len(pixels)] = np.frombuffer(pixels, dtype=np.uint8)
    assert (whole.cpu().numpy() == want).all()


def _defects():
    """(name, chunk) of every failure; the expected code is the oracle's for the
    stored bytes with out_nbytes_avail = n and no actual_out"""
    oracle = oracle_util.load_oracle()

    def base(seed):
        c = ec.Chunk([H] * 4, (61, 9), em.PIXELS, [3, 2, 1, 0], extra=5, few=True, seed=seed)
        assert len(c.stored) < c.n - 16
        return c
    out = []
    c = base(1)
    c.stored = c.stored[:-7]
    out.append(("truncated", c, BAD_DATA))
    c = base(2)
    c.stored = zlib.compress(em.apply(c.raw)[:-1], 6)
    out.append(("short", c, SHORT_OUTPUT))
    c = base(3)
    c.stored = zlib.compress(em.apply(c.raw) + b"\x00", 6)
    out.append(("long", c, INSUFFICIENT_SPACE))
    c = base(4)
    z = bytearray(c.stored)
    z[-1] ^= 0x10
    c.stored = bytes(z)
    out.append(("adler", c, BAD_DATA))
    c = ec.Chunk([F], (300, 2), few=True, seed=5)       # ... and a direct row
    z = bytearray(c.stored)
    z[-2] ^= 0x01
    c.stored = bytes(z)
    out.append(("adler-direct", c, BAD_DATA))
    for name, c, code in out:
        assert len(c.stored) < c.n
        c.want, c.room = oracle.decompress_ex("zlib", c.stored, c.n, want_actual_out=False)[0], "any"
        assert c.want == code, name
    c = base(6)
    c.stored = ec.random_bytes(6, c.n + 1)      # dataSize > n: the call's own verdict, nothing written
    c.want, c.room = BAD_DATA, "canary"
    out.append(("oversize", c, BAD_DATA))
    return [(name, c) for name, c, _ in out]


def test_failures_leave_their_neighbours_intact(torch, dec):
    good = [ec.Chunk([H] * 3, (50, 11), em.PIXELS, [2, 1, 0], extra=3, few=True, seed=20),
            ec.Chunk([H], (301, 3), few=True, seed=21), ec.Chunk([F], (53, 6), extra=1, seed=22),
            ec.Chunk([H] * 4 + [F], (9, 16), em.PIXELS, [3, 2, 1, 0, 4], few=True, seed=23),
            ec.Chunk([H] * 5, (77, 2), em.PIXELS, None, few=True, seed=24)]
    defects = _defects()
    chunks = []
    for k, (name, c) in enumerate(defects):
        chunks += [good[k % len(good)], c, good[(k + 3) % len(good)]]
    run(torch, dec, chunks, seed=6)
    # each first and last of a batch
    for name, c in defects:
        run(torch, dec, [c, good[0], c], seed=7)


def test_two_calls_queued_on_a_side_stream(torch, dec, edge_chunks):
    """a non-default stream, and two calls on one object without a
    synchronisation between them: the second call's plan and scratch follow the
    first's in stream order"""
    st = torch.cuda.Stream()
    check_a = run(torch, dec, edge_chunks[::5], seed=9, stream=st, sync=False)
    check_b = run(torch, dec, edge_chunks[2::7], seed=10, stream=st, sync=False)
    st.synchronize()
    check_a()
    check_b()


def test_nothing_to_do(torch, dec):
    from libdeflate_amd import binding
    out = torch.full((16,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((1,), UNSET, dtype=torch.int32, device="cuda")
    dec.decode_exr_batch(np.zeros((0, binding.EXR_WORDS), dtype=np.uint64), out, out, per)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [UNSET] and (out.cpu().numpy() == CANARY).all()
