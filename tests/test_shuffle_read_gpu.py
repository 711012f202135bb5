"""Byte-shuffled deflate chunks (HDF5, NetCDF-4, Zarr) read on the GPU
(libdeflate_amd_shuffle_decompress_batch).  No tolerance anywhere: every result
and every byte of every room equal what Python's zlib and the CPU model
(tools/models/shuffle_model.py) state, and the canary bytes in front of d_out,
in every gap between rooms and behind out_avail stay untouched.  The stored
chunks are packed at unaligned offsets with junk between them, the rooms at
unaligned offsets too, and out_avail is exactly the end of the last room.  The
shapes aim at the kernels' tiles: for every element size es, T =
sm.tile_elems(es) elements."""
import random
import zlib

import numpy as np
import pytest

from tests.shuffle_chunks import raw_bytes, shapes
from tools.models import shuffle_model as sm

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
CANARY = 0xA5
UNSET = -7      # d_results where nothing was written
GUARD = 64
WBITS = {"deflate": -15, "zlib": 15, "gzip": 31}


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


def _compress(fmt, data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt])
    return c.compress(data) + c.flush()


class Chunk:
    """raw: the chunk's bytes; stored: what the file holds; stored_n, raw_n: words
    1 and 3 where a test lies about them; want: the result; room: 'raw' (the
    room holds raw), 'any' (undefined) or 'canary' (not written)"""

    def __init__(self, fmt, es, n, mask=0, level=6):
        self.es, self.mask, self.raw = es, mask, raw_bytes(es, n)
        self.stored = sm.stored(self.raw, es, mask, lambda b: _compress(fmt, b, level))
        self.raw_n, self.want, self.room = n, SUCCESS, "raw"


def run(torch, dec, fmt, chunks, seed=0, stream=None, sync=True):
    """one call over the chunks -> a closure that checks everything (called at
    once unless sync is False)"""
    rng = random.Random(seed)
    buf, rows, at = bytearray(), [], 0
    for c in chunks:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 8)))
        at += rng.randrange(0, 4)       # a gap of canary bytes in front of the room
        rows.append([len(buf), len(c.stored), at, c.raw_n, c.es, c.mask])
        buf += c.stored
        at += c.raw_n
    buf += b"\x78\x9c" * 5              # behind the last chunk: never read as part of it
    total = at
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((len(chunks) + 1,), UNSET, dtype=torch.int32, device="cuda")
    if stream is not None:      # the uploads are the current stream's work
        stream.wait_stream(torch.cuda.current_stream())
    got_rows = dec.decompress_shuffle_batch(fmt, rows, d_in, whole[GUARD:], per, stream=stream,
                                            out_avail=total)
    assert got_rows.tolist() == rows

    def check():
        host = whole.cpu().numpy()
        assert not (host[:GUARD] != CANARY).any(), "bytes written in front of d_out"
        assert not (host[GUARD + total:] != CANARY).any(), "bytes written past out_avail"
        host = host[GUARD:GUARD + total]
        res = per.cpu().numpy()
        assert res[len(chunks)] == UNSET
        want = np.full(total, CANARY, dtype=np.uint8)
        defined = np.ones(total, dtype=bool)
        for c, r in zip(chunks, rows):
            if c.room == "raw":
                want[r[2]:r[2] + r[3]] = np.frombuffer(c.raw, dtype=np.uint8)
            elif c.room == "any":
                defined[r[2]:r[2] + r[3]] = False
        assert res[:len(chunks)].tolist() == [c.want for c in chunks]
        bad = np.nonzero((host != want) & defined)[0]
        if bad.size:
            k = max(i for i, r in enumerate(rows) if r[2] <= bad[0])
            raise AssertionError("first wrong byte at %d of %d: chunk %d (es %d, n %d, mask %d) "
                                 "byte %d" % (bad[0], total, k, chunks[k].es, rows[k][3],
                                              chunks[k].mask, bad[0] - rows[k][2]))
        return host, rows, bytes(buf)
    if not sync:
        return check
    torch.cuda.synchronize()
    return check()


@pytest.mark.parametrize("fmt", ["deflate", "zlib", "gzip"])
def test_all_shapes_mixed_in_one_batch(torch, dec, fmt):
    chunks = [Chunk(fmt, es, n) for es, n in shapes()]
    random.Random(3).shuffle(chunks)
    run(torch, dec, fmt, chunks, seed=1)


@pytest.mark.parametrize("mask", [sm.NO_DEFLATE, sm.NO_SHUFFLE, sm.NO_DEFLATE | sm.NO_SHUFFLE])
def test_masks(torch, dec, mask):
    """the stored bytes are the shuffled bytes; the shuffle was skipped; both -
    every third chunk keeps mask 0, so that all four classes of row meet"""
    chunks = [Chunk("zlib", es, n, 0 if k % 3 == 2 else mask) for k, (es, n) in enumerate(shapes())]
    random.Random(4).shuffle(chunks)
    run(torch, dec, "zlib", chunks, seed=2)


def test_identity_batch_is_decompress_batch(torch, dec):
    """a batch that is the identity throughout, byte for byte against
    libdeflate_amd_decompress_batch on the same streams and rooms"""
    chunks = [Chunk("gzip", es, n, mask) for es, n, mask in
              [(1, 0, 0), (1, 1, 0), (1, 70001, 0), (4, 7, 0), (256, 511, 0), (8, 8, 0),
               (4, 40000, sm.NO_SHUFFLE), (3, 3001, sm.NO_SHUFFLE), (16, 0, 0)]]
    for c in chunks:
        assert sm.classify([0, len(c.stored), 0, c.raw_n, c.es, c.mask]) == sm.DECODE_DIRECT
    host, rows, buf = run(torch, dec, "gzip", chunks, seed=5)
    # the same bytes and rooms through the plain batch call
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    r = np.array(rows, dtype=np.int64)
    cols = [torch.tensor(r[:, w].tolist(), dtype=torch.int64, device="cuda") for w in range(4)]
    total = int(r[-1, 2] + r[-1, 3])
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((len(chunks),), UNSET, dtype=torch.int32, device="cuda")
    dec.decompress_batch("gzip", d_in, cols[0], cols[1], out, cols[2], cols[3], per)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [SUCCESS] * len(chunks)
    assert (out.cpu().numpy() == host).all()


def _defects(fmt):
    """(name, chunk) of every failure, built on a chunk of two tiles and a tail"""
    es, n = 4, (2 * sm.tile_elems(4) + 1) * 4 + 3
    out = []
    for name in ("footer", "header"):
        c = Chunk(fmt, es, n)
        s = bytearray(c.stored)
        s[-1 if name == "footer" else 0] ^= 0x10
        c.stored, c.want, c.room = bytes(s), BAD_DATA, "any"
        out.append((name, c))
    c = Chunk(fmt, es, n - 1)           # the stream ends one byte short of the raw size
    c.raw_n, c.want, c.room = n, SHORT_OUTPUT, "any"
    out.append(("short", c))
    c = Chunk(fmt, es, n + 1)           # ... and one byte long
    c.raw_n, c.want, c.room = n, INSUFFICIENT_SPACE, "any"
    out.append(("long", c))
    for d in (-1, 1):                   # a NO_DEFLATE row whose two sizes differ
        c = Chunk(fmt, es, n + d, sm.NO_DEFLATE)
        c.raw_n, c.want, c.room = n, BAD_DATA, "canary"
        out.append(("stored%+d" % d, c))
    return out


@pytest.mark.parametrize("fmt", ["zlib", "gzip"])
def test_failures_leave_their_neighbours_intact(torch, dec, fmt):
    good = [Chunk(fmt, es, n, mask) for es, n, mask in
            [(4, 4 * 4097 + 1, 0), (3, 3 * 100 + 2, 0), (8, 8 * 33, sm.NO_DEFLATE), (1, 50, 0),
             (2, 2 * 17 + 1, 0), (16, 16 * 1025, 0), (5, 5 * 3265 + 4, sm.NO_DEFLATE)]]
    chunks = []
    for k, (name, c) in enumerate(_defects(fmt)):
        chunks += [good[k % len(good)], c, good[(k + 3) % len(good)]]
    run(torch, dec, fmt, chunks, seed=6)
    # each alone between two neighbours, and first and last of a batch
    for name, c in _defects(fmt):
        run(torch, dec, fmt, [c, good[0], c], seed=7)


def test_raw_deflate_failures(torch, dec):
    """without a checksum: the two length failures and the unequal stored sizes"""
    chunks = [c for name, c in _defects("deflate") if name not in ("footer", "header")]
    run(torch, dec, "deflate", [Chunk("deflate", 2, 9001)] + chunks + [Chunk("deflate", 8, 8 * 4097)],
        seed=8)


def test_two_calls_queued_on_a_side_stream(torch, dec):
    """a non-default stream, and two calls on one object without a
    synchronisation between them: the second call's plan and scratch follow the
    first's in stream order"""
    s = torch.cuda.Stream()
    a = [Chunk("zlib", es, n) for es, n in shapes()[::3]]
    b = [Chunk("zlib", es, n, k % 4) for k, (es, n) in enumerate(shapes()[1::2])]
    check_a = run(torch, dec, "zlib", a, seed=9, stream=s, sync=False)
    check_b = run(torch, dec, "zlib", b, seed=10, stream=s, sync=False)
    s.synchronize()
    check_a()
    check_b()


def test_nothing_to_do(torch, dec):
    from libdeflate_amd import binding
    out = torch.full((16,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((1,), UNSET, dtype=torch.int32, device="cuda")
    dec.decompress_shuffle_batch("zlib", np.zeros((0, binding.SHUF_WORDS), dtype=np.uint64), out, out,
                                 per)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [UNSET] and (out.cpu().numpy() == CANARY).all()
