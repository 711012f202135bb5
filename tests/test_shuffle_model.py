"""The CPU model of the byte shuffle of HDF5, NetCDF-4 and Zarr chunks
(tools/models/shuffle_model.py), the oracle of the GPU tests: the two
hand-checked vectors of the interface's description, the identity cases, the
round trip for every small size and element size, and the numpy form against a
plain double loop.  No GPU."""
import random

import pytest

from tools.models import shuffle_model as sm


def _loop(raw, es):
    """the transform as the header states it"""
    n = len(raw)
    ne, out = n // es, bytearray(n)
    for j in range(es):
        for k in range(ne):
            out[j * ne + k] = raw[k * es + j]
    for t in range(n % es):
        out[es * ne + t] = raw[es * ne + t]
    return bytes(out)


def test_the_two_vectors():
    assert list(sm.shuffle(bytes(range(10)), 4)) == [0, 4, 1, 5, 2, 6, 3, 7, 8, 9]
    assert list(sm.shuffle(bytes(range(7)), 3)) == [0, 3, 1, 4, 2, 5, 6]
    assert sm.unshuffle(bytes([0, 4, 1, 5, 2, 6, 3, 7, 8, 9]), 4) == bytes(range(10))
    assert sm.unshuffle(bytes([0, 3, 1, 4, 2, 5, 6]), 3) == bytes(range(7))


def test_identity_for_es_1_and_at_most_one_element():
    rng = random.Random(1)
    for n in range(0, 40):
        raw = bytes(rng.randrange(256) for _ in range(n))
        assert sm.shuffle(raw, 1) == raw == sm.unshuffle(raw, 1)
        assert sm.identity(n, 1)
        for es in range(1, 20):
            if n // es <= 1:
                assert sm.identity(n, es)
                assert sm.shuffle(raw, es) == raw == sm.unshuffle(raw, es)
    assert not sm.identity(4, 2) and sm.identity(4, 2, sm.NO_SHUFFLE) and sm.identity(3, 2)


def test_round_trip_and_the_double_loop():
    rng = random.Random(2)
    for n in range(0, 71):
        raw = bytes(rng.randrange(256) for _ in range(n))
        for es in range(1, 18):
            sh = sm.shuffle(raw, es)
            assert sh == _loop(raw, es)
            assert sm.unshuffle(sh, es) == raw


def test_tiles_rows_and_bound():
    assert [sm.tile_elems(es) for es in (1, 2, 4, 8)] == [4096] * 4
    assert [sm.tile_elems(es) for es in (3, 5, 16, 255, 256)] == [5456, 3264, 1024, 64, 64]
    for es in range(1, 257):
        t = sm.tile_elems(es)
        assert t % 16 == 0 and t >= 64
        # the staging area of the kernels' generic path: es planes of t + 16 bytes
        assert es in (1, 2, 4, 8) or es * (t + 16) <= 20480
        assert sm.tiles(0, es) == 0 and sm.tiles(es, es) == 1
        assert sm.tiles(t * es + es - 1, es) == 1 and sm.tiles((t + 1) * es, es) == 2
    r = sm.rows([0, 40], [40, 7], [4, 3], [5, 9], [11, 7], [0, sm.NO_DEFLATE])
    assert r.tolist() == [[5, 11, 0, 40, 4, 0], [9, 7, 40, 7, 3, 1]]
    assert [sm.classify(x) for x in r] == [sm.DECODE_UNSHUFFLE, sm.STORED_UNSHUFFLE]
    assert sm.bound("zlib", r[:1]) == 40 + 5 + 6 and sm.bound("gzip", r[:1]) == 40 + 5 + 18
    assert sm.bound("deflate", r) == 0      # NO_DEFLATE is no writer's mask
    assert sm.stream_bound("deflate", 5001) == 5001 + 10


@pytest.mark.parametrize("mask,n,es,want", [
    (0, 8, 1, sm.DECODE_DIRECT), (0, 7, 4, sm.DECODE_DIRECT), (2, 80, 4, sm.DECODE_DIRECT),
    (0, 8, 4, sm.DECODE_UNSHUFFLE), (1, 8, 4, sm.STORED_UNSHUFFLE), (3, 8, 4, sm.STORED_COPY),
    (1, 4, 4, sm.STORED_COPY), (1, 0, 4, sm.STORED_EMPTY)])
def test_classification(mask, n, es, want):
    assert sm.classify([0, n, 0, n, es, mask]) == want
    if mask & 1:
        assert sm.classify([0, n + 1, 0, n, es, mask]) == sm.STORED_BAD
