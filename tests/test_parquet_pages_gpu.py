"""Hand-built Parquet pages (tests/parquet_pages.py) through
libdeflate_amd_parquet_decode_batch at the smallest shapes where the kernels can
go wrong: slot counts around the expand tile and the pieces of a level run,
every index bit width that changes how bits straddle bytes, the run shapes, the
places of nulls, the value widths and the page forms.  No tolerance: results,
slot bytes and validity bytes equal the CPU model's, canaries hold, page bodies
lie at unaligned offsets with junk between them and slots at unaligned offsets
with gaps (tests/parquet_pages.py: lay_out, run_gpu)."""
import random

import numpy as np
import pytest

from tests import parquet_pages as pp
from tools.models import parquet_model as pm

pytestmark = pytest.mark.gpu

T = pm.TILE
COUNTS = [1, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]


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


def entries_of(rng, e, width):
    """e distinct entries of `width` bytes: the entry's number, then random bytes"""
    a = np.frombuffer(bytes(rng.randrange(256) for _ in range(e * width)), dtype=np.uint8)
    a = a.reshape(e, width).copy()
    for k in range(min(width, 4)):
        a[:, k] = (np.arange(e) >> (8 * k)) & 255
    return a


def mask_of(rng, n, share=0.2):
    return [int(rng.random() >= share) for _ in range(n)]


def go(torch, dec, pages, seed=0, fmt="gzip"):
    buf, rows, out_n, valid_n = pp.lay_out(pages, random.Random(seed))
    return pp.run_gpu(torch, dec, buf, rows, fmt, out_n, valid_n, [0] * len(pages))


def test_slot_counts_around_the_tile(torch, dec):
    rng = random.Random(1)
    entries = entries_of(rng, 300, 4)
    d = pp.dict_page(entries)
    pages = [d]
    for k, n in enumerate(COUNTS):
        v = 1 + k % 2
        pages.append(pp.data_page(rng, v, 4, n=n)[0])
        pages.append(pp.data_page(rng, 3 - v, 8, mask=mask_of(rng, n))[0])
        pages.append(pp.data_page(rng, v, 4, mask=mask_of(rng, n), dictionary=d, entries=entries,
                                  shape="alt", level_shape="alt")[0])
        pages.append(pp.data_page(rng, 3 - v, 4, n=n, dictionary=d, entries=entries)[0])
    go(torch, dec, pages)


def test_many_one_value_pages_in_a_tile(torch, dec):
    """a tile of the expand kernel spans hundreds of pages"""
    rng = random.Random(2)
    entries = entries_of(rng, 5, 4)
    d = pp.dict_page(entries, compress=False)
    pages = [d]
    for k in range(1500):
        kind = k % 4
        if kind == 0:
            pages.append(pp.data_page(rng, 1, 4, n=1, compress=False)[0])
        elif kind == 1:
            pages.append(pp.data_page(rng, 2, 4, mask=[k // 4 % 2], compress=k % 40 == 1)[0])
        elif kind == 2:
            pages.append(pp.data_page(rng, 1, 4, mask=[1], dictionary=d, entries=entries,
                                      compress=k % 40 == 2)[0])
        else:
            pages.append(pp.data_page(rng, 2, 4, n=1, dictionary=d, entries=entries, compress=False)[0])
    go(torch, dec, pages)


@pytest.mark.parametrize("w", [0, 1, 7, 8, 9, 16, 17, 31, 32])
def test_index_bit_widths(torch, dec, w):
    rng = random.Random(100 + w)
    e = 1 if w == 0 else 70000 if w >= 17 else 1 << w
    entries = entries_of(rng, e, 4)
    d = pp.dict_page(entries)
    pages = [d]
    for shape in ("bp", "alt", "rle1", "rle"):
        for hdr in (None, 2, 5):
            n = rng.choice([1, 9, 300, 505, 1100])
            idx = [rng.choice([0, e - 1, rng.randrange(e)]) for _ in range(n)]
            if shape == "rle":
                idx = sorted(idx)
            pages.append(pp.data_page(rng, 1 + len(pages) % 2, 4, n=n, dictionary=d, entries=entries, w=w,
                                      shape=shape, hdr=hdr, indices=idx)[0])
            m = mask_of(rng, n)
            pages.append(pp.data_page(rng, 1 + len(pages) % 2, 4, mask=m, dictionary=d, entries=entries,
                                      w=w, shape=shape, level_shape=shape, hdr=hdr)[0])
    go(torch, dec, pages, seed=w)


def test_run_shapes(torch, dec):
    rng = random.Random(3)
    entries = entries_of(rng, 9, 8)
    d = pp.dict_page(entries)
    pages = [d]
    n = 2 * T + 3
    # one RLE run for the whole page, levels and indices
    pages.append(pp.data_page(rng, 1, 8, mask=[1] * n, dictionary=d, entries=entries, indices=[4] * n,
                              shape="rle", level_shape="rle")[0])
    assert len(pages[-1].stored) < 200
    # RLE runs of 1
    pages.append(pp.data_page(rng, 2, 8, mask=mask_of(rng, 700, 0.5), dictionary=d, entries=entries,
                              shape="rle1", level_shape="rle1")[0])
    # a last bit-packed group padded past N: one run of all groups, and pyarrow's runs of 63 groups
    for n2 in (T + 1, 3 * 504 + 5):
        pages.append(pp.data_page(rng, 1, 8, mask=mask_of(rng, n2), dictionary=d, entries=entries)[0])
        m = mask_of(rng, n2)
        pages.append(pp.data_page(rng, 2, 8, mask=m, dictionary=d, entries=entries,
                                  level_runs=pp.runs_of(m, 1, "bp", rng, group_max=1 << 20))[0])
    # a run boundary on a tile boundary and one slot either side; level runs and
    # index runs cut at different places
    for cut in (T - 1, T, T + 1):
        lev = [("rle", 1, cut), ("rle", 0, 2), ("rle", 1, T + 5)]
        nv = cut + T + 5
        ind = [("rle", 3, T - 7), ("rle", 8, nv - (T - 7) - 16), ("bp", [2] * 16)]
        mask = [1] * cut + [0] * 2 + [1] * (T + 5)
        idx = [3] * (T - 7) + [8] * (nv - (T - 7) - 16) + [2] * 16
        pages.append(pp.data_page(rng, 1, 8, mask=mask, dictionary=d, entries=entries, indices=idx,
                                  level_runs=lev, index_runs=ind, w=4)[0])
        # the same boundary between two bit-packed level runs (cut a multiple of 8 only)
        if cut % 8 == 0:
            m = mask_of(rng, 2 * cut)
            runs = [("bp", m[:cut]), ("bp", m[cut:])]
            pages.append(pp.data_page(rng, 2, 8, mask=m, level_runs=runs)[0])
    # a level run of more than 64 pieces
    m = mask_of(rng, 70 * pm.LEVEL_PIECE + 8, 0.5)
    pages.append(pp.data_page(rng, 1, 4, mask=m, level_runs=[("bp", m)], compress=False)[0])
    go(torch, dec, pages)


def test_nulls(torch, dec):
    rng = random.Random(4)
    entries = entries_of(rng, 17, 4)
    d = pp.dict_page(entries)
    pages = [d]
    for n in (5, T, 2 * T + 3):
        edge = [1] * n
        for k in (0, T - 1, T, n - 1):
            if k < n:
                edge[k] = 0
        for mask in ([1] * n, [0] * n, edge, [1 - x for x in edge]):
            for v in (1, 2):
                pages.append(pp.data_page(rng, v, 4, mask=mask)[0])
                pages.append(pp.data_page(rng, v, 4, mask=mask, dictionary=d, entries=entries,
                                          level_shape="alt")[0])
    # all null: the values section is empty
    assert any(p.enc and p.usize - p.def_len == 0 for p in pages if p.kind == pm.DATA_V2)
    go(torch, dec, pages)


@pytest.mark.parametrize("width", [1, 4, 5, 8, 12, 16, 33, 256])
def test_value_widths(torch, dec, width):
    rng = random.Random(width)
    entries = entries_of(rng, 21, width)
    d = pp.dict_page(entries)
    pages = [d]
    for n in (1, 70, 260):
        pages.append(pp.data_page(rng, 1, width, n=n)[0])
        pages.append(pp.data_page(rng, 2, width, mask=mask_of(rng, n))[0])
        pages.append(pp.data_page(rng, 2, width, mask=mask_of(rng, n), dictionary=d, entries=entries)[0])
    go(torch, dec, pages, seed=width)


@pytest.mark.parametrize("fmt", ["gzip", "zlib", "deflate"])
def test_page_forms(torch, dec, fmt):
    rng = random.Random(6)
    e1, e2 = entries_of(rng, 40, 4), entries_of(rng, 3, 4)
    pages = []
    for entries, packed in ((e1, True), (e2, False)):    # two chunks, each with its own dictionary
        d = pp.dict_page(entries, compress=packed, fmt=fmt)
        pages.append(d)
        for v in (1, 2):
            for compress in (True, False):
                pages.append(pp.data_page(rng, v, 4, mask=mask_of(rng, 333), dictionary=d, entries=entries,
                                          compress=compress, fmt=fmt)[0])
                pages.append(pp.data_page(rng, v, 4, mask=mask_of(rng, 90), compress=compress, fmt=fmt)[0])
                pages.append(pp.data_page(rng, v, 4, n=90, compress=compress, fmt=fmt)[0])
    go(torch, dec, pages, fmt=fmt)
