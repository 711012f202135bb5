"""Hand-built BYTE_ARRAY pages (tests/parquet_string_pages.py) through
libdeflate_amd_parquet_decode_batch_ex at the smallest shapes where its kernels
can go wrong: value starts around the edge of the walk's 1 KiB window, runs of
empty strings around 256, a string longer than the window, slot counts around
the tile of 1024, tiles that span hundreds of pages, nulls at the tiles' ends,
dictionaries of one, an empty and 300 entries, strings across the copy's 4 KiB
tiles, and every verdict with good neighbours.  No tolerance: results, the
total, offsets, bytes and validity equal the CPU model's, canaries hold."""
import random

import numpy as np
import pytest

from tests import parquet_pages as pp
from tests import parquet_string_pages as sp
from tools.models import parquet_model as pm
from tools.models import parquet_strings_model as sm

pytestmark = pytest.mark.gpu

T = pm.TILE


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


def go(torch, dec, pages, seed=0, fmt="gzip", want=None, **kw):
    buf, rows, out_n, valid_n = sp.lay_out(pages, random.Random(seed))
    m = sp.run_gpu(torch, dec, buf, rows, fmt, out_n, valid_n,
                   want_results=[0] * len(pages) if want is None else want, **kw)
    return m, rows


def words(rng, n, lo=0, hi=12):
    return [bytes(rng.randrange(256) for _ in range(rng.randrange(lo, hi + 1))) for _ in range(n)]


def with_nulls(rng, vals, share=0.2):
    return [None if rng.random() < share else v for v in vals]


# ---- the walk ----

@pytest.mark.parametrize("edge", range(1020, 1029))
def test_a_value_starts_around_the_window_edge(torch, dec, edge):
    """the second value's prefix at 1020 .. 1028 of the section: it straddles
    the window's end, or opens the next window"""
    rng = random.Random(edge)
    vals = [bytes(rng.randrange(256) for _ in range(edge - 4)), b"second", b"", b"x" * 40]
    assert len(sp.section_of(vals[:1])) == edge
    m, rows = go(torch, dec, [sp.data_page(rng, 1, vals, required=True),
                              sp.dict_page(vals), sp.data_page(rng, 2, vals, compress=False)], edge)
    assert sp.strings_of(m, rows[0], 4) == vals == sp.strings_of(m, rows[2], 4)


@pytest.mark.parametrize("n", [255, 256, 257, 600])
def test_empty_strings_in_a_row(torch, dec, n):
    rng = random.Random(n)
    vals = [b"a"] + [b""] * n + [b"tail"]
    m, rows = go(torch, dec, [sp.data_page(rng, 1, vals, required=True),
                              sp.data_page(rng, 2, [b""] * n, required=True)], n)
    assert sp.strings_of(m, rows[0], n + 2) == vals and m["total"] == 5


def test_a_string_longer_than_the_window_and_sections_that_end_with_their_last_byte(torch, dec):
    rng = random.Random(3)
    long = bytes(rng.randrange(256) for _ in range(3000))
    vals = [b"a", b"b", long, b"c", b"d"]
    one = sp.data_page(rng, 1, [b"only"], required=True, compress=False)
    pages = [sp.data_page(rng, 1, vals, required=True), one,
             sp.data_page(rng, 2, with_nulls(rng, vals * 3)), sp.dict_page([long]),
             sp.data_page(rng, 1, [b""], required=True)]
    assert one.stored == sp.section_of([b"only"])       # nothing behind the last value's last byte
    m, rows = go(torch, dec, pages, 3)
    assert sp.strings_of(m, rows[0], 5) == vals and sp.strings_of(m, rows[1], 1) == [b"only"]


# ---- the slots ----

@pytest.mark.parametrize("n", [1, T - 1, T, T + 1])
def test_slot_counts_around_the_tile(torch, dec, n):
    rng = random.Random(n)
    entries = words(rng, 7, 1, 9)
    d = sp.dict_page(entries)
    pages = [d, sp.data_page(rng, 1, with_nulls(rng, words(rng, n))),
             sp.data_page(rng, 2, [entries[rng.randrange(7)] for _ in range(n)], d, required=True),
             sp.data_page(rng, 1, with_nulls(rng, [entries[rng.randrange(7)] for _ in range(n)]), d,
                          shape="alt", level_shape="alt")]
    go(torch, dec, pages, n)


def test_300_pages_of_one_value(torch, dec):
    rng = random.Random(300)
    d = sp.dict_page([b"zero", b"", b"two"])
    pages = [d]
    for k in range(300):
        v = [None if k % 7 == 3 else bytes([65 + k % 26]) * (k % 5)]
        pages.append(sp.data_page(rng, 1 + k % 2, v, compress=k % 3 == 0) if k % 4 else
                     sp.data_page(rng, 1, [b"two"], d, compress=False))
    m, _ = go(torch, dec, pages, 300)
    assert m["total"] == sum(3 if k % 4 == 0 else 0 if k % 7 == 3 else k % 5 for k in range(300))


@pytest.mark.parametrize("nulls", ["none", "all", "ends"])
def test_nulls_nowhere_everywhere_and_at_both_ends_of_a_tile(torch, dec, nulls):
    rng = random.Random(len(nulls))
    vals = words(rng, 2 * T + 5, 0, 6)
    if nulls == "all":
        vals = [None] * len(vals)
    elif nulls == "ends":
        for k in (0, T - 1, T, 2 * T - 1, 2 * T, len(vals) - 1):
            vals[k] = None
    m, _ = go(torch, dec, [sp.data_page(rng, 1, vals, level_shape="rle"),
                           sp.data_page(rng, 2, vals[:T + 1])], 9)
    assert nulls != "all" or m["total"] == 0


# ---- the dictionaries ----

def test_dictionaries(torch, dec):
    """one entry and index width 0, an empty entry, 300 entries, a dictionary
    shared by two data pages, a PLAIN page behind a dictionary-coded one"""
    rng = random.Random(11)
    one, big = sp.dict_page([b"the only one"]), sp.dict_page([b""] + words(rng, 299, 1, 20))
    pick = [big.entries[rng.randrange(300)] for _ in range(700)]
    pages = [one, big,
             sp.data_page(rng, 1, with_nulls(rng, [b"the only one"] * 70), one, w=0),
             sp.data_page(rng, 2, pick, big, required=True),
             sp.data_page(rng, 1, with_nulls(rng, pick[:99] + [b""] * 30), big, shape="alt"),
             sp.data_page(rng, 1, with_nulls(rng, words(rng, 50)))]
    m, rows = go(torch, dec, pages, 11)
    assert sp.strings_of(m, rows[3], 700) == pick


# ---- the copy ----

def test_strings_across_copy_tiles_and_a_total_of_zero(torch, dec):
    rng = random.Random(12)
    a = bytes(rng.randrange(256) for _ in range(4096 - 7))
    b = bytes(rng.randrange(256) for _ in range(2 * 4096 + 100))   # spans three tiles
    vals = [b"seven77", a, b"x", b, b"", b"tail"]                   # a ends on a tile's edge
    m, rows = go(torch, dec, [sp.data_page(rng, 1, vals, required=True)], 12)
    assert sp.strings_of(m, rows[0], 6) == vals
    m, _ = go(torch, dec, [sp.data_page(rng, 1, [b"", None, b""]), sp.dict_page([b"unused"])], 13)
    assert m["total"] == 0


# ---- the call's shape ----

@pytest.mark.parametrize("fmt", ["gzip", "zlib", "deflate"])
def test_two_string_columns_and_an_int64_column(torch, dec, fmt):
    """V1 and V2, compressed and not, in every format; the fixed-width pages
    between the string pages take no room in d_bytes"""
    rng = random.Random(len(fmt))
    ents = np.frombuffer(bytes(rng.randrange(256) for _ in range(40 * 8)), np.uint8).reshape(40, 8)
    di = pp.dict_page(ents, fmt=fmt)
    ds = sp.dict_page(words(rng, 20, 0, 30), fmt=fmt, compress=False)
    pages = [ds, di]
    for k in range(4):
        v, c = 1 + k % 2, k < 2
        pages.append(sp.data_page(rng, v, with_nulls(rng, words(rng, 300 + k)), compress=c, fmt=fmt))
        pages.append(pp.data_page(rng, v, 8, [int(rng.random() < 0.8) for _ in range(200 + k)], di,
                                  ents, compress=not c, fmt=fmt)[0])
        pages.append(sp.data_page(rng, 3 - v, [ds.entries[rng.randrange(20)] for _ in range(500)], ds,
                                  required=True, compress=c, fmt=fmt))
    go(torch, dec, pages, 21, fmt)


# ---- the verdicts: one bad page among good neighbours ----

def bad_pages(rng):
    """{name: (the page - or pages, the bad one last -, its verdict)}"""
    vals = words(rng, 40, 1, 9)
    sec = sp.section_of(vals)
    leaves = sp.section_of(vals[:20]) + (10 ** 6).to_bytes(4, "little") + b"abc"
    short = sp.dict_page(vals, section=sec, count=41)
    d = sp.dict_page(vals)
    return {
        "a length that leaves the section": (sp.data_page(rng, 1, vals[:21], required=True, section=leaves),),
        "a section that ends inside a prefix": (sp.data_page(rng, 2, vals, required=True, section=sec + b"\x01\x00"),
                                                ),
        "one value too few": (sp.data_page(rng, 1, vals + [b"more"], section=sec),),
        "a dictionary one entry short": (short, sp.data_page(rng, 1, vals[:5], short, indices=[0, 1, 2, 3, 4])),
        "an index equal to the entry count": (d, sp.data_page(rng, 1, vals[:3], d, indices=[1, 40, 2], w=6,
                                                              required=True)),
    }


@pytest.mark.parametrize("name", ["a length that leaves the section", "a section that ends inside a prefix",
                                  "one value too few", "a dictionary one entry short",
                                  "an index equal to the entry count"])
def test_one_bad_page_among_good_neighbours(torch, dec, name):
    rng = random.Random(len(name))
    bad = bad_pages(rng)[name]
    if name == "a section that ends inside a prefix":
        # 40 values and two bytes of a 41st prefix: 41 values are owed
        bad[0].count = 41
    before = [sp.data_page(rng, 1, with_nulls(rng, words(rng, 90))),
              sp.data_page(rng, 2, words(rng, T + 3, 0, 3), required=True)]
    after = [sp.data_page(rng, 2, with_nulls(rng, words(rng, 70))),
             sp.data_page(rng, 1, [b"the", b"end"], required=True)]
    want = [0, 0] + [1] * len(bad) + [0, 0]
    if name == "an index equal to the entry count":
        want[2] = 0     # the dictionary itself is good
    m, rows = go(torch, dec, before + list(bad) + after, 31, want=want)
    assert sp.strings_of(m, rows[-1], 2) == [b"the", b"end"]


def test_bytes_avail_one_short_and_the_sizing_call(torch, dec):
    rng = random.Random(41)
    pages = [sp.data_page(rng, 1, with_nulls(rng, words(rng, 400, 1, 20))),
             sp.data_page(rng, 2, words(rng, 30, 1, 5), required=True),
             sp.data_page(rng, 1, [b"last page", b"!"], required=True)]
    buf, rows, out_n, valid_n = sp.lay_out(pages, rng)
    total = sm.decode(rows, buf, "gzip", out_n, valid_n, 0)["total"]
    # one byte short: the last page alone does not fit, and run_gpu's canary
    # behind bytes_avail shows that no byte at or behind it is touched
    m = sp.run_gpu(torch, dec, buf, rows, "gzip", out_n, valid_n, total - 1, [0, 0, 3])
    assert m["total"] == total
    sp.run_gpu(torch, dec, buf, rows, "gzip", out_n, valid_n, total, [0, 0, 0])
    # the sizing call: d_bytes NULL, every page with bytes is INSUFFICIENT_SPACE
    m = sp.run_gpu(torch, dec, buf, rows, "gzip", out_n, valid_n, 0, [3, 3, 3], sizing=True)
    assert m["total"] == total
