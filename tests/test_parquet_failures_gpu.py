"""Malformed Parquet pages through libdeflate_amd_parquet_decode_batch: one bad
page among good neighbours per case.  The verdicts are the header's, stated
here and checked against the CPU model too; the neighbours stay exact, the bad
page's own slots are all that may differ, and the canaries hold
(tests/parquet_pages.py: run_gpu)."""
import random

import numpy as np
import pytest

from tests import parquet_pages as pp
from tools.models import parquet_model as pm

pytestmark = pytest.mark.gpu

OK, BAD, SHORT, SPACE = pm.SUCCESS, pm.BAD_DATA, pm.SHORT_OUTPUT, pm.INSUFFICIENT_SPACE


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


ENTRIES = (np.arange(40, dtype=np.uint8).reshape(10, 4) * 3 + 1).astype(np.uint8)


def neighbours(rng, d):
    return [pp.data_page(rng, 1, 4, mask=[1, 0, 1] * 50, dictionary=d, entries=ENTRIES)[0],
            pp.data_page(rng, 2, 4, mask=[0, 1] * 600)[0]]


def case(torch, dec, make, want, seed):
    """make(rng, d) -> the bad page, between good neighbours that share its
    dictionary d"""
    rng = random.Random(seed)
    d = pp.dict_page(ENTRIES)
    a, b = neighbours(rng, d)
    bad = make(rng, d)
    buf, rows, out_n, valid_n = pp.lay_out([d, a, bad, b], rng)
    pp.run_gpu(torch, dec, buf, rows, "gzip", out_n, valid_n, [OK, OK, want, OK])


def flipped(rng, d):
    p = pp.data_page(rng, 1, 4, n=500)[0]
    s = bytearray(p.stored)
    s[-6] ^= 0x10       # in the member's CRC-32
    p.stored = bytes(s)
    return p


def levels_and_indices(levels, section, n, version=2, width=4):
    p = pp.Page(pm.DATA_V1 if version == 1 else pm.DATA_V2, width, n, section, levels,
                pm.RLE_DICTIONARY, 1)
    return p


def with_dict(p, d):
    p.dict_page = d
    return p


ALL_VALID = bytes([8 << 1, 1])          # an RLE run of 8 ones
CASES = {
    "a flipped byte in a gzip body": (flipped, BAD),
    "uncompressed_page_size one too small": (
        lambda rng, d: pp.Page(pm.DATA_V1, 4, 100, bytes(400), usize_delta=-1), SPACE),
    "uncompressed_page_size one too large": (
        lambda rng, d: pp.Page(pm.DATA_V1, 4, 100, bytes(400), usize_delta=1), SHORT),
    "an index equal to the entry count": (
        lambda rng, d: pp.data_page(rng, 1, 4, n=300, dictionary=d, entries=ENTRIES,
                                    indices=[9] * 299 + [10], w=4)[0], BAD),
    "an RLE index equal to the entry count": (
        lambda rng, d: pp.data_page(rng, 2, 4, n=300, dictionary=d, entries=ENTRIES,
                                    indices=[10] * 300, w=4, shape="rle")[0], BAD),
    "a zero-length RLE run": (
        lambda rng, d: with_dict(levels_and_indices(ALL_VALID, bytes([4, 0, 3, 8 << 1, 3]), 8), d), BAD),
    "a zero-length bit-packed run": (
        lambda rng, d: with_dict(levels_and_indices(bytes([1, 8 << 1, 1]), bytes([4, 8 << 1, 3]), 8), d), BAD),
    "an index stream that ends before N": (
        lambda rng, d: with_dict(levels_and_indices(ALL_VALID, bytes([4, 7 << 1, 3]), 8), d), BAD),
    "a level stream that ends before N": (
        lambda rng, d: with_dict(levels_and_indices(bytes([7 << 1, 1]), bytes([4, 8 << 1, 3]), 8, 1), d), BAD),
    "a bit-packed run that leaves the stream": (
        lambda rng, d: with_dict(levels_and_indices(ALL_VALID, bytes([4, 3, 0x21, 0x43, 0x65]), 8), d), BAD),
    "a missing bit-width byte": (
        lambda rng, d: with_dict(levels_and_indices(ALL_VALID, b"", 8), d), BAD),
    "a run header of six bytes": (
        lambda rng, d: with_dict(levels_and_indices(pp.uleb(8 << 1, 6) + b"\x01", bytes([4, 8 << 1, 3]), 8), d),
        BAD),
    "bit width 33": (
        lambda rng, d: with_dict(levels_and_indices(ALL_VALID, bytes([33, 8 << 1, 3, 0, 0, 0, 0]), 8), d), BAD),
    "an RLE level of 2": (
        lambda rng, d: with_dict(levels_and_indices(bytes([8 << 1, 2]), bytes([4, 8 << 1, 3]), 8), d), BAD),
    "a V1 level length that leaves the page": (
        lambda rng, d: pp.Page(pm.DATA_V1, 4, 8, bytes(32), ALL_VALID, pm.PLAIN, 1, level_len=35), BAD),
    "a short PLAIN section": (
        lambda rng, d: pp.Page(pm.DATA_V2, 8, 9, bytes(71), bytes([9 << 1, 1]), pm.PLAIN, 1), BAD),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_bad_page_among_good_ones(torch, dec, name):
    make, want = CASES[name]
    case(torch, dec, make, want, len(name))


def test_the_good_forms_of_the_cases_pass(torch, dec):
    """the hand-written streams above are wrong only where they mean to be"""
    def good(rng, d):
        return with_dict(levels_and_indices(ALL_VALID, bytes([4, 8 << 1, 3]), 8), d)
    case(torch, dec, good, OK, 1)
    case(torch, dec, lambda rng, d: with_dict(
        levels_and_indices(pp.uleb(8 << 1, 5) + b"\x01", bytes([4, 3, 0x21, 0x43, 0x65, 0x07]), 8), d), OK, 2)
    case(torch, dec, lambda rng, d: pp.Page(pm.DATA_V2, 8, 9, bytes(72), bytes([9 << 1, 1]), pm.PLAIN, 1),
         OK, 3)


def test_a_dictionary_page_that_fails_poisons_its_pages(torch, dec):
    for how, want_dict in (("inflate", BAD), ("short", BAD), ("size", SHORT)):
        rng = random.Random(7)
        d, other = pp.dict_page(ENTRIES), pp.dict_page(ENTRIES[:5])
        if how == "inflate":
            s = bytearray(d.stored)
            s[-6] ^= 1
            d.stored = bytes(s)
        elif how == "short":
            d.count = 11        # 44 bytes of entries in a section of 40
        else:
            d.usize += 1
        a, b = neighbours(rng, d)
        c = pp.data_page(rng, 1, 4, mask=[1, 1, 0, 1], dictionary=other, entries=ENTRIES[:5])[0]
        buf, rows, out_n, valid_n = pp.lay_out([d, other, a, c, b], rng)
        # a, coded with the failed dictionary, is BAD_DATA; b is PLAIN and c has its own dictionary
        pp.run_gpu(torch, dec, buf, rows, "gzip", out_n, valid_n, [want_dict, OK, BAD, OK, OK])
