"""The CPU model of libdeflate_amd_parquet_decode_batch_ex
(tools/models/parquet_strings_model.py) over the rows of
libdeflate_amd.parquet.pages(strings=True) reproduces what pyarrow read back
from tests/golden/parquet_strings - offsets, bytes and validity, byte for byte -
for whole files and for columns and row groups selected and reordered; the
layout and the estimate of pages(); and the model's verdicts and rooms on
hand-built pages.  No GPU."""
import random

import numpy as np
import pytest

from libdeflate_amd import binding, parquet
from tests import parquet_pages as pp
from tests import parquet_string_pages as sp
from tools.models import parquet_model as pm
from tools.models import parquet_strings_model as sm


def model_read(buf, want, columns=None, row_groups=None):
    pg = parquet.pages(buf, columns, row_groups, strings=True)
    m = sm.decode(pg.rows, buf, pg.format, pg.out_nbytes, pg.valid_nbytes, pg.bytes_estimate, 0xA5)
    assert m["results"] == [0] * len(pg.rows) and m["total"] <= pg.bytes_estimate
    check_columns(pg, m["out"], m["valid"], m["data"], buf, want, row_groups)
    return pg, m


def check_columns(pg, out, valid, data, buf, want, row_groups=None):
    """the columns of layout pg against pyarrow's read-back, the rows of the
    selected row groups in their order"""
    sizes = [g[0] for g in parquet.parse(buf).row_groups]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    groups = range(len(sizes)) if row_groups is None else row_groups
    order = np.concatenate([np.arange(starts[g], starts[g + 1]) for g in groups])
    for name, c in pg.columns.items():
        w_off, w_bytes, w_valid = want[name]
        assert c.byte_array and c.rows == len(order) and c.offset % 64 == 0
        o = out[c.offset:c.offset + (c.rows + 1) * 8].view("<i8")
        lens = np.diff(w_off)[order]
        assert (np.diff(o) == lens).all(), name
        got = bytes(data[o[0]:o[-1]])
        assert got == b"".join(bytes(w_bytes[w_off[r]:w_off[r + 1]]) for r in order), name
        if c.valid_offset is not None:
            assert (valid[c.valid_offset:c.valid_offset + c.rows] == w_valid[order]).all(), name


@pytest.mark.parametrize("name", sp.fixture_files())
def test_the_model_reads_what_pyarrow_reads(name):
    buf, want = sp.fixture(name)
    pg, m = model_read(buf, want)
    assert set(pg.columns) == set(want) == {"pool", "uniq", "req", "nulls", "empty"}
    assert pg.columns["req"].valid_offset is None and pg.columns["pool"].valid_offset is not None
    # column by column: the first column's bytes start at 0, the next one's where they end
    first = [int(m["out"][c.offset:c.offset + 8].view("<i8")[0]) for c in pg.columns.values()]
    assert first[0] == 0 and first == sorted(first)
    assert (pg.rows[:, 3] & np.uint64(binding.PARQUET_BYTE_ARRAY)).all()
    assert not (pg.rows[:, 3] >> np.uint64(16) & np.uint64(255)).any()


@pytest.mark.parametrize("name", ["s_small_v1.parquet", "s_dict_v2.parquet"])
def test_columns_and_row_groups_selected_and_reordered(name):
    buf, want = sp.fixture(name)
    model_read(buf, want, ["uniq"], [2, 0])
    model_read(buf, want, ["empty", "req", "pool"], [1])
    model_read(buf, want, ["nulls", "pool"], [2, 1, 0])


def test_pages_keeps_refusing_strings_by_default_and_mixes_with_fixed_columns():
    buf, _ = sp.fixture("s_small_v1.parquet")
    with pytest.raises(ValueError, match="column 'pool': physical type BYTE_ARRAY"):
        parquet.pages(buf)
    pg = parquet.pages(buf, ["req"], strings=True)
    assert pg.columns["req"].width is None and pg.out_nbytes == (1200 + 1) * 8 // 64 * 64 + 64
    assert pg.bytes_estimate > 0
    fixed, _ = pp.fixture("a_small_v1.parquet")
    a, b = parquet.pages(fixed), parquet.pages(fixed, strings=True)
    assert (a.rows == b.rows).all() and b.bytes_estimate == 0 and a.out_nbytes == b.out_nbytes
    assert not any(c.byte_array for c in b.columns.values())


def test_parquet_rows_byte_array_keyword():
    from libdeflate_amd import api
    args = ([0, 20], [20, 30], [40, 90], [pm.DICT, pm.DATA_V1], [10, 50], [4, 1])
    old, new = api.parquet_rows(*args), api.parquet_rows(*args, byte_array=[0, 1])
    assert (old[0] == new[0]).all() and new[1, 3] == old[1, 3] | binding.PARQUET_BYTE_ARRAY
    assert sm.BYTE_ARRAY == binding.PARQUET_BYTE_ARRAY == 1 << 14


def test_the_model_on_hand_built_pages():
    rng = random.Random(5)
    d = sp.dict_page([b"", b"ab", b"xyz" * 50])
    good = sp.data_page(rng, 1, [b"ab", None, b"", b"xyz" * 50, None], d)
    plain = sp.data_page(rng, 2, [None, b"q", b"", b"rs"])
    short = sp.data_page(rng, 1, [b"abc", b"d"], section=sp.section_of([b"abc", b"d"])[:-1],
                         required=True)
    bad_idx = sp.data_page(rng, 1, [b"ab", b"ab", b"ab"], d, indices=[1, 3, 1], w=2, required=True)
    last = sp.data_page(rng, 1, [b"tail"], required=True)
    buf, rows, out_n, valid_n = sp.lay_out([d, good, plain, short, bad_idx, last], rng)
    m = sm.decode(rows, buf, "gzip", out_n, valid_n, 1000)
    assert m["results"] == [0, 0, 0, 1, 1, 0]
    assert sp.strings_of(m, rows[1], 5) == [b"ab", b"", b"", b"xyz" * 50, b""]
    assert sp.strings_of(m, rows[2], 4) == [b"", b"q", b"", b"rs"]
    assert sp.strings_of(m, rows[5], 1) == [b"tail"]
    # the short page takes no room, the bad index counts as length 0
    assert m["total"] == 152 + 3 + 0 + 4 + 4
    one_short = sm.decode(rows, buf, "gzip", out_n, valid_n, m["total"] - 1)
    assert one_short["results"] == [0, 0, 0, 1, 1, 3] and one_short["total"] == m["total"]
    assert sm.decode(rows, buf, "gzip", out_n, valid_n, 0)["results"] == [0, 3, 3, 1, 1, 3]
