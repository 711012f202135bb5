"""Parquet files with BYTE_ARRAY columns written by pyarrow, read on the GPU
(libdeflate_amd_parquet_decode_batch_ex through
libdeflate_amd.parquet.pages(strings=True) and read_columns()).  No tolerance:
results, the total, offsets, string bytes and validity bytes equal the CPU
model's (tools/models/parquet_strings_model.py) and what pyarrow itself read
back (tests/golden/parquet_strings/*.npz), and the canaries in front of, between
and behind the offsets, the bytes and the validity stay untouched
(tests/parquet_string_pages.py: run_gpu)."""
import numpy as np
import pytest

from libdeflate_amd import parquet
from tests import parquet_pages as pp
from tests import parquet_string_pages as sp
from tests.test_parquet_strings_model import check_columns

pytestmark = pytest.mark.gpu


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


def read(torch, dec, buf, want, columns=None, row_groups=None):
    pg = parquet.pages(buf, columns, row_groups, strings=True)
    m = sp.run_gpu(torch, dec, buf, pg.rows, pg.format, pg.out_nbytes, pg.valid_nbytes,
                   want_results=[0] * len(pg.rows))
    check_columns(pg, m["out"], m["valid"], m["data"], buf, want, row_groups)
    return pg


@pytest.mark.parametrize("name", sp.fixture_files())
def test_whole_files_decode_to_pyarrows_strings(torch, dec, name):
    buf, want = sp.fixture(name)
    assert set(read(torch, dec, buf, want).columns) == set(want)


def test_columns_and_row_groups_selected_and_reordered(torch, dec):
    buf, want = sp.fixture("s_small_v2.parquet")
    read(torch, dec, buf, want, ["uniq", "pool"], [2, 0])
    read(torch, dec, buf, want, ["empty", "nulls"], [1])


def as_host(cols):
    return {k: ((v[0][0].cpu().numpy(), v[0][1].cpu().numpy()) if isinstance(v[0], tuple)
                else v[0].cpu().numpy(), None if v[1] is None else v[1].cpu().numpy())
            for k, v in cols.items()}


@pytest.mark.parametrize("estimate", [None, 0])
@pytest.mark.parametrize("name", sp.fixture_files())
def test_read_columns_in_one_pass_and_in_two(torch, dec, name, estimate, monkeypatch):
    """estimate None: the page headers' estimate suffices, one call; 0: every
    string page says INSUFFICIENT_SPACE and the call is made again"""
    buf, want = sp.fixture(name)
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    calls = []
    real = type(dec).parquet_decode_batch_ex
    monkeypatch.setattr(type(dec), "parquet_decode_batch_ex",
                        lambda self, *a, **k: (calls.append(a[5].numel()), real(self, *a, **k))[1])
    cols = as_host(parquet.read_columns(dec, buf, d_in, bytes_estimate=estimate))
    total = sum(len(w[1]) for w in want.values())
    assert calls == ([parquet.pages(buf, strings=True).bytes_estimate] if estimate is None
                     else [0, total])
    assert set(cols) == set(want)
    for col, ((offsets, data), mask) in cols.items():
        w_off, w_bytes, w_valid = want[col]
        assert offsets.dtype == np.int64 and offsets.tolist() == w_off.tolist(), col
        assert data.tobytes() == w_bytes.tobytes(), col
        assert (mask is None) == (col == "req")
        assert mask is None or mask.tolist() == w_valid.astype(bool).tolist()


def test_a_string_column_and_a_fixed_width_column_in_one_call(torch, dec):
    """the pages of a string column and of the columns of an existing
    fixed-width fixture side by side in one buffer and one call"""
    s_buf, s_want = sp.fixture("s_small_v1.parquet")
    a_buf, a_want = pp.fixture("a_small_v1.parquet")
    ps = parquet.pages(s_buf, ["pool"], strings=True)
    pa = parquet.pages(a_buf, ["i64", "req_i32"])
    rows_a = pa.rows.copy()
    data = rows_a[:, 3] & np.uint64(15) != np.uint64(2)
    rows_a[:, 0] += np.uint64(len(s_buf))
    rows_a[data, 5] += np.uint64(ps.out_nbytes)
    rows_a[data, 6] += np.uint64(ps.valid_nbytes)
    coded = data & ((rows_a[:, 3] >> np.uint64(4) & np.uint64(255)) != np.uint64(0))
    rows_a[coded, 7] += np.uint64(3)         # they stand behind the first three string rows
    # the two columns' pages in turns: fixed-width rows between the string pages
    rows = np.concatenate([ps.rows[:3], rows_a, ps.rows[3:]])
    late = np.arange(len(rows)) >= 3 + len(rows_a)
    s_coded = late & ((rows[:, 3] >> np.uint64(4) & np.uint64(255)) != np.uint64(0)) & \
        (rows[:, 7] >= np.uint64(3))
    rows[s_coded, 7] += np.uint64(len(rows_a))
    assert ps.format == pa.format
    m = sp.run_gpu(torch, dec, s_buf + a_buf, rows, ps.format, ps.out_nbytes + pa.out_nbytes,
                   ps.valid_nbytes + pa.valid_nbytes, want_results=[0] * len(rows))
    check_columns(ps, m["out"], m["valid"], m["data"], s_buf, s_want)
    for name, c in pa.columns.items():
        at = ps.out_nbytes + c.offset
        assert (m["out"][at:at + c.rows * c.width].reshape(c.rows, c.width) == a_want[name][0]).all()
        if c.valid_offset is not None:
            at = ps.valid_nbytes + c.valid_offset
            assert (m["valid"][at:at + c.rows] == a_want[name][1]).all()
