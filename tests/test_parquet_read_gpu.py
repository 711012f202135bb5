"""Parquet files written by pyarrow read on the GPU
(libdeflate_amd_parquet_decode_batch through libdeflate_amd.parquet.pages()).
No tolerance anywhere: every result, every slot byte and every validity byte
equal the CPU model's (tools/models/parquet_model.py) and what pyarrow itself
read back (tests/golden/parquet/*.npy), and the canary bytes in front of d_out
and d_valid, between the columns and behind out_avail and valid_avail stay
untouched (tests/parquet_pages.py: run_gpu)."""
import numpy as np
import pytest

from libdeflate_amd import parquet
from tests import parquet_pages as pp

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
    pg = parquet.pages(buf, columns, row_groups)
    res, out, valid = pp.run_gpu(torch, dec, buf, pg.rows, pg.format, pg.out_nbytes, pg.valid_nbytes,
                                 [0] * len(pg.rows))
    f = parquet.parse(buf)
    sizes = [g[0] for g in f.row_groups]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    groups = range(len(sizes)) if row_groups is None else row_groups
    order = np.concatenate([np.arange(starts[g], starts[g + 1]) for g in groups])
    for name, c in pg.columns.items():
        got = out[c.offset:c.offset + c.rows * c.width].reshape(c.rows, c.width)
        assert (got == want[name][0][order]).all(), name
        if c.valid_offset is not None:
            assert (valid[c.valid_offset:c.valid_offset + c.rows] == want[name][1][order]).all(), name
    return pg


@pytest.mark.parametrize("name", pp.fixture_files())
def test_whole_files_decode_to_pyarrows_values(torch, dec, name):
    buf, want = pp.fixture(name)
    pg = read(torch, dec, buf, want)
    assert set(pg.columns) == set(want)


@pytest.mark.parametrize("name", ["a_small_v1.parquet", "b_dict_v2.parquet"])
def test_single_columns(torch, dec, name):
    buf, want = pp.fixture(name)
    for col in want:
        pg = read(torch, dec, buf, want, [col])
        assert list(pg.columns) == [col] and pg.columns[col].offset == 0


@pytest.mark.parametrize("name", ["a_small_v2.parquet", "b_small_v1.parquet", "a_dict_v2_none.parquet"])
def test_row_groups_in_reverse_order(torch, dec, name):
    buf, want = pp.fixture(name)
    read(torch, dec, buf, want, None, [2, 1, 0])
    read(torch, dec, buf, want, list(want)[::-1][:2], [1])


def test_read_columns_returns_tensors(torch, dec):
    for name in ("a_small_v2.parquet", "b_small_v1.parquet"):
        buf, want = pp.fixture(name)
        d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        cols = parquet.read_columns(dec, buf, d_in)
        for col, (values, mask) in cols.items():
            w_values, w_valid = want[col]
            assert values.device.type == "cuda" and values.shape[0] == len(w_valid)
            assert values.cpu().numpy().view(np.uint8).reshape(w_values.shape).tolist() == \
                w_values.tolist()
            if col == "req_i32":
                assert mask is None
            else:
                assert mask.dtype == torch.bool and mask.cpu().numpy().tolist() == \
                    w_valid.astype(bool).tolist()
        if name.startswith("a"):
            assert [cols[c][0].dtype for c in ("req_i32", "i32", "i64", "f32")] == \
                [torch.int32, torch.int32, torch.int64, torch.float32]
        else:
            assert cols["ts96"][0].dtype == torch.uint8 and tuple(cols["ts96"][0].shape) == (1200, 12)
            assert tuple(cols["b5"][0].shape) == (1200, 5) and cols["f64_null"][0].dtype == torch.float64
