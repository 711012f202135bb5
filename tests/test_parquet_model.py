"""The CPU model of the Parquet call (tools/models/parquet_model.py) and the host
side that feeds it (libdeflate_amd/parquet.py: the Thrift reader, parse(),
pages()): fed by parquet.pages(), the model reproduces exactly what pyarrow read
back from every file of tests/golden/parquet; its hybrid decoder undoes the
hand-built encoder of tests/parquet_pages.py over random run structures and
gives the header's verdicts on malformed streams; and, where pyarrow is
installed, it agrees with pyarrow's read-back of randomized tables.  No GPU."""
import random

import numpy as np
import pytest

from libdeflate_amd import parquet
from tests import parquet_pages as pp
from tools.models import parquet_model as pm

FILL = 0xA5


def model_columns(buf, columns=None, row_groups=None):
    pg = parquet.pages(buf, columns, row_groups)
    res, out, valid, out_def, valid_def = pm.decode(pg.rows, buf, pg.format, pg.out_nbytes,
                                                    pg.valid_nbytes, FILL)
    assert res == [pm.SUCCESS] * len(pg.rows)
    assert out_def.all() and valid_def.all()
    return pg, out, valid


@pytest.mark.parametrize("name", pp.fixture_files())
def test_the_model_reproduces_pyarrows_values(name):
    buf, want = pp.fixture(name)
    f = parquet.parse(buf)
    assert {leaf.name for leaf in f.leaves} == set(want)
    pg, out, valid = model_columns(buf)
    w_out, w_valid = pp.expected(pg, want, FILL)
    assert (out == w_out).all() and (valid == w_valid).all()
    for c in pg.columns.values():
        assert c.offset % 64 == 0 and (c.valid_offset or 0) % 64 == 0
        assert c.rows == f.num_rows == len(want[c.name][0])


def test_the_fixtures_cover_what_they_are_for():
    seen = set()
    widths = set()
    for name in pp.fixture_files():
        buf, _ = pp.fixture(name)
        f = parquet.parse(buf)
        pg = parquet.pages(buf, file=f)
        chunk_pages = {}
        for r in pg.rows:
            u = pm.unpack(r)
            seen.add((u["kind"], u["enc"], u["compressed"], u["max_def"]))
            if u["kind"] != pm.DICT and u["enc"] != pm.PLAIN:
                chunk_pages[u["dict"]] = chunk_pages.get(u["dict"], 0) + 1
                sec = pm.section(u, buf, pg.format)[1]
                at = 4 + int.from_bytes(sec[:4], "little") if u["kind"] == pm.DATA_V1 and u["max_def"] else 0
                if at < len(sec):
                    widths.add(sec[at])
        if "_dict_" in name and not name.startswith("w"):
            assert max(chunk_pages.values()) > 1       # several dictionary-coded pages per chunk
        if "_small_" in name:
            assert any(k[1] == pm.PLAIN and k[0] != pm.DICT for k in
                       ((pm.unpack(r)["kind"], pm.unpack(r)["enc"]) for r in pg.rows))
        assert len(f.row_groups) == (1 if name.startswith("w") else 3)
    assert {k[0] for k in seen} == {pm.DATA_V1, pm.DICT, pm.DATA_V2}
    assert {k[1] for k in seen} == {pm.PLAIN, pm.RLE_DICTIONARY}
    assert {k[2] for k in seen} == {0, 1} and {k[3] for k in seen} == {0, 1}
    assert widths >= {0, 1, 8, 17}, widths


def test_columns_and_row_groups_are_selected():
    buf, want = pp.fixture("b_small_v2.parquet")
    pg, out, valid = model_columns(buf, ["ts96", "b5"], [2, 0])
    f = parquet.parse(buf)
    sizes = [g[0] for g in f.row_groups]
    order = np.concatenate([np.arange(sum(sizes[:2]), sum(sizes)), np.arange(sizes[0])])
    assert list(pg.columns) == ["ts96", "b5"]
    for name, c in pg.columns.items():
        got = out[c.offset:c.offset + c.rows * c.width].reshape(c.rows, c.width)
        assert (got == want[name][0][order]).all()
        assert (valid[c.valid_offset:c.valid_offset + c.rows] == want[name][1][order]).all()


def test_out_of_scope_raises_with_the_column():
    buf, _ = pp.fixture("a_small_v1.parquet")
    with pytest.raises(KeyError):
        parquet.pages(buf, ["nope"])
    f = parquet.parse(buf)
    f.leaves[1].max_def = 2
    with pytest.raises(ValueError, match="'i32'.*nested"):
        parquet.pages(buf, file=f)
    f = parquet.parse(buf)
    f.leaves[2].type = parquet.BYTE_ARRAY
    with pytest.raises(ValueError, match="'i64'.*BYTE_ARRAY"):
        parquet.pages(buf, file=f)
    f = parquet.parse(buf)
    f.row_groups[0][1][0].codec = parquet.SNAPPY
    with pytest.raises(ValueError, match="'req_i32'.*SNAPPY"):
        parquet.pages(buf, file=f)
    with pytest.raises(ValueError, match="PAR1"):
        parquet.parse(buf[:-1])


@pytest.mark.parametrize("w", [0, 1, 2, 7, 8, 9, 16, 17, 31, 32])
def test_the_hybrid_decoder_undoes_the_encoder(w):
    rng = random.Random(w)
    for trial in range(30):
        n = rng.choice([1, 7, 8, 9, 63, 64, 65, 500, 1025])
        if rng.random() < 0.5:      # stretches of equal values, so that RLE runs have lengths
            vals = []
            while len(vals) < n:
                vals += [rng.randrange(1 << w) if w else 0] * rng.randrange(1, 20)
            vals = vals[:n]
        else:
            vals = [rng.randrange(1 << w) if w else 0 for _ in range(n)]
        for shape in ("rle", "rle1", "bp", "alt"):
            for hdr in (None, 2, 5):
                runs = pp.runs_of(vals, w, shape, rng, group_max=rng.choice([1, 3, 63]))
                stream = pp.encode_runs(runs, w, hdr)
                got = pm.hybrid(stream + b"junk", w, n)
                assert got is not None and got.tolist() == vals, (w, n, shape, hdr)
                # bytes behind the last needed run are not needed
                assert pm.hybrid(stream, w, n).tolist() == vals


def test_the_hybrid_verdicts():
    bp8 = pp.encode_runs([("bp", [1, 0, 1, 1, 0, 0, 1, 0])], 1)
    assert pm.hybrid(bp8, 1, 8).tolist() == [1, 0, 1, 1, 0, 0, 1, 0]
    assert pm.hybrid(bytes([0x90, 0x4E, 0x01]), 1, 5000).tolist() == [1] * 5000     # pyarrow's 5000 non-nulls
    assert pm.hybrid(b"\x00\x01", 1, 1) is None             # a run of 0 copies
    assert pm.hybrid(b"\x01", 1, 1) is None                 # a run of 0 groups
    assert pm.hybrid(pp.uleb(8 << 1, 6) + b"\x01", 1, 8) is None        # a header of 6 bytes
    assert pm.hybrid(pp.uleb(8 << 1, 5) + b"\x01", 1, 8).tolist() == [1] * 8
    assert pm.hybrid(bp8, 1, 9) is None                     # the stream ends before N
    assert pm.hybrid(bp8[:1], 1, 8) is None
    assert pm.hybrid(b"\x10", 8, 8) is None                 # an RLE value that leaves the stream
    assert pm.hybrid(b"\x10\x02", 1, 8, levels=True) is None            # an RLE level of 2
    # only the bytes that cover the values owed must be there: 3 groups of width 8, 9 values owed
    assert pm.hybrid(bytes([7]) + bytes(range(9)), 8, 9).tolist() == list(range(9))
    assert pm.hybrid(bytes([7]) + bytes(range(8)), 8, 9) is None
    assert pm.hybrid(b"", 5, 0).tolist() == []


def test_page_verdicts_on_hand_built_pages():
    rng = random.Random(5)
    entries = np.arange(12, dtype=np.uint8).reshape(3, 4)
    d = pp.dict_page(entries)
    ok, want = pp.data_page(rng, 1, 4, mask=[1, 0, 1, 1], dictionary=d, entries=entries)
    bad_index, _ = pp.data_page(rng, 2, 4, mask=[1, 1], dictionary=d, entries=entries, indices=[0, 3], w=2)
    empty, _ = pp.data_page(rng, 2, 4, mask=[0, 0, 0], dictionary=d, entries=entries)
    assert empty.stored[empty.def_len:] == pp.pack("gzip", b"")
    short = pp.data_page(rng, 1, 8, n=3)[0]
    short.count = 4
    buf, rows, out_n, valid_n = pp.lay_out([d, ok, bad_index, empty, short], rng)
    res, out, valid, out_def, _ = pm.decode(rows, buf, "gzip", out_n, valid_n, FILL)
    assert res == [0, 0, pm.BAD_DATA, 0, pm.BAD_DATA]
    u = pm.unpack(rows[1])
    assert (out[u["out"]:u["out"] + 16].reshape(4, 4) == want).all()
    assert valid[u["valid"]:u["valid"] + 4].tolist() == [1, 0, 1, 1]
    u = pm.unpack(rows[2])
    assert not out_def[u["out"]:u["out"] + 8].any()
    # a dictionary that fails poisons its pages; an inflate result comes first
    rows[0, 2] += 1
    res = pm.decode(rows, buf, "gzip", out_n, valid_n)[0]
    assert res == [pm.SHORT_OUTPUT, pm.BAD_DATA, pm.BAD_DATA, pm.BAD_DATA, pm.BAD_DATA]


def test_the_model_agrees_with_pyarrow_on_random_tables(tmp_path):
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    from tools import make_parquet_fixtures as mk
    for seed in range(4):
        rng = np.random.RandomState(seed)
        n = int(rng.randint(1, 3000))
        fields, arrays = [], []
        for k, (t, lo, hi) in enumerate([(np.int32, -5, 5), (np.int64, -2 ** 40, 2 ** 40),
                                         (np.float32, 0, 3), (np.float64, 0, 100000)]):
            nullable = bool(rng.randint(2))
            mask = rng.random_sample(n) < rng.choice([0.0, 0.1, 1.0]) if nullable else None
            fields.append(pa.field("c%d" % k, pa.from_numpy_dtype(t), nullable=nullable))
            arrays.append(pa.array(rng.randint(lo, hi, size=n).astype(t), mask=mask))
        path = str(tmp_path / ("t%d.parquet" % seed))
        pq.write_table(pa.Table.from_arrays(arrays, schema=pa.schema(fields)), path,
                       compression=["gzip", "none"][seed % 2],
                       data_page_version=["1.0", "2.0"][seed // 2 % 2],
                       data_page_size=int(rng.choice([256, 4096, 1 << 20])),
                       dictionary_pagesize_limit=int(rng.choice([64, 1 << 20])),
                       row_group_size=int(rng.choice([n // 2 + 1, n + 1])))
        buf = open(path, "rb").read()
        back = pq.read_table(path)
        pg, out, valid = model_columns(buf)
        for name, c in pg.columns.items():
            values, ok = mk.slot_bytes(back.column(name))
            assert (out[c.offset:c.offset + c.rows * c.width].reshape(c.rows, c.width) == values).all()
            if c.valid_offset is not None:
                assert (valid[c.valid_offset:c.valid_offset + c.rows] == ok).all()
            else:
                assert ok.all()
