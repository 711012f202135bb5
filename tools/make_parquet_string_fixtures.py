#!/usr/bin/env python3
"""Writes tests/golden/parquet_strings: small Parquet files with BYTE_ARRAY
columns made by pyarrow and what pyarrow reads back from them, per column
s.<column>.npz with `offsets` (int64 [rows + 1], from 0), `bytes` (uint8) and
`valid` (uint8 [rows]); c.<column>.npz for the 300-row cut.

    python tools/make_parquet_string_fixtures.py       # rewrites the directory

Deterministic: fixed seeds, no timestamps, no statistics, store_schema=False.
MANIFEST.txt states the pyarrow version it ran under.

The table, 1200 rows in row groups of 500: `pool`, a nullable string drawn from
60 values, among them "" and a 140-byte word of multi-byte characters; `uniq`,
a nullable binary of unique values; `req`, a required string; `nulls`, a string
column of nulls only; `empty`, a string column of "" only.  The settings are
tools/make_parquet_fixtures.py's: "small" gives a dictionary page, a
dictionary-coded data page and then PLAIN pages - the fallback -, "dict"
several dictionary-coded pages per chunk; both in data page versions 1.0 and
2.0 with gzip.  One file of the first 300 rows is uncompressed, a cut to keep
it below 32 KiB.  The script checks that the files hold
the page kinds they are there for."""
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "parquet_strings")
ROWS, CUT = 1200, 300
SETTINGS = {
    "small": dict(dictionary_pagesize_limit=300, data_page_size=512, write_batch_size=100),
    "dict": dict(dictionary_pagesize_limit=1 << 20, data_page_size=512, write_batch_size=100),
}


def table(rng, n):
    letters = "abcdefghijklmnopqrstuvwxyz -_"
    pool = ["", "ä世\U0001f600x" * 14]     # 140 bytes of UTF-8
    assert len(pool[1].encode()) == 140
    while len(pool) < 60:
        pool.append("".join(letters[k] for k in rng.randint(0, len(letters), size=rng.randint(1, 24))))
    m_pool, m_uniq = rng.random_sample(n) < 0.15, rng.random_sample(n) < 0.1
    uniq = [bytes(rng.randint(0, 256, size=rng.randint(0, 20), dtype=np.uint8)) + k.to_bytes(2, "little")
            for k in range(n)]
    cols = [
        (pa.field("pool", pa.string()),
         pa.array([None if m_pool[k] else pool[rng.randint(0, 60)] for k in range(n)], type=pa.string())),
        (pa.field("uniq", pa.binary()),
         pa.array([None if m_uniq[k] else uniq[k] for k in range(n)], type=pa.binary())),
        (pa.field("req", pa.string(), nullable=False),
         pa.array(["row %d of the %s" % (k, pool[2 + k % 7]) for k in range(n)], type=pa.string())),
        (pa.field("nulls", pa.string()), pa.array([None] * n, type=pa.string())),
        (pa.field("empty", pa.string()), pa.array([""] * n, type=pa.string())),
    ]
    return pa.Table.from_arrays([c for _, c in cols], schema=pa.schema([f for f, _ in cols]))


def read_back(col):
    """(offsets int64 from 0, bytes uint8, valid uint8): what pyarrow read"""
    vals = col.combine_chunks().to_pylist()
    raw = [b"" if v is None else v.encode() if isinstance(v, str) else v for v in vals]
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in raw])]).astype(np.int64)
    return offsets, np.frombuffer(b"".join(raw), dtype=np.uint8), \
        np.array([v is not None for v in vals], dtype=np.uint8)


def page_kinds(path):
    """[(column, [(kind, encoding) per page])] per column chunk, by the
    project's own footer and page header reader"""
    from libdeflate_amd import parquet
    buf = open(path, "rb").read()
    f, out = parquet.parse(buf), []
    for _, chunks in f.row_groups:
        for ch in chunks:
            at, kinds, slots = ch.start, [], 0
            while slots < ch.num_values:
                th = parquet.Thrift(buf, at)
                ph = th.struct()
                at = th.at + ph[3]
                if ph[1] == parquet.DICTIONARY_PAGE:
                    kinds.append((ph[1], ph[7].get(2, 0)))
                else:
                    h = ph[5] if ph[1] == parquet.DATA_PAGE else ph[8]
                    kinds.append((ph[1], h[2 if ph[1] == parquet.DATA_PAGE else 4]))
                    slots += h[1]
            out.append((f.leaves[ch.leaf].name, kinds))
    return out


def main():
    from libdeflate_amd import parquet
    os.makedirs(OUT, exist_ok=True)
    for name in os.listdir(OUT):
        os.remove(os.path.join(OUT, name))
    full = table(np.random.RandomState(20261022), ROWS)
    files = [("s", full, s, v, "gzip") for s in SETTINGS for v in ("1.0", "2.0")]
    files.append(("c", full.slice(0, CUT), "small", "1.0", "none"))
    saved = {}
    for group, tab, setting, version, codec in files:
        name = "%s_%s_v%s%s.parquet" % (group, setting, version[0], "" if codec == "gzip" else "_none")
        path = os.path.join(OUT, name)
        pq.write_table(tab, path, compression=codec, use_dictionary=True, data_page_version=version,
                       row_group_size=500, write_statistics=False, store_schema=False,
                       **SETTINGS[setting])
        back = pq.read_table(path)
        assert back.num_rows == tab.num_rows
        for col in back.column_names:
            got = read_back(back.column(col))
            key = "%s.%s" % (group, col)
            if key in saved:
                assert all((a == b).all() for a, b in zip(saved[key], got)), (name, col)
                continue
            saved[key] = got
            np.savez_compressed(os.path.join(OUT, key + ".npz"), offsets=got[0], bytes=got[1],
                                valid=got[2])
        # the page kinds the file is there for
        kinds = page_kinds(path)
        data = (parquet.DATA_PAGE, parquet.DATA_PAGE_V2)
        assert any(k in data and e == parquet.RLE_DICTIONARY for _, ks in kinds for k, e in ks), name
        if setting == "small":
            assert any(ks[0][0] == parquet.DICTIONARY_PAGE and
                       any(k in data and e == parquet.PLAIN for k, e in ks[1:])
                       for _, ks in kinds), name
    with open(os.path.join(OUT, "MANIFEST.txt"), "w") as f:
        f.write("written by tools/make_parquet_string_fixtures.py under pyarrow %s, numpy %s\n" %
                (pa.__version__, np.__version__))
        total = 0
        for name in sorted(os.listdir(OUT)):
            if name != "MANIFEST.txt":
                size = os.path.getsize(os.path.join(OUT, name))
                total += size
                f.write("%8d %s\n" % (size, name))
                assert size < 32 << 10, (name, size)
        assert total < 256 << 10, total
    print("wrote %d files, %d bytes" % (len(os.listdir(OUT)), total))
    return 0


if __name__ == "__main__":
    sys.exit(main())
