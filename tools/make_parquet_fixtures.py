#!/usr/bin/env python3
"""Writes tests/golden/parquet: small Parquet files made by pyarrow - the only
place in this repository that imports it - and, per group of columns, what
pyarrow reads back from them: <group>.<column>.values.npy (uint8 [rows, width],
the little-endian bytes of every slot, nulls as zeros) and
<group>.<column>.valid.npy (uint8 [rows]).  Every file of a group holds the same
table, so the .npy files are the group's; the script checks that pyarrow reads
every file back to them.

    python tools/make_parquet_fixtures.py          # rewrites the directory

Deterministic: fixed seeds, no timestamps, no statistics.  MANIFEST.txt states
the pyarrow version it ran under.

The settings, per group: "small" (dictionary_pagesize_limit 300, data_page_size
512, write_batch_size 100) gives one dictionary page, one dictionary-coded data
page and then PLAIN pages - the dictionary fallback; "dict" (a dictionary limit
of 1 MiB) gives several dictionary-coded data pages per chunk.  Both in data
page versions 1.0 and 2.0.  Group a is also written with compression "none".

Group w holds one int32 column of 70 000 distinct values, for index bit width
17.  70 000 distinct 32-bit words do not deflate below about 1.3 bytes each,
so w_dict_v1.parquet and what pyarrow reads back from it (w.wide.npz, values and
validity in one compressed file) are the two files above 32 KiB here, and with
them the directory is above 512 KiB; without them it is far below."""
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "parquet")
ROWS = 1200
SETTINGS = {
    "small": dict(dictionary_pagesize_limit=300, data_page_size=512, write_batch_size=100),
    "dict": dict(dictionary_pagesize_limit=1 << 20, data_page_size=512, write_batch_size=100),
}


def nulls(rng, n, share):
    return rng.random_sample(n) < share


def group_a(rng):
    n = ROWS
    pool64 = rng.randint(-2 ** 62, 2 ** 62, size=300, dtype=np.int64)
    pool32 = (rng.random_sample(150) * 1000).astype(np.float32)
    cols = [
        (pa.field("req_i32", pa.int32(), nullable=False),
         pa.array(rng.randint(0, 200, size=n).astype(np.int32) * 1001)),       # 200 entries: width 8
        (pa.field("i32", pa.int32()), pa.array(np.where(rng.random_sample(n) < 0.3, 7, -9).astype(np.int32))),
        (pa.field("i64", pa.int64()), pa.array(pool64[rng.randint(0, 300, size=n)], mask=nulls(rng, n, 0.1))),
        (pa.field("f32", pa.float32()), pa.array(pool32[rng.randint(0, 150, size=n)], mask=nulls(rng, n, 0.1))),
    ]
    return pa.Table.from_arrays([c for _, c in cols], schema=pa.schema([f for f, _ in cols]))


def group_b(rng):
    n = ROWS
    words = [bytes(rng.randint(0, 256, size=5, dtype=np.uint8)) for _ in range(40)]
    uuids = [bytes(rng.randint(0, 256, size=16, dtype=np.uint8)) for _ in range(90)]
    m5, mt, m1 = nulls(rng, n, 0.1), nulls(rng, n, 0.1), nulls(rng, n, 0.1)
    stamps = (np.int64(1_600_000_000) + rng.randint(0, 400, size=n) * 86_399) * 1_000_000_000 + \
        rng.randint(0, 1000, size=n)
    cols = [
        (pa.field("f64_null", pa.float64()), pa.array([None] * n, type=pa.float64())),
        (pa.field("one", pa.int64()), pa.array(np.full(n, 123456789012, dtype=np.int64), mask=m1)),
        (pa.field("b5", pa.binary(5)),
         pa.array([None if m5[k] else words[rng.randint(0, 40)] for k in range(n)], type=pa.binary(5))),
        (pa.field("b16", pa.binary(16)),
         pa.array([uuids[rng.randint(0, 90)] for _ in range(n)], type=pa.binary(16))),
        (pa.field("ts96", pa.timestamp("ns")), pa.array(stamps, type=pa.timestamp("ns"), mask=mt)),
    ]
    return pa.Table.from_arrays([c for _, c in cols], schema=pa.schema([f for f, _ in cols]))


def group_w(rng):
    v = (np.arange(70_000, dtype=np.int64) * 3 - 100_000).astype(np.int32)
    return pa.Table.from_arrays([pa.array(v)], schema=pa.schema([pa.field("wide", pa.int32())]))


def slot_bytes(col):
    """(uint8 [rows, width], uint8 [rows]): what pyarrow read back, as the slots'
    little-endian bytes; INT96 as Parquet stores it - nanoseconds of the day,
    then the Julian day"""
    col = col.combine_chunks()
    valid = np.array([v is not None for v in col.to_pylist()], dtype=np.uint8) if col.null_count \
        else np.ones(len(col), dtype=np.uint8)
    t = col.type
    if pa.types.is_fixed_size_binary(t):
        out = np.zeros((len(col), t.byte_width), dtype=np.uint8)
        for k, v in enumerate(col.to_pylist()):
            if v is not None:
                out[k] = np.frombuffer(v, dtype=np.uint8)
        return out, valid
    if pa.types.is_timestamp(t):
        ns = np.asarray(col.cast(pa.int64()).fill_null(0)).astype(np.int64)
        out = np.zeros((len(col), 12), dtype=np.uint8)
        out[:, :8] = (ns % 86_400_000_000_000).astype("<i8").view(np.uint8).reshape(-1, 8)
        out[:, 8:] = (ns // 86_400_000_000_000 + 2_440_588).astype("<i4").view(np.uint8).reshape(-1, 4)
        out[valid == 0] = 0
        return out, valid
    a = np.asarray(col.fill_null(0))
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(col), a.dtype.itemsize), valid


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in os.listdir(OUT):
        os.remove(os.path.join(OUT, name))
    files = [("a", group_a, s, v, "gzip") for s in SETTINGS for v in ("1.0", "2.0")]
    files += [("b", group_b, s, v, "gzip") for s in SETTINGS for v in ("1.0", "2.0")]
    files += [("a", group_a, "small", "1.0", "none"), ("a", group_a, "dict", "2.0", "none")]
    files += [("w", group_w, "dict", "1.0", "gzip")]
    saved = {}
    for group, make, setting, version, codec in files:
        table = make(np.random.RandomState(20261021 + ord(group)))
        opts = dict(SETTINGS[setting])
        if group == "w":
            opts = dict(dictionary_pagesize_limit=1 << 20)
        name = "%s_%s_v%s%s.parquet" % (group, setting, version[0], "" if codec == "gzip" else "_none")
        path = os.path.join(OUT, name)
        pq.write_table(table, path, compression=codec, use_dictionary=True, data_page_version=version,
                       row_group_size=500 if group != "w" else 1 << 20, write_statistics=False,
                       use_deprecated_int96_timestamps=True, store_schema=False, **opts)
        back = pq.read_table(path)
        assert back.num_rows == table.num_rows
        for col in back.column_names:
            values, valid = slot_bytes(back.column(col))
            key = "%s.%s" % (group, col)
            if key in saved:
                assert (saved[key][0] == values).all() and (saved[key][1] == valid).all(), (name, col)
                continue
            saved[key] = (values, valid)
            if group == "w":
                np.savez_compressed(os.path.join(OUT, key + ".npz"), values=values, valid=valid)
                continue
            np.save(os.path.join(OUT, key + ".values.npy"), values)
            np.save(os.path.join(OUT, key + ".valid.npy"), valid)
    with open(os.path.join(OUT, "MANIFEST.txt"), "w") as f:
        f.write("written by tools/make_parquet_fixtures.py under pyarrow %s, numpy %s\n" %
                (pa.__version__, np.__version__))
        total = wide = 0
        for name in sorted(os.listdir(OUT)):
            if name != "MANIFEST.txt":
                size = os.path.getsize(os.path.join(OUT, name))
                total += size
                f.write("%8d %s\n" % (size, name))
                wide += size if name.startswith("w") else 0
                assert size < 32 << 10 or name.startswith("w"), (name, size)
        assert total - wide < 512 << 10 and total < 1 << 20, (total, wide)
    print("wrote %d files, %d bytes" % (len(os.listdir(OUT)), total))
    return 0


if __name__ == "__main__":
    sys.exit(main())
