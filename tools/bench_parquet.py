"""Parquet pages read on the device: the call and its kernels alone, against
the plain batch decode of the same gzip members and a plain copy, in the same
run on the same card.

    python tools/bench_parquet.py [--mib 256] [--steps 7] [--rounds 3] [--file F] [--out FILE]

A synthetic table of --mib MiB of column bytes, made here page by page (numpy;
no Parquet library): four columns of equal size - int64 PLAIN with 10 % nulls,
int32 dictionary-coded (1000 entries, bit width 10) with 10 % nulls, double
PLAIN required, int64 dictionary-coded (200 entries, bit width 8) required -,
values from small pools so that pages deflate, levels and indices bit-packed in
runs of 63 groups as pyarrow writes them, V1 pages, every body one gzip member
(zlib level 6); --pool distinct pages per column, repeated.  Two shards: pages
of about 1 MiB (pyarrow's default) and of about 64 KiB.  Per shard and round,
device times by HIP events around the enqueued work, best of --steps after
--warmup (every run is kept as *_runs):
  read_ms            libdeflate_amd_parquet_decode_batch: plan upload, inflate
                     into scratch, run lists, expand, verdicts
  plain_read_ms      libdeflate_amd_decompress_batch of the same members into
                     scratch: the decode a caller pays anyway
  runs_ms, expand_ms the call with the run-list kernel, the expand kernel alone
                     queued, on the scratch a full call filled
  no_stage_ms        the same with no stage queued: the host's plan, the upload
                     and the verdict kernel; *_kernel_ms are the two less this
  memcpy_ms          one device-to-device copy of the column bytes: the
                     kernels' yardstick
  call_host_ms       wall time of the call's return (the host's plan)
--file: a Parquet file (any writer's); parquet.pages() over it is timed on the
host (pages_host_ms) and it is read once.  One JSON object on stdout (and
--out; profiles/parquet_bench.json holds the run quoted in DESIGN.md).
"""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding, parquet  # noqa: E402
from tools.bench_png import timed  # noqa: E402
from tools.models import parquet_model as pm  # noqa: E402

RUN = 504       # values of a bit-packed run of 63 groups


def packed_runs(np, values, w):
    """values (a multiple of RUN) bit-packed LSB-first in runs of 63 groups"""
    bits = ((values[:, None] >> np.arange(w)) & 1).astype(np.uint8).reshape(-1)
    body = np.packbits(bits, bitorder="little").reshape(-1, 63 * w)
    head = np.full((len(body), 1), 63 << 1 | 1, dtype=np.uint8)
    return np.concatenate([head, body], axis=1).tobytes()


def page(np, rng, kind, n):
    """-> (the V1 body, uint8 [n, width] slots, uint8 [n] validity or None, the
    dictionary's entries or None)"""
    width, nullable, entries = {"i64": (8, 1, 0), "i32d": (4, 1, 1000), "f64": (8, 0, 0),
                                "i64d": (8, 0, 200)}[kind]
    mask = (rng.random_sample(n) >= 0.1).astype(np.int64) if nullable else np.ones(n, dtype=np.int64)
    nv = int(mask.sum())
    body = b""
    if nullable:
        lev = packed_runs(np, mask, 1)
        body = len(lev).to_bytes(4, "little") + lev
    dt = {4: "<i4", 8: "<i8"}[width]
    table = None
    if entries:
        table = (np.arange(entries, dtype=np.int64) * 7919 - 1000).astype(dt)
        idx = rng.randint(0, entries, size=nv)
        w = int(entries - 1).bit_length()
        pad = np.concatenate([idx, np.zeros(-nv % RUN, dtype=idx.dtype)])
        body += bytes([w]) + packed_runs(np, pad, w)
        vals = table[idx]
    elif kind == "f64":
        vals = (rng.randint(0, 5000, size=nv) / 8.0).astype("<f8")
        body += vals.tobytes()
    else:
        vals = (rng.randint(0, 3000, size=nv).astype(np.int64) * 1_000_003).astype(dt)
        body += vals.tobytes()
    slots = np.zeros((n, width), dtype=np.uint8)
    slots[mask == 1] = vals.view(np.uint8).reshape(nv, width)
    return body, slots, mask.astype(np.uint8) if nullable else None, table


def gz(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def build(np, mib, page_bytes, pool):
    """-> (file bytes, rows, expected out, expected valid)"""
    rng = np.random.RandomState(page_bytes)
    buf, rows, outs, valids = bytearray(b"PAR1"), [], [], []
    out_at = valid_at = 0
    for kind, per_value in (("i64", 8), ("i32d", 1.25), ("f64", 8), ("i64d", 1)):
        n = max(RUN, int(page_bytes / per_value) // RUN * RUN)
        made = [page(np, rng, kind, n) for _ in range(pool)]
        stored = [gz(m[0]) for m in made]
        width = made[0][1].shape[1]
        count = max(1, (mib << 20) // 4 // (n * width))
        dict_row = 0
        if made[0][3] is not None:
            d = made[0][3].tobytes()
            z = gz(d)
            dict_row = len(rows)
            rows.append([len(buf), len(z), len(d), pm.DICT | 1 << 12 | (width - 1) << 16,
                         len(made[0][3]), 0, 0, 0])
            buf += z
        out_at, valid_at = (out_at + 63) // 64 * 64, (valid_at + 63) // 64 * 64
        outs.append(np.zeros(out_at - sum(len(o) for o in outs), dtype=np.uint8))
        valids.append(np.zeros(valid_at - sum(len(v) for v in valids), dtype=np.uint8))
        for k in range(count):
            body, slots, valid, table = made[k % pool]
            enc = pm.RLE_DICTIONARY if table is not None else pm.PLAIN
            rows.append([len(buf), len(stored[k % pool]), len(body),
                         pm.DATA_V1 | enc << 4 | 1 << 12 | int(valid is not None) << 13 | (width - 1) << 16,
                         n, out_at, valid_at if valid is not None else 0, dict_row])
            buf += stored[k % pool]
            outs.append(slots.reshape(-1))
            out_at += n * width
            if valid is not None:
                valids.append(valid)
                valid_at += n
    return bytes(buf), np.array(rows, dtype=np.uint64), np.concatenate(outs), np.concatenate(valids)


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--pool", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--file")
    ap.add_argument("--out")
    a = ap.parse_args()
    d = api.Decompressor()
    lib = binding.load()
    P, SZ, U, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    stages = lib.lda_parquet_stages     # the benchmark's hook, not part of the interface
    stages.restype = I
    stages.argtypes = [P, I, SZ, P, P, SZ, P, SZ, P, SZ, P, U, P]
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "mib": a.mib, "shards": {}}
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    for name, page_bytes in (("pages_1m", 1 << 20), ("pages_64k", 64 << 10)):
        buf, rows, want_out, want_valid = build(np, a.mib, page_bytes, a.pool)
        d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        w_out = torch.from_numpy(want_out).cuda()
        w_valid = torch.from_numpy(want_valid).cuda()
        out, valid = torch.empty_like(w_out), torch.empty_like(w_valid)
        per = torch.zeros(len(rows), dtype=torch.int32, device="cuda")
        packed = rows[(rows[:, 3] >> np.uint64(12) & np.uint64(1)) == 1]
        sizes = packed[:, 2].astype(np.int64)
        r_off = t64(np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)[:-1]]).tolist())
        s_off, s_n, r_n = t64(packed[:, 0].astype(np.int64).tolist()), \
            t64(packed[:, 1].astype(np.int64).tolist()), t64(sizes.tolist())
        other = torch.empty(int(((sizes + 15) // 16 * 16).sum()) + 16, dtype=torch.uint8, device="cuda")
        per2 = torch.zeros(len(packed), dtype=torch.int32, device="cuda")
        e = {"pages": len(rows), "page_bytes": page_bytes, "column_bytes": int(w_out.numel()),
             "slots": int((rows[:, 4] & np.uint64(0xFFFFFFFF))[(rows[:, 3] & np.uint64(15)) != 2].sum()),
             "file_bytes": len(buf), "uncompressed_bytes": int(sizes.sum()), "rounds": []}

        def read():
            d.parquet_decode_batch("gzip", rows, d_in, out, valid, per)

        def plain_read():
            d.decompress_batch("gzip", d_in, s_off, s_n, other, r_off, r_n, per2)

        def part(mask):
            def run():
                rc = stages(d._h, 2, len(rows), rows.ctypes.data_as(P), d_in.data_ptr(), len(buf),
                            out.data_ptr(), out.numel(), valid.data_ptr(), valid.numel(),
                            per.data_ptr(), mask, None)
                assert rc == 0, binding.last_error()
            return run

        def memcpy():
            out.copy_(w_out)

        def exact():
            # the bytes between the columns are never written
            return not per.any().item() and torch.equal(out, w_out) and torch.equal(valid, w_valid)
        for _ in range(a.rounds):
            r = {}

            def keep(key, pair):
                r[key], r[key + "_runs"] = pair
            out.zero_(), valid.zero_()
            keep("read_ms", timed(read, a.steps, a.warmup))
            assert exact()
            keep("plain_read_ms", timed(plain_read, a.steps, a.warmup))
            assert not per2.any().item()
            read()
            out.zero_(), valid.zero_()
            keep("runs_ms", timed(part(2), a.steps, a.warmup))
            keep("expand_ms", timed(part(4), a.steps, a.warmup))
            assert exact()
            keep("no_stage_ms", timed(part(0), a.steps, a.warmup))
            keep("memcpy_ms", timed(memcpy, a.steps, a.warmup))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            read()
            r["call_host_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
            torch.cuda.synchronize()
            e["rounds"].append(r)
        for key in ("read_ms", "plain_read_ms", "runs_ms", "expand_ms", "no_stage_ms", "memcpy_ms"):
            e[key] = min(r[key] for r in e["rounds"])
            e[key + "_max"] = max(max(r[key + "_runs"]) for r in e["rounds"])
        e["call_host_ms"] = min(r["call_host_ms"] for r in e["rounds"])
        e["runs_kernel_ms"] = round(e["runs_ms"] - e["no_stage_ms"], 4)
        e["expand_kernel_ms"] = round(e["expand_ms"] - e["no_stage_ms"], 4)
        e["read_over_plain_read"] = round(e["read_ms"] / e["plain_read_ms"], 4)
        e["runs_kernel_over_memcpy"] = round(e["runs_kernel_ms"] / e["memcpy_ms"], 3)
        e["expand_kernel_over_memcpy"] = round(e["expand_kernel_ms"] / e["memcpy_ms"], 3)
        e["runs_kernel_over_plain_read"] = round(e["runs_kernel_ms"] / e["plain_read_ms"], 4)
        e["memcpy_gb_s"] = round(w_out.numel() / e["memcpy_ms"] / 1e6, 1)
        e["read_gb_s"] = round(w_out.numel() / e["read_ms"] / 1e6, 1)
        res["shards"][name] = e
        del d_in, out, valid, other, w_out, w_valid
    if a.file:
        buf = open(a.file, "rb").read()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            pg = parquet.pages(buf)
            runs.append(round((time.perf_counter() - t0) * 1e3, 3))
        d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        cols = parquet.read_columns(d, buf, d_in)
        res["file"] = {"bytes": len(buf), "pages": len(pg.rows), "columns": len(cols),
                       "column_bytes": pg.out_nbytes, "pages_host_ms": min(runs), "pages_host_ms_runs": runs}
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
