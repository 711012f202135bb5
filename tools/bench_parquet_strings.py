"""Parquet BYTE_ARRAY pages read on the device: the _ex call and its kernels
alone, against the plain batch decode of the same gzip members and a plain copy
of the column bytes, in the same run on the same card.

    python tools/bench_parquet_strings.py [--mib 64] [--steps 5] [--rounds 2] [--out FILE]

Synthetic string columns of --mib MiB of string bytes each, made here page by
page (numpy; no Parquet library), lower-case letters, lengths uniform in 0 ..
2 x mean: mean lengths 2, 12 and 100, each PLAIN with 10 % nulls and
dictionary-coded (1000 entries, bit width 10, required), in pages of about 64
KiB, and mean length 12 PLAIN in pages of about 1 MiB.  V1 pages, every body one
gzip member (zlib level 6), levels and indices bit-packed in runs of 63 groups;
--pool distinct pages per column, repeated.  Per shard and round, device times
by HIP events around the enqueued work, best of --steps after --warmup (every
run is kept as *_runs), the protocol of tools/bench_parquet.py:
  read_ms            libdeflate_amd_parquet_decode_batch_ex, the strings' room
                     known: one call
  plain_read_ms      (a) libdeflate_amd_decompress_batch of the same members
  inflate_ms, runs_ms, walk_ms, sum_ms, sum_offsets_ms, sum_offsets_copy_ms
                     the call with those stages alone queued, on the scratch a
                     full call filled; no_stage_ms with none (the host's plan,
                     the upload, the scan and the verdict kernels);
                     *_kernel_ms are the stages less this, offsets_kernel_ms and
                     copy_kernel_ms the differences of the last three
  memcpy_ms          (b) one device-to-device copy of the string bytes
  call_host_ms       wall time of the call's return
One JSON object on stdout (and --out; profiles/parquet_strings_bench.json keeps
every run quoted in DESIGN.md)."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tools.bench_parquet import RUN, gz, packed_runs  # noqa: E402
from tools.bench_png import timed  # noqa: E402
from tools.models import parquet_model as pm  # noqa: E402

S = binding.PARQUET_BYTE_ARRAY
# the offsets kernel turns the lengths the sum kernel left into places, and the
# copy reads places: either is only ever queued behind the stages it reads from
STAGES = (("inflate", 1), ("runs", 2), ("walk", 8), ("sum", 16), ("sum_offsets", 16 | 32),
          ("sum_offsets_copy", 16 | 32 | 64))


def values(np, rng, n, mean):
    """n length-prefixed values -> (the section, the lengths)"""
    lens = rng.randint(0, 2 * mean + 1, size=n).astype(np.int64)
    at = np.concatenate([[0], np.cumsum(lens + 4)])
    sec = rng.randint(97, 123, size=int(at[-1])).astype(np.uint8)
    sec[(at[:-1, None] + np.arange(4)).reshape(-1)] = lens.astype("<u4").view(np.uint8)
    return sec, lens, at


def strip(np, sec, lens, at):
    """the section's values without their prefixes"""
    keep = np.ones(len(sec), dtype=bool)
    keep[(at[:-1, None] + np.arange(4)).reshape(-1)] = False
    return sec[keep]


def plain_page(np, rng, mean, page_bytes):
    """-> (the V1 body, the slots' lengths, their bytes, validity)"""
    n = max(RUN, page_bytes // (4 + mean) // RUN * RUN)
    mask = (rng.random_sample(n) >= 0.1).astype(np.int64)
    sec, lens, at = values(np, rng, int(mask.sum()), mean)
    lev = packed_runs(np, mask, 1)
    slot_lens = np.zeros(n, dtype=np.int64)
    slot_lens[mask == 1] = lens
    return len(lev).to_bytes(4, "little") + lev + sec.tobytes(), slot_lens, strip(np, sec, lens, at), \
        mask.astype(np.uint8)


def dict_pages(np, rng, mean, page_bytes, pool, entries=1000):
    """-> (the dictionary's section, [(body, lengths, bytes, None)])"""
    sec, lens, at = values(np, rng, entries, mean)
    flat, made = strip(np, sec, lens, at), []
    first = np.concatenate([[0], np.cumsum(lens)])
    n = max(RUN, int(page_bytes / 1.25) // RUN * RUN)
    for _ in range(pool):
        idx = rng.randint(0, entries, size=n)
        body = bytes([10]) + packed_runs(np, idx, 10)
        data = np.concatenate([flat[first[i]:first[i + 1]] for i in idx]) if n else flat[:0]
        made.append((body, lens[idx], data, None))
    return sec.tobytes(), entries, made


def build(np, mib, mean, coded, page_bytes, pool):
    """-> (file bytes, rows, expected offsets of every page back to back,
    expected bytes, expected valid)"""
    rng = np.random.RandomState(mean * 7 + coded + page_bytes)
    buf, rows = bytearray(b"PAR1"), []
    if coded:
        dsec, entries, made = dict_pages(np, rng, mean, page_bytes, pool)
        z = gz(dsec)
        rows.append([len(buf), len(z), len(dsec), pm.DICT | 1 << 12 | S, entries, 0, 0, 0])
        buf += z
    else:
        made = [plain_page(np, rng, mean, page_bytes) for _ in range(pool)]
    stored = [gz(m[0]) for m in made]
    per_page = max(1, int(np.mean([len(m[2]) for m in made])))
    count = max(1, (mib << 20) // per_page)
    n = len(made[0][1])
    lens, datas, valids = [], [], []
    for k in range(count):
        body, slot_lens, data, valid = made[k % pool]
        enc = pm.RLE_DICTIONARY if coded else pm.PLAIN
        rows.append([len(buf), len(stored[k % pool]), len(body),
                     pm.DATA_V1 | enc << 4 | 1 << 12 | int(valid is not None) << 13 | S,
                     n, k * n * 8, k * n if valid is not None else 0, 0])
        buf += stored[k % pool]
        lens.append(slot_lens)
        datas.append(data)
        if valid is not None:
            valids.append(valid)
    offsets = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
    return bytes(buf), np.array(rows, dtype=np.uint64), offsets, np.concatenate(datas), \
        np.concatenate(valids) if valids else np.zeros(0, dtype=np.uint8)


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--pool", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    d = api.Decompressor()
    lib = binding.load()
    P, SZ, U, I, U64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64
    stages = lib.lda_parquet_ex_stages      # the benchmark's hook, not part of the interface
    stages.restype = I
    stages.argtypes = [P, I, SZ, P, P, SZ, P, SZ, P, SZ, P, SZ, P, U64, P, U, P]
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "mib": a.mib, "shards": {}}
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    shards = [("len%d_%s_64k" % (m, "dict" if c else "plain"), m, c, 64 << 10)
              for m in (2, 12, 100) for c in (0, 1)] + [("len12_plain_1m", 12, 0, 1 << 20)]
    for name, mean, coded, page_bytes in shards:
        buf, rows, w_off, w_data, w_valid = build(np, a.mib, mean, coded, page_bytes, a.pool)
        d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        slots = len(w_off) - 1
        # consecutive pages share an entry: slots + 1 offsets in all
        out = torch.empty((slots + 1) * 8, dtype=torch.uint8, device="cuda")
        valid = torch.empty(max(len(w_valid), 64), dtype=torch.uint8, device="cuda")
        data = torch.empty(len(w_data), dtype=torch.uint8, device="cuda")
        g_data = torch.from_numpy(w_data).cuda()
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        per = torch.zeros(len(rows), dtype=torch.int32, device="cuda")
        sizes = rows[:, 2].astype(np.int64)
        r_off = t64(np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)[:-1]]).tolist())
        s_off, s_n, r_n = t64(rows[:, 0].astype(np.int64).tolist()), \
            t64(rows[:, 1].astype(np.int64).tolist()), t64(sizes.tolist())
        other = torch.empty(int(((sizes + 15) // 16 * 16).sum()) + 16, dtype=torch.uint8, device="cuda")
        per2 = torch.zeros(len(rows), dtype=torch.int32, device="cuda")
        e = {"pages": len(rows), "page_bytes": page_bytes, "mean_length": mean, "coded": bool(coded),
             "string_bytes": len(w_data), "slots": slots, "file_bytes": len(buf),
             "uncompressed_bytes": int(sizes.sum()), "rounds": []}

        def read():
            d.parquet_decode_batch_ex("gzip", rows, d_in, out, valid, data, total, per)

        def plain_read():
            d.decompress_batch("gzip", d_in, s_off, s_n, other, r_off, r_n, per2)

        def part(mask):
            def run():
                rc = stages(d._h, 2, len(rows), rows.ctypes.data_as(P), d_in.data_ptr(), len(buf),
                            out.data_ptr(), out.numel(), valid.data_ptr(), valid.numel(),
                            data.data_ptr(), data.numel(), total.data_ptr(), 0, per.data_ptr(),
                            mask, None)
                assert rc == 0, binding.last_error()
            return run

        def memcpy():
            data.copy_(g_data)

        def exact():
            return not per.any().item() and total.item() == len(w_data) and \
                torch.equal(out.view(torch.int64).cpu(), torch.from_numpy(w_off)) and \
                torch.equal(data, g_data) and \
                torch.equal(valid[:len(w_valid)].cpu(), torch.from_numpy(w_valid))
        for _ in range(a.rounds):
            r = {}

            def keep(key, pair):
                r[key], r[key + "_runs"] = pair
            out.zero_(), valid.zero_(), data.zero_()
            keep("read_ms", timed(read, a.steps, a.warmup))
            assert exact()
            keep("plain_read_ms", timed(plain_read, a.steps, a.warmup))
            assert not per2.any().item()
            read()
            for key, mask in STAGES:
                keep(key + "_ms", timed(part(mask), a.steps, a.warmup))
            keep("no_stage_ms", timed(part(0), a.steps, a.warmup))
            read()
            assert exact()
            keep("memcpy_ms", timed(memcpy, a.steps, a.warmup))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            read()
            r["call_host_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
            torch.cuda.synchronize()
            e["rounds"].append(r)
        keys = ["read_ms", "plain_read_ms", "no_stage_ms", "memcpy_ms"] + [k + "_ms" for k, _ in STAGES]
        for key in keys:
            e[key] = min(r[key] for r in e["rounds"])
            e[key + "_max"] = max(max(r[key + "_runs"]) for r in e["rounds"])
        e["call_host_ms"] = min(r["call_host_ms"] for r in e["rounds"])
        for key, _ in STAGES[:4]:
            e[key + "_kernel_ms"] = round(e[key + "_ms"] - e["no_stage_ms"], 4)
        e["offsets_kernel_ms"] = round(e["sum_offsets_ms"] - e["sum_ms"], 4)
        e["copy_kernel_ms"] = round(e["sum_offsets_copy_ms"] - e["sum_offsets_ms"], 4)
        e["read_over_plain_read"] = round(e["read_ms"] / e["plain_read_ms"], 4)
        e["walk_kernel_over_inflate"] = round(e["walk_kernel_ms"] / max(e["inflate_kernel_ms"], 1e-4), 4)
        e["copy_kernel_over_memcpy"] = round(e["copy_kernel_ms"] / e["memcpy_ms"], 3)
        e["memcpy_gb_s"] = round(len(w_data) / e["memcpy_ms"] / 1e6, 1)
        e["read_gb_s"] = round(len(w_data) / e["read_ms"] / 1e6, 1)
        res["shards"][name] = e
        del d_in, out, valid, data, g_data, other
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
