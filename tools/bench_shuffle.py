"""Byte-shuffled deflate chunks (HDF5, NetCDF-4, Zarr) read and written on the
device: both calls and their transpose stage alone, against the plain batch
calls on the same bytes and a plain copy, in the same run on the same card.

    python tools/bench_shuffle.py [--scale 1] [--steps 7] [--rounds 3] [--out FILE]

Two shards of float data with a smooth signal (a random walk, so that the
shuffle matters; --pool distinct chunks each, repeated): `small`, 4096 / scale
chunks of 64 KiB, and `large`, 256 / scale chunks of 4 MiB, each as float32
(element size 4) and float64 (8).  The streams are zlib, written by the
writer under test at level 6 and checked against Python's zlib and the model.
Per shard, element size and round, device times by HIP events around the
enqueued work, best of --steps after --warmup (every run is kept as *_runs:
the spread):
  read_ms           libdeflate_amd_shuffle_decompress_batch: plan upload,
                    inflate into scratch, unshuffle, verdicts
  plain_read_ms     libdeflate_amd_decompress_batch of the same streams: the
                    decode a caller pays anyway (its output stays shuffled)
  unshuffle_ms      the call with the unshuffle stage alone queued (on the
                    scratch a full call filled)
  read_no_stage_ms  the same with no stage queued: the host's plan, the upload
                    and the verdict kernel; unshuffle_kernel_ms is unshuffle_ms
                    less this
  write_ms          libdeflate_amd_shuffle_compress_batch
  plain_write_ms    libdeflate_amd_compress_batch on the pre-shuffled bytes
  shuffle_ms, write_no_stage_ms, shuffle_kernel_ms
                    as on the read side, of the writer
  memcpy_ms         one device-to-device copy of the raw bytes: the kernels'
                    yardstick (below about 256 MiB it runs out of the
                    last-level cache and flatters itself)
  stream_bytes, unshuffled_stream_bytes
                    the compressed size with the shuffle and with
                    LIBDEFLATE_AMD_SHUF_NO_SHUFFLE on every row
Then `unshuffle_paths`: the unshuffle kernel alone on 4096 / scale chunks of
64 KiB for element sizes of the register paths (1, 2, 4, 8) and of the LDS path
(3, 5, 12, 16, 255, 256), as NO_DEFLATE rows, less a call with no stage queued.
One JSON object on stdout (and --out; profiles/shuffle_bench.json holds the
runs quoted in DESIGN.md).
"""
import argparse
import ctypes
import json
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tools.bench_png import timed  # noqa: E402
from tools.models import shuffle_model as sm  # noqa: E402


def pool_chunks(np, nbytes, es, pool):
    """`pool` chunks of nbytes: a random walk as float32 or float64"""
    out = []
    for i in range(pool):
        rng = np.random.RandomState(0x5AF + i)
        walk = np.cumsum(rng.standard_normal(nbytes // es)) * 0.01 + 20.0
        out.append(walk.astype(np.float32 if es == 4 else np.float64).tobytes())
    return out


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the chunk counts by this")
    ap.add_argument("--pool", type=int, default=16, help="distinct chunks per shard")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--out")
    a = ap.parse_args()
    d, c = api.Decompressor(), api.Compressor(a.level)
    lib = binding.load()
    P, SZ, U, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    # the benchmark's hooks, not part of the interface
    rstages, wstages = lib.lda_shuffle_stages, lib.lda_shuffle_write_stages
    rstages.restype = wstages.restype = I
    rstages.argtypes = [P, I, SZ, P, P, SZ, P, SZ, P, U, P]
    wstages.argtypes = [P, I, SZ, P, P, SZ, P, SZ, P, P, U, P]
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "level": a.level, "shards": {}}
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    for name, count, nbytes in (("small", 4096 // a.scale, 64 << 10), ("large", 256 // a.scale, 4 << 20)):
        for es in (4, 8):
            pool = pool_chunks(np, nbytes, es, min(a.pool, count))
            reps = (count + len(pool) - 1) // len(pool)
            total = count * nbytes
            raw = torch.frombuffer(bytearray(b"".join(pool)), dtype=torch.uint8).cuda().repeat(reps)[:total]
            pre = torch.frombuffer(bytearray(b"".join(sm.shuffle(p, es) for p in pool)),
                                   dtype=torch.uint8).cuda().repeat(reps)[:total]
            offs = [k * nbytes for k in range(count)]
            rows = api.shuffle_rows(offs, [nbytes] * count, es)
            plain_rows = api.shuffle_rows(offs, [nbytes] * count, es, mask=binding.SHUF_NO_SHUFFLE)
            bound = c.shuffle_compress_bound("zlib", rows)
            comp = torch.empty(bound, dtype=torch.uint8, device="cuda")
            other = torch.empty(total, dtype=torch.uint8, device="cuda")
            back = torch.empty(total, dtype=torch.uint8, device="cuda")
            result = torch.zeros(4, dtype=torch.int64, device="cuda")
            index = torch.zeros(6 * count, dtype=torch.int64, device="cuda")
            per = torch.zeros(count, dtype=torch.int32, device="cuda")
            e = {"chunks": count, "chunk_bytes": nbytes, "es": es, "raw_bytes": total, "rounds": []}

            def write(r=rows):
                c.compress_shuffle_batch("zlib", r, raw, comp, result, index)
            write(plain_rows)
            torch.cuda.synchronize()
            e["unshuffled_stream_bytes"] = int(result[1].item())
            write()
            torch.cuda.synchronize()
            assert result[0].item() == 0
            e["stream_bytes"] = int(result[1].item())
            rrows = index.cpu().numpy().view(np.uint64).reshape(-1, 6).copy()
            k = count - 1
            one = comp[int(rrows[k, 0]):int(rrows[k, 0] + rrows[k, 1])].cpu().numpy().tobytes()
            assert sm.unshuffle(zlib.decompress(one), es) == pool[k % len(pool)]
            s_off, s_n = t64(rrows[:, 0].astype(np.int64).tolist()), t64(rrows[:, 1].astype(np.int64).tolist())
            r_off, r_n = t64(offs), t64([nbytes] * count)
            b1 = c.bound("zlib", nbytes)
            slots = torch.empty(count * b1, dtype=torch.uint8, device="cuda")
            sl_off, sl_av = t64([k * b1 for k in range(count)]), t64([b1] * count)
            out_n = torch.zeros(count, dtype=torch.int64, device="cuda")

            def read():
                d.decompress_shuffle_batch("zlib", rrows, comp, back, per, in_nbytes=e["stream_bytes"])

            def plain_read():
                d.decompress_batch("zlib", comp, s_off, s_n, other, r_off, r_n, per)

            def plain_write():
                c.compress_batch("zlib", pre, r_off, r_n, slots, sl_off, sl_av, out_n)

            def rpart(mask):
                def run():
                    rc = rstages(d._h, 1, count, rrows.ctypes.data_as(P), comp.data_ptr(),
                                 e["stream_bytes"], back.data_ptr(), total, per.data_ptr(), mask, None)
                    assert rc == 0, binding.last_error()
                return run

            def wpart(mask):
                def run():
                    rc = wstages(c._h, 1, count, rows.ctypes.data_as(P), raw.data_ptr(), total,
                                 comp.data_ptr(), bound, result.data_ptr(), index.data_ptr(), mask,
                                 None)
                    assert rc == 0, binding.last_error()
                return run

            def memcpy():
                other.copy_(raw)

            def verify():
                assert not per.any().item()
                assert torch.equal(back, raw)
            for _ in range(a.rounds):
                r = {}

                def keep(key, pair):
                    r[key], r[key + "_runs"] = pair
                back.zero_()
                keep("read_ms", timed(read, a.steps, a.warmup))
                verify()
                keep("plain_read_ms", timed(plain_read, a.steps, a.warmup))
                assert not per.any().item() and torch.equal(other, pre)
                read()
                back.zero_()
                keep("unshuffle_ms", timed(rpart(2), a.steps, a.warmup))
                assert torch.equal(back, raw)
                keep("read_no_stage_ms", timed(rpart(0), a.steps, a.warmup))
                keep("write_ms", timed(write, a.steps, a.warmup))
                assert result[0].item() == 0 and result[1].item() == e["stream_bytes"]
                keep("plain_write_ms", timed(plain_write, a.steps, a.warmup))
                # (whole chunks: the same bytes only below the writer's segment rule)
                assert out_n.min().item() > 0
                e["plain_write_stream_bytes"] = int(out_n.sum().item())
                keep("shuffle_ms", timed(wpart(1), a.steps, a.warmup))
                keep("write_no_stage_ms", timed(wpart(0), a.steps, a.warmup))
                keep("memcpy_ms", timed(memcpy, a.steps, a.warmup))
                write()     # the later rounds read what a full call wrote
                torch.cuda.synchronize()
                e["rounds"].append(r)
            keys = ("read_ms", "plain_read_ms", "unshuffle_ms", "read_no_stage_ms", "write_ms",
                    "plain_write_ms", "shuffle_ms", "write_no_stage_ms", "memcpy_ms")
            for key in keys:
                e[key] = min(r[key] for r in e["rounds"])
                e[key + "_max"] = max(max(r[key + "_runs"]) for r in e["rounds"])
            e["unshuffle_kernel_ms"] = round(e["unshuffle_ms"] - e["read_no_stage_ms"], 4)
            e["shuffle_kernel_ms"] = round(e["shuffle_ms"] - e["write_no_stage_ms"], 4)
            e["unshuffle_kernel_over_memcpy"] = round(e["unshuffle_kernel_ms"] / e["memcpy_ms"], 3)
            e["shuffle_kernel_over_memcpy"] = round(e["shuffle_kernel_ms"] / e["memcpy_ms"], 3)
            e["read_over_plain_read"] = round(e["read_ms"] / e["plain_read_ms"], 4)
            e["write_over_plain_write"] = round(e["write_ms"] / e["plain_write_ms"], 4)
            e["memcpy_gb_s"] = round(total / e["memcpy_ms"] / 1e6, 1)
            e["unshuffle_kernel_gb_s"] = round(total / max(e["unshuffle_kernel_ms"], 1e-6) / 1e6, 1)
            e["shuffle_kernel_gb_s"] = round(total / max(e["shuffle_kernel_ms"], 1e-6) / 1e6, 1)
            res["shards"]["%s_es%d" % (name, es)] = e
            del raw, pre, comp, other, back, slots
    # the kernels' paths against each other: 4096 / scale chunks of 64 KiB as
    # NO_DEFLATE rows, which the reader unshuffles straight from the stored bytes -
    # the call is the plan, its upload, the kernel and the verdict kernel - for
    # element sizes of the register paths and of the generic path
    count, nbytes = 4096 // a.scale, 64 << 10
    total = count * nbytes
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    per = torch.zeros(count, dtype=torch.int32, device="cuda")
    offs = [k * nbytes for k in range(count)]
    paths = {}
    for es in (1, 2, 4, 8, 3, 5, 12, 16, 255, 256):
        rows = api.shuffle_rows(offs, [nbytes] * count, es, offs, [nbytes] * count,
                                binding.SHUF_NO_DEFLATE)

        def part(mask, rows=rows):
            def run():
                rc = rstages(d._h, 1, count, rows.ctypes.data_as(P), src.data_ptr(), total,
                             dst.data_ptr(), total, per.data_ptr(), mask, None)
                assert rc == 0, binding.last_error()
            return run
        best = [timed(part(2), a.steps, a.warmup) for _ in range(a.rounds)]
        none = [timed(part(0), a.steps, a.warmup) for _ in range(a.rounds)]
        k = count - 1
        got = dst[k * nbytes:(k + 1) * nbytes].cpu().numpy().tobytes()
        assert got == sm.unshuffle(src[k * nbytes:(k + 1) * nbytes].cpu().numpy().tobytes(), es)
        call, idle = min(b[0] for b in best), min(b[0] for b in none)
        paths["es%d" % es] = {"call_ms": call, "no_stage_ms": idle,
                              "kernel_ms": round(call - idle, 4),
                              "kernel_gb_s": round(total / max(call - idle, 1e-6) / 1e6, 1),
                              "call_ms_runs": [b[1] for b in best]}
    res["unshuffle_paths"] = {"chunks": count, "chunk_bytes": nbytes, "by_es": paths}
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
