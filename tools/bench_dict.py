"""Preset dictionaries on a records corpus: the device batch with and without
a dictionary, against Python's zlib with `zdict` at the same level.

    python tools/bench_dict.py [--records 65536] [--level 6] [--out FILE]

Records are text_chunk()s of 256 B - 4 KiB (tests/datagen.py: records of
different seeds share a vocabulary); the dictionary is 16 KiB cut from
records of other seeds.  Writes one JSON object (stdout, and --out):
  gpu.{plain,dict}.{compress_ms,decompress_ms}  device time of one batch
      (HIP events, best of --steps after --warmup), HBM to HBM
  bytes.{gpu,zlib}_{plain,dict}  total output of the corpus
  cpu_zlib_dict_{compress,decompress}_ms  zlib with zdict on --threads host
      threads (the CPU baseline; zlib releases the GIL)
"""
import argparse
import json
import os
import random
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api  # noqa: E402
from tests import datagen  # noqa: E402


def corpus(count, seed):
    rng = random.Random(seed)
    return [datagen.text_chunk(rng.randrange(256, 4097), seed + i) for i in range(count)]


def dictionary(n, seed):
    out, k = b"", 0
    while len(out) < n:
        out += datagen.text_chunk(4096, seed + k)
        k += 1
    return out[:n]


def pack(chunks, dev, slot=None):
    import torch
    offs, pos = [], 0
    sizes = [len(c) if slot is None else slot(len(c)) for c in chunks]
    for s in sizes:
        offs.append(pos)
        pos += (s + 15) // 16 * 16 + 16
    buf = bytearray(pos + 64)
    if slot is None:
        for o, c in zip(offs, chunks):
            buf[o:o + len(c)] = c
    t = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
    return (t, torch.tensor(offs, dtype=torch.int64, device=dev),
            torch.tensor(sizes, dtype=torch.int64, device=dev))


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--dict-bytes", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    recs = corpus(args.records, 0x2A71)
    d = dictionary(args.dict_bytes, 0x90000)
    td = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev)
    c, dec = api.Compressor(args.level), api.Decompressor()
    data, off, n = pack(recs, dev)
    res = {"records": len(recs), "input_bytes": sum(map(len, recs)), "level": args.level,
           "dict_bytes": len(d), "gpu": {}, "bytes": {}}
    for mode in ("plain", "dict"):
        out, ooff, oav = pack(recs, dev, lambda k: c.bound("zlib", k) + 4)
        on = torch.zeros(len(recs), dtype=torch.int64, device=dev)
        if mode == "dict":
            comp = lambda: c.compress_batch_dict("deflate", td, data, off, n, out, ooff, oav, on)
        else:
            comp = lambda: c.compress_batch("deflate", data, off, n, out, ooff, oav, on)
        cms = timed(comp, args.steps, args.warmup)
        dout, doff, dav = pack(recs, dev, lambda k: k)
        rr = torch.zeros(len(recs), dtype=torch.int32, device=dev)
        ain = torch.zeros(len(recs), dtype=torch.int64, device=dev)
        aout = torch.zeros(len(recs), dtype=torch.int64, device=dev)
        if mode == "dict":
            dcmp = lambda: dec.decompress_batch_dict("deflate", td, out, ooff, on, dout, doff,
                                                     dav, rr, ain, aout)
        else:
            dcmp = lambda: dec.decompress_batch("deflate", out, ooff, on, dout, doff, dav, rr,
                                                ain, aout)
        dms = timed(dcmp, args.steps, args.warmup)
        torch.cuda.synchronize()
        assert int((rr != 0).sum()) == 0 and torch.equal(aout, n), f"{mode}: decode failed"
        res["gpu"][mode] = {"compress_ms": round(cms, 3), "decompress_ms": round(dms, 3)}
        res["bytes"]["gpu_" + mode] = int(on.sum())

    def zc(r, zd):
        co = zlib.compressobj(args.level, zlib.DEFLATED, -15, **({"zdict": zd} if zd else {}))
        return co.compress(r) + co.flush()

    def zd(z):
        do = zlib.decompressobj(-15, zdict=d)
        return do.decompress(z) + do.flush()

    res["bytes"]["zlib_plain"] = sum(len(zc(r, None)) for r in recs)
    with ThreadPoolExecutor(args.threads) as ex:
        t0 = time.perf_counter()
        zs = list(ex.map(lambda r: zc(r, d), recs, chunksize=256))
        t1 = time.perf_counter()
        back = list(ex.map(zd, zs, chunksize=256))
        t2 = time.perf_counter()
    assert back == recs
    res["bytes"]["zlib_dict"] = sum(map(len, zs))
    res["cpu_zlib_dict_compress_ms"] = round((t1 - t0) * 1e3, 2)
    res["cpu_zlib_dict_decompress_ms"] = round((t2 - t1) * 1e3, 2)
    res["cpu_threads"] = args.threads
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
