"""PNG files decoded on the device: the index call, the decode call and its
three parts each alone, against two yardsticks that are not the code under
test.

    python tools/bench_png.py [--scale 1] [--steps 7] [--rounds 3] [--out FILE]

Two shards built with tests/png_files.py (8-bit RGB, smooth content with noise,
adaptive filters, one IDAT; --pool distinct images each, repeated): `large`,
4096 / scale images of 256 x 256, and `small`, the same pixel count as 65536 /
scale images of 64 x 64.  Per shard and round, device times by HIP events
around the enqueued work, best of --steps after --warmup (every run is kept as
*_runs: the spread):
  index_ms      libdeflate_amd_png_index_batch over all files
  decode_ms     libdeflate_amd_png_decode_batch over all files: plan upload,
                gather, inflate, unfilter, verdicts
  gather_ms, inflate_ms, unfilter_ms
                the same call with one stage queued (on the scratch a full
                call filled; each includes the plan's upload and the verdict
                kernel, as decode_ms does once)
  zlib_batch_ms libdeflate_amd_decompress_batch over the same zlib streams laid
                out on the host: what a caller could do before, which leaves
                the unfilter undone
  memcpy_ms     one device-to-device copy of the output bytes
One JSON object on stdout (and --out).
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import png_files as pf  # noqa: E402
from tools.models import png_model as pm  # noqa: E402


def timed(fn, steps, warmup):
    """-> (best ms, every run)"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        runs.append(round(a.elapsed_time(b), 4))
    return min(runs), runs


def build_shard(count, side, pool):
    """-> (shard bytes, file offsets, file sizes, zlib streams laid end to end,
    their offsets, their sizes, the pool's pixel bytes)"""
    imgs = [pf.make(side, side, 8, 2, pixels=pf.pixels_smooth(side, side, 8, 2, 0x504E + i))
            for i in range(min(pool, count))]
    zs = []
    for g in imgs:
        res, row = pm.index(g.data)
        ok, z = pm.gather(g.data, row)
        assert res == 0 and ok
        zs.append(z)
    shard, offs, sizes, zbuf, zoffs, zsizes = bytearray(), [], [], bytearray(), [], []
    for i in range(count):
        g, z = imgs[i % len(imgs)], zs[i % len(imgs)]
        offs.append(len(shard))
        sizes.append(len(g.data))
        shard += g.data
        zoffs.append(len(zbuf))
        zsizes.append(len(z))
        zbuf += z
    return bytes(shard), offs, sizes, bytes(zbuf), zoffs, zsizes, [g.pixels for g in imgs]


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the image counts by this")
    ap.add_argument("--pool", type=int, default=64, help="distinct images per shard")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    d = api.Decompressor()
    lib = binding.load()
    stages = lib.lda_png_decode_stages  # the benchmark's hook, not part of the interface
    P, SZ = ctypes.c_void_p, ctypes.c_size_t
    stages.restype = ctypes.c_int
    stages.argtypes = [P, P, SZ, P, SZ, SZ, P, P, SZ, SZ, ctypes.c_uint32, P, P, ctypes.c_uint32, P]
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "shards": {}}
    for name, count, side in (("large", 4096 // a.scale, 256), ("small", 65536 // a.scale, 64)):
        shard, offs, sizes, zbuf, zoffs, zsizes, pixels = build_shard(count, side, a.pool)
        n, npix = len(shard), side * side * 3
        total, raw = count * npix, npix + side
        f = torch.frombuffer(bytearray(shard), dtype=torch.uint8).cuda()
        zf = torch.frombuffer(bytearray(zbuf), dtype=torch.uint8).cuda()
        t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
        d_off, d_n, d_zoff, d_zn = t64(offs), t64(sizes), t64(zoffs), t64(zsizes)
        d_roff = t64([i * raw for i in range(count)])
        d_rav = t64([raw] * count)
        out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
        rawbuf = torch.empty(count * raw + 64, dtype=torch.uint8, device="cuda")
        idx = torch.zeros(8 * count, dtype=torch.int64, device="cuda")
        per = torch.zeros(count, dtype=torch.int32, device="cuda")
        sel = np.arange(count, dtype=np.uint64)
        e = {"file_bytes": n, "images": count, "side": side, "zlib_bytes": len(zbuf),
             "output_bytes": total, "rounds": []}

        def index():
            d.index_png_batch(f, d_off, d_n, idx, per)
        index()
        torch.cuda.synchronize()
        assert not per.any().item()
        rows = idx.cpu().numpy().view(np.uint64).reshape(-1, 8).copy()

        def decode():
            d.decode_png_batch(f, rows, sel, out, per, out_avail=total)

        def part(mask):
            def run():
                rc = stages(d._h, f.data_ptr(), n, rows.ctypes.data_as(P), count, count,
                            sel.ctypes.data_as(P), out.data_ptr(), total, 1, 0, None,
                            per.data_ptr(), mask, None)
                assert rc == 0, binding.last_error()
            return run

        def zlib_batch():
            d.decompress_batch("zlib", zf, d_zoff, d_zn, rawbuf, d_roff, d_rav, per)

        def memcpy():
            out[:total].copy_(rawbuf[:total])

        def verify():
            assert not per.any().item()
            for k in (0, count // 2, count - 1):
                got = out[k * npix:(k + 1) * npix].cpu().numpy().tobytes()
                assert got == pixels[k % len(pixels)]
        for _ in range(a.rounds):
            r = {}

            def keep(key, pair):
                r[key], r[key + "_runs"] = pair
            keep("index_ms", timed(index, a.steps, a.warmup))
            out.zero_()
            keep("decode_ms", timed(decode, a.steps, a.warmup))
            verify()
            keep("gather_ms", timed(part(1), a.steps, a.warmup))
            keep("inflate_ms", timed(part(2), a.steps, a.warmup))
            keep("unfilter_ms", timed(part(4), a.steps, a.warmup))
            decode()
            verify()
            keep("zlib_batch_ms", timed(zlib_batch, a.steps, a.warmup))
            assert not per.any().item()
            keep("memcpy_ms", timed(memcpy, a.steps, a.warmup))
            e["rounds"].append(r)
        keys = ("index_ms", "decode_ms", "gather_ms", "inflate_ms", "unfilter_ms",
                "zlib_batch_ms", "memcpy_ms")
        for key in keys:
            e[key] = min(r[key] for r in e["rounds"])
        e["unfilter_over_inflate"] = round(e["unfilter_ms"] / e["inflate_ms"], 4)
        e["decode_over_zlib_batch"] = round(e["decode_ms"] / e["zlib_batch_ms"], 4)
        e["decode_gb_s"] = round(total / e["decode_ms"] / 1e6, 2)
        e["memcpy_gb_s"] = round(total / e["memcpy_ms"] / 1e6, 2)
        res["shards"][name] = e
        del out, f, zf, rawbuf
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
