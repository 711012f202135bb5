"""Adam7-interlaced PNG files decoded on the device: the decode call and its
stages each alone, against the same images stored without interlace and a
plain copy of the output, in the same run on the same card.

    python tools/bench_png_adam7.py [--scale 1] [--steps 7] [--rounds 3] [--out FILE]

Two shards built with tests/png_adam7_files.py and tests/png_files.py (8-bit
RGB, smooth content with noise, adaptive filters, one IDAT; --pool distinct
images each, repeated): `large`, 4096 / scale images of 256 x 256, and `small`,
the same pixel count as 65536 / scale images of 64 x 64 - every image once
interlaced and once not.  Per shard and round, device times by HIP events
around the enqueued work, best of --steps after --warmup (every run is kept as
*_runs: the spread):
  index_ms        libdeflate_amd_png_index_batch_ex with PNG_ADAM7 over the
                  interlaced files
  decode_ms       libdeflate_amd_png_decode_batch_ex (format 0) over them: plan
                  upload, gather, inflate, unfilter over the pass units,
                  deinterlace, verdicts
  twin_decode_ms  libdeflate_amd_png_decode_batch over the non-interlaced twins
  gather_ms, inflate_ms, unfilter_ms, deinterlace_ms
                  the interlaced call with one stage queued (on the scratch a
                  full call filled; each includes the plan's upload, one memset
                  and the verdict kernel, as decode_ms does once)
  no_stage_ms     the same with no stage queued: what every *_ms of a single
                  stage carries besides its kernel (the host's plan, the upload,
                  the memset, the verdict kernel); deinterlace_kernel_ms is
                  deinterlace_ms less this
  memcpy_ms       one device-to-device copy of the output bytes: the
                  deinterlace kernel's yardstick
One JSON object on stdout (and --out; profiles/png_adam7_bench.json holds the
runs quoted in DESIGN.md).
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import png_adam7_files as p7  # noqa: E402
from tests import png_files as pf  # noqa: E402
from tools.bench_png import timed  # noqa: E402


def build_shard(count, side, pool):
    """-> (interlaced shard, its offsets and sizes, the twins' shard, offsets
    and sizes, the pool's pixel bytes)"""
    pixels = [pf.pixels_smooth(side, side, 8, 2, 0x504E + i) for i in range(min(pool, count))]
    inter = [p7.make7(side, side, 8, 2, pixels=p).data for p in pixels]
    plain = [pf.make(side, side, 8, 2, pixels=p).data for p in pixels]
    shards = []
    for files in (inter, plain):
        shard, offs, sizes = bytearray(), [], []
        for i in range(count):
            g = files[i % len(files)]
            offs.append(len(shard))
            sizes.append(len(g))
            shard += g
        shards += [bytes(shard), offs, sizes]
    return shards + [pixels]


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
    stages = lib.lda_png_adam7_stages  # the benchmark's hook, not part of the interface
    P, SZ, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    stages.restype = ctypes.c_int
    stages.argtypes = [P, P, SZ, P, SZ, SZ, P, U, P, SZ, SZ, U, P, P, U, P]
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "shards": {}}
    for name, count, side in (("large", 4096 // a.scale, 256), ("small", 65536 // a.scale, 64)):
        shard7, offs7, sizes7, shard, offs, sizes, pixels = build_shard(count, side, a.pool)
        npix = side * side * 3
        total = count * npix
        f7 = torch.frombuffer(bytearray(shard7), dtype=torch.uint8).cuda()
        f = torch.frombuffer(bytearray(shard), dtype=torch.uint8).cuda()
        t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
        out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
        other = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
        idx = torch.zeros(8 * count, dtype=torch.int64, device="cuda")
        per = torch.zeros(count, dtype=torch.int32, device="cuda")
        sel = np.arange(count, dtype=np.uint64)
        e = {"file_bytes": len(shard7), "twin_file_bytes": len(shard), "images": count,
             "side": side, "output_bytes": total, "rounds": []}
        d_off7, d_n7, d_off, d_n = t64(offs7), t64(sizes7), t64(offs), t64(sizes)

        def index():
            d.index_png_batch_ex(f7, d_off7, d_n7, idx, per, flags=binding.PNG_ADAM7)
        d.index_png_batch(f, d_off, d_n, idx, per)
        torch.cuda.synchronize()
        assert not per.any().item()
        rows = idx.cpu().numpy().view(np.uint64).reshape(-1, 8).copy()
        index()
        torch.cuda.synchronize()
        assert not per.any().item()
        rows7 = idx.cpu().numpy().view(np.uint64).reshape(-1, 8).copy()
        assert ((rows7[:, 3] >> np.uint64(16)) & np.uint64(0xFF) == 1).all()

        def decode():
            d.decode_png_batch_ex(f7, rows7, sel, out, per, 0, flags=binding.PNG_ADAM7,
                                  out_avail=total)

        def twin_decode():
            d.decode_png_batch(f, rows, sel, out, per, out_avail=total)

        def part(mask):
            def run():
                rc = stages(d._h, f7.data_ptr(), len(shard7), rows7.ctypes.data_as(P), count, count,
                            sel.ctypes.data_as(P), 0, out.data_ptr(), total, 1, binding.PNG_ADAM7,
                            None, per.data_ptr(), mask, None)
                assert rc == 0, binding.last_error()
            return run

        def memcpy():
            other[:total].copy_(out[:total])

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
            keep("twin_decode_ms", timed(twin_decode, a.steps, a.warmup))
            verify()
            out.zero_()
            keep("decode_ms", timed(decode, a.steps, a.warmup))
            verify()
            keep("gather_ms", timed(part(1), a.steps, a.warmup))
            keep("inflate_ms", timed(part(2), a.steps, a.warmup))
            keep("unfilter_ms", timed(part(4), a.steps, a.warmup))
            keep("deinterlace_ms", timed(part(8), a.steps, a.warmup))
            keep("no_stage_ms", timed(part(0), a.steps, a.warmup))
            decode()
            verify()
            keep("memcpy_ms", timed(memcpy, a.steps, a.warmup))
            e["rounds"].append(r)
        keys = ("index_ms", "decode_ms", "twin_decode_ms", "gather_ms", "inflate_ms",
                "unfilter_ms", "deinterlace_ms", "no_stage_ms", "memcpy_ms")
        for key in keys:
            e[key] = min(r[key] for r in e["rounds"])
        e["decode_over_twin_decode"] = round(e["decode_ms"] / e["twin_decode_ms"], 4)
        e["deinterlace_kernel_ms"] = round(e["deinterlace_ms"] - e["no_stage_ms"], 4)
        e["deinterlace_kernel_over_memcpy"] = round(e["deinterlace_kernel_ms"] / e["memcpy_ms"], 4)
        e["decode_gb_s"] = round(total / e["decode_ms"] / 1e6, 2)
        e["memcpy_gb_s"] = round(total / e["memcpy_ms"] / 1e6, 2)
        res["shards"][name] = e
        del out, other, f, f7
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
