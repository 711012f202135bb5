"""Predictor-coded deflate strips and tiles (TIFF, GeoTIFF) read on the device:
the call and its unpredict stage alone, against the plain batch decode of the
same streams and a plain copy, in the same run on the same card.

    python tools/bench_tiff.py [--scale 1] [--steps 7] [--rounds 3] [--out FILE]

Three shards of smooth data (random walks, so that the predictor matters;
--pool distinct segments each, repeated):
  rgb8_tiles    4096 / scale tiles of 256 x 256 RGB8, predictor 2, laid out as
                one square mosaic: every tile lands at the image's pitch
  f32_tiles     4096 / scale tiles of 256 x 256 float32, predictor 3, the same
  u16_strips    64 / scale strips of 16 x 32768 uint16, predictor 2, back to back
The streams are written by the writer under test at level 6 and one of them is
checked against Python's zlib and the model.  Per shard and round, device times
by HIP events around the enqueued work, best of --steps after --warmup (every
run is kept as *_runs: the spread):
  read_ms            libdeflate_amd_tiff_decode_batch: plan upload, inflate into
                     scratch, unpredict (predictor 3: and gather), verdicts
  plain_read_ms      libdeflate_amd_decompress_batch of the same streams: the
                     decode a caller pays anyway (its output holds differences)
  unpredict_ms       the call with the unpredict stage alone queued (on the
                     scratch a full call filled; a predictor-3 scan runs in
                     place, so the pixels of such a re-run are not looked at)
  read_no_stage_ms   the same with no stage queued: the host's plan, the upload
                     and the verdict kernel; unpredict_kernel_ms is unpredict_ms
                     less this
  write_ms           libdeflate_amd_tiff_encode_batch
  memcpy_ms          one device-to-device copy of the output bytes: the kernel's
                     yardstick (below about 256 MiB it runs out of the
                     last-level cache and flatters itself)
One JSON object on stdout (and --out; profiles/tiff_bench.json holds the runs
quoted in DESIGN.md).
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
from tools.models import tiff_model as tm  # noqa: E402


def pool_segments(np, width, rows, spp, dtype, pool):
    """`pool` segments of rows x width x spp: random walks in the sample type"""
    out = []
    for i in range(pool):
        rng = np.random.RandomState(0x71FF + i)
        walk = np.cumsum(rng.standard_normal((rows, width, spp)), axis=1) * 3.0 + 1000.0
        out.append(np.ascontiguousarray(walk.astype(dtype)).tobytes())
    return out


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the segment counts by this")
    ap.add_argument("--pool", type=int, default=16, help="distinct segments per shard")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--out")
    a = ap.parse_args()
    d, c = api.Decompressor(), api.Compressor(a.level)
    lib = binding.load()
    P, SZ, U, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    stages = lib.lda_tiff_stages    # the benchmark's hook, not part of the interface
    stages.restype = I
    stages.argtypes = [P, SZ, P, P, SZ, P, SZ, P, U, P]
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "level": a.level, "shards": {}}
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    shards = (("rgb8_tiles", 4096 // a.scale, 256, 256, 3, np.uint8, 2, True),
              ("f32_tiles", 4096 // a.scale, 256, 256, 1, np.float32, 3, True),
              ("u16_strips", max(1, 64 // a.scale), 32768, 16, 1, np.uint16, 2, False))
    for name, count, width, rows_, spp, dtype, pred, mosaic in shards:
        bps = np.dtype(dtype).itemsize
        px, seg_bytes = spp * bps, width * rows_ * spp * bps
        pool = pool_segments(np, width, rows_, spp, dtype, min(a.pool, count))
        total = count * seg_bytes
        # the raw image: a mosaic of side x side tiles, or the strips back to back
        side = int(round(count ** 0.5)) if mosaic else 1
        if mosaic:
            assert side * side == count
            pitch = side * width * px
            offs = [(k // side) * rows_ * pitch + (k % side) * width * px for k in range(count)]
        else:
            pitch = width * px
            offs = [k * seg_bytes for k in range(count)]
        rows = api.tiff_rows(offs, pitch, (width, rows_), None, spp, bps, pred)
        tiles = torch.frombuffer(bytearray(b"".join(pool)), dtype=torch.uint8).cuda()
        tiles = tiles.view(len(pool), rows_, width * px)
        raw = torch.empty(total, dtype=torch.uint8, device="cuda")
        if mosaic:
            img = raw.view(side, rows_, side, width * px)
            for k in range(count):
                img[k // side, :, k % side, :] = tiles[k % len(pool)]
        else:
            raw.view(count, rows_, width * px)[:] = tiles.repeat((count + len(pool) - 1) // len(pool), 1, 1)[:count]
        bound = c.tiff_encode_bound(rows)
        comp = torch.empty(bound, dtype=torch.uint8, device="cuda")
        other = torch.empty(total, dtype=torch.uint8, device="cuda")
        back = torch.empty(total, dtype=torch.uint8, device="cuda")
        result = torch.zeros(4, dtype=torch.int64, device="cuda")
        index = torch.zeros(8 * count, dtype=torch.int64, device="cuda")
        per = torch.zeros(count, dtype=torch.int32, device="cuda")
        e = {"segments": count, "segment_bytes": seg_bytes, "spp": spp, "bps": bps, "predictor": pred,
             "pitch": pitch, "raw_bytes": total, "rounds": []}

        def write():
            c.encode_tiff_batch(rows, raw, comp, result, index)
        write()
        torch.cuda.synchronize()
        assert result[0].item() == 0
        e["stream_bytes"] = int(result[1].item())
        rrows = index.cpu().numpy().view(np.uint64).reshape(-1, 8).copy()
        k = count - 1
        one = comp[int(rrows[k, 0]):int(rrows[k, 0] + rrows[k, 1])].cpu().numpy().tobytes()
        assert tm.undo(zlib.decompress(one), rows_, width, spp, bps, pred) == pool[k % len(pool)]
        s_off, s_n = t64(rrows[:, 0].astype(np.int64).tolist()), t64(rrows[:, 1].astype(np.int64).tolist())
        r_off, r_n = t64([k * seg_bytes for k in range(count)]), t64([seg_bytes] * count)

        def read():
            d.decode_tiff_batch(rrows, comp, back, per, in_nbytes=e["stream_bytes"])

        def plain_read():
            d.decompress_batch("zlib", comp, s_off, s_n, other, r_off, r_n, per)

        def part(mask):
            def run():
                rc = stages(d._h, count, rrows.ctypes.data_as(P), comp.data_ptr(), e["stream_bytes"],
                            back.data_ptr(), total, per.data_ptr(), mask, None)
                assert rc == 0, binding.last_error()
            return run

        def memcpy():
            other.copy_(raw)
        for _ in range(a.rounds):
            r = {}

            def keep(key, pair):
                r[key], r[key + "_runs"] = pair
            back.zero_()
            keep("read_ms", timed(read, a.steps, a.warmup))
            assert not per.any().item() and torch.equal(back, raw)
            keep("plain_read_ms", timed(plain_read, a.steps, a.warmup))
            assert not per.any().item()
            read()
            keep("unpredict_ms", timed(part(2), a.steps, a.warmup))
            if pred != 3:
                assert torch.equal(back, raw)
            keep("read_no_stage_ms", timed(part(0), a.steps, a.warmup))
            keep("write_ms", timed(write, a.steps, a.warmup))
            assert result[0].item() == 0 and result[1].item() == e["stream_bytes"]
            keep("memcpy_ms", timed(memcpy, a.steps, a.warmup))
            e["rounds"].append(r)
        keys = ("read_ms", "plain_read_ms", "unpredict_ms", "read_no_stage_ms", "write_ms", "memcpy_ms")
        for key in keys:
            e[key] = min(r[key] for r in e["rounds"])
            e[key + "_max"] = max(max(r[key + "_runs"]) for r in e["rounds"])
        e["unpredict_kernel_ms"] = round(e["unpredict_ms"] - e["read_no_stage_ms"], 4)
        e["unpredict_kernel_over_memcpy"] = round(e["unpredict_kernel_ms"] / e["memcpy_ms"], 3)
        e["read_over_plain_read"] = round(e["read_ms"] / e["plain_read_ms"], 4)
        e["memcpy_gb_s"] = round(total / e["memcpy_ms"] / 1e6, 1)
        e["unpredict_kernel_gb_s"] = round(total / max(e["unpredict_kernel_ms"], 1e-6) / 1e6, 1)
        e["read_gb_s"] = round(total / e["read_ms"] / 1e6, 1)
        e["write_gb_s"] = round(total / e["write_ms"] / 1e6, 1)
        res["shards"][name] = e
        del raw, comp, other, back, tiles
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
