"""OpenEXR ZIP / ZIPS chunks read and written on the device: the calls and
their transform kernels alone, against the plain batch decode and encode of
the same streams and a plain copy, in the same run on the same card.

    python tools/bench_exr.py [--frames 12] [--steps 7] [--rounds 3] [--out FILE]

--frames frames of 2048 x 1556 RGBA half (smooth ramps with noise in the low
bits, --pool distinct frames, repeated), each an H x W x 4 tensor of R, G, B, A
that the file holds as A, B, G, R planes, in three shards:
  zip      scanline chunks of 16 lines (98 a frame, the last 4 lines)
  zips     scanline chunks of 1 line (1556 a frame)
  tiles64  the same bytes as 64 x 64 tiles (32 x 25 a frame, the last row 20 lines)
The chunks are written by the writer under test at level 6 and one of them is
checked against Python's zlib and the model.  Per shard and round, device times
by HIP events around the enqueued work, best of --steps after --warmup (every
run is kept as *_runs: the spread):
  read_ms            libdeflate_amd_exr_decode_batch: plan upload, inflate into
                     scratch, sums, carries, undo, layout, verdicts
  plain_read_ms      (a) libdeflate_amd_decompress_batch of the same streams
                     into scratch: the decode a caller pays anyway
  undo_ms            the call with the copy, undo and layout kernels alone
                     queued, on the scratch a full call filled
  read_no_stage_ms   the same with no stage queued: the host's plan, the upload
                     and the verdict kernel; undo_kernels_ms is undo_ms less this
  write_ms           libdeflate_amd_exr_encode_batch
  plain_write_ms     (c) libdeflate_amd_compress_batch of the coded bytes
  memcpy_ms          (b) one device-to-device copy of the raw bytes: the
                     kernels' yardstick (below about 256 MiB it runs out of the
                     last-level cache and flatters itself)
One JSON object on stdout (and --out; profiles/exr_bench.json holds the runs
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
from tools.models import exr_model as em  # noqa: E402

WIDTH, HEIGHT, PX = 2048, 1556, 8


def frame(np, i):
    """H x W x 4 half bit patterns: ramps around 1.0 with three noisy low bits"""
    rng = np.random.RandomState(0xE0 + i)
    y, x = np.mgrid[0:HEIGHT, 0:WIDTH]
    out = np.empty((HEIGHT, WIDTH, 4), dtype=np.uint16)
    for ch in range(4):
        out[:, :, ch] = 0x3C00 + ((x * (ch + 1) + y * 3) >> 3) % 0x300 + rng.randint(0, 8, (HEIGHT, WIDTH))
    return out


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--pool", type=int, default=2, help="distinct frames")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--out")
    a = ap.parse_args()
    d, c = api.Decompressor(), api.Compressor(a.level)
    lib = binding.load()
    P, SZ, U, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    stages = lib.lda_exr_stages     # the benchmark's hook, not part of the interface
    stages.restype = I
    stages.argtypes = [P, SZ, P, P, SZ, P, SZ, P, U, P]
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "level": a.level,
           "frames": a.frames, "shards": {}}
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    pool = [frame(np, i) for i in range(min(a.pool, a.frames))]
    fbytes = WIDTH * HEIGHT * PX
    total = a.frames * fbytes
    raw = torch.empty(total, dtype=torch.uint8, device="cuda")
    for f in range(a.frames):
        raw[f * fbytes:(f + 1) * fbytes] = torch.frombuffer(
            bytearray(pool[f % len(pool)].tobytes()), dtype=torch.uint8).cuda()
    pitch = WIDTH * PX
    for name, tw, tl in (("zip", WIDTH, 16), ("zips", WIDTH, 1), ("tiles64", 64, 64)):
        regions = [(f, x0, y0, min(tw, WIDTH - x0), min(tl, HEIGHT - y0)) for f in range(a.frames)
                   for y0 in range(0, HEIGHT, tl) for x0 in range(0, WIDTH, tw)]
        count = len(regions)
        heads = [(x0 // tw, y0 // tl, 0, 0) if tw < WIDTH else (y0,) for _, x0, y0, _, _ in regions]
        rows = api.exr_rows([f * fbytes + y0 * pitch + x0 * PX for f, x0, y0, _, _ in regions], pitch,
                            [(w, l) for _, _, _, w, l in regions], [False] * 4, binding.EXR_PIXELS,
                            [3, 2, 1, 0], None, None, heads)
        sizes = [w * l * PX for _, _, _, w, l in regions]
        bound = c.exr_encode_bound(rows)
        comp = torch.empty(bound, dtype=torch.uint8, device="cuda")
        other = torch.empty(total + 16 * count, dtype=torch.uint8, device="cuda")
        again = torch.empty(bound + 64 * count, dtype=torch.uint8, device="cuda")
        back = torch.empty(total, dtype=torch.uint8, device="cuda")
        result = torch.zeros(4, dtype=torch.int64, device="cuda")
        index = torch.zeros(em.WORDS * count, dtype=torch.int64, device="cuda")
        per = torch.zeros(count, dtype=torch.int32, device="cuda")
        e = {"chunks": count, "chunk_bytes": sizes[0], "raw_bytes": total, "rounds": []}

        def write():
            c.encode_exr_batch(rows, raw, comp, result, index)
        write()
        torch.cuda.synchronize()
        assert result[0].item() == 0
        e["file_bytes"] = int(result[1].item())
        rrows = index.cpu().numpy().view(np.uint64).reshape(-1, em.WORDS).copy()
        e["raw_chunks"] = int((rrows[:, 1] == np.array(sizes, dtype=np.uint64)).sum())
        assert e["raw_chunks"] == 0, "the frames are meant to deflate"
        k = count - 1
        one = comp[int(rrows[k, 0]):int(rrows[k, 0] + rrows[k, 1])].cpu().numpy().tobytes()
        f, x0, y0, w, l = regions[k]
        want = pool[f % len(pool)][y0:y0 + l, x0:x0 + w].tobytes()
        assert b"".join(em.expected(rrows[k], em.undo(zlib.decompress(one)))) == want
        s_off, s_n = t64(rrows[:, 0].astype(np.int64).tolist()), t64(rrows[:, 1].astype(np.int64).tolist())
        r_off = t64(np.concatenate([[0], np.cumsum([(n + 15) // 16 * 16 for n in sizes])[:-1]]).tolist())
        r_n = t64(sizes)
        c_off = t64(np.concatenate([[0], np.cumsum([n + 64 for n in sizes])[:-1]]).tolist())
        c_av = t64([n + 64 for n in sizes])
        c_n = torch.zeros(count, dtype=torch.int64, device="cuda")

        def read():
            d.decode_exr_batch(rrows, comp, back, per, in_nbytes=e["file_bytes"])

        def plain_read():
            d.decompress_batch("zlib", comp, s_off, s_n, other, r_off, r_n, per)

        def plain_write():
            c.compress_batch("zlib", other, r_off, r_n, again, c_off, c_av, c_n)

        def part(mask):
            def run():
                rc = stages(d._h, count, rrows.ctypes.data_as(P), comp.data_ptr(), e["file_bytes"],
                            back.data_ptr(), total, per.data_ptr(), mask, None)
                assert rc == 0, binding.last_error()
            return run

        def memcpy():
            back.copy_(raw)
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
            back.zero_()
            keep("undo_ms", timed(part(2), a.steps, a.warmup))
            assert torch.equal(back, raw)
            keep("read_no_stage_ms", timed(part(0), a.steps, a.warmup))
            keep("write_ms", timed(write, a.steps, a.warmup))
            assert result[0].item() == 0 and result[1].item() == e["file_bytes"]
            keep("plain_write_ms", timed(plain_write, a.steps, a.warmup))
            r["plain_write_bytes"] = int(c_n.sum().item())
            keep("memcpy_ms", timed(memcpy, a.steps, a.warmup))
            e["rounds"].append(r)
        keys = ("read_ms", "plain_read_ms", "undo_ms", "read_no_stage_ms", "write_ms", "plain_write_ms",
                "memcpy_ms")
        for key in keys:
            e[key] = min(r[key] for r in e["rounds"])
            e[key + "_max"] = max(max(r[key + "_runs"]) for r in e["rounds"])
        e["undo_kernels_ms"] = round(e["undo_ms"] - e["read_no_stage_ms"], 4)
        e["undo_kernels_over_memcpy"] = round(e["undo_kernels_ms"] / e["memcpy_ms"], 3)
        e["read_over_plain_read"] = round(e["read_ms"] / e["plain_read_ms"], 4)
        e["write_over_plain_write"] = round(e["write_ms"] / e["plain_write_ms"], 4)
        e["memcpy_gb_s"] = round(total / e["memcpy_ms"] / 1e6, 1)
        e["undo_kernels_gb_s"] = round(total / max(e["undo_kernels_ms"], 1e-6) / 1e6, 1)
        e["read_gb_s"] = round(total / e["read_ms"] / 1e6, 1)
        e["write_gb_s"] = round(total / e["write_ms"] / 1e6, 1)
        res["shards"][name] = e
        del comp, other, again, back
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
