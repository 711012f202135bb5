"""The seek index over one plain gzip stream: what building it costs on top of
the decode that happens anyway, and ranged reads through it beside the BGZF
reader on the same data.

    python tools/bench_seek.py [--mib 256] [--steps 5] [--out FILE]
    python tools/bench_seek.py --large-only      # decompress_large alone
    python tools/bench_seek.py --reads-only N --spacing S   # for a kernel trace

--mib MiB of tests/datagen.py text, compressed by zlib at level 6 into one
gzip member (what `gzip -6` writes) and - the yardstick - by
libdeflate_amd_bgzf_compress_batch into a BGZF file.  Reported:
  large_ms       libdeflate_amd_decompress_large, HBM to HBM; blocking, so
                 wall clock: best of --steps after --warmup, and every run.
                 --large-only measures only this, so that another build of
                 the library (LIBDEFLATE_AMD_LIB, e.g. the parent commit's)
                 can be measured by the same code on the same stream.
  index_ms       libdeflate_amd_decompress_large_index at spacings of 64 KiB
                 and 1 MiB, the same way; points, points per MiB
  reads          1, 64 and 4096 ranges of 64 KiB at random offsets in one
                 libdeflate_amd_seek_read_batch per spacing, device time by
                 HIP events, ms and GB/s of output; beside it
                 libdeflate_amd_bgzf_read_batch for the same ranges, and the
                 ratio.  BGZF parses a member once; a seek read parses every
                 touched interval twice and resolves it: slower by design.
--reads-only N does nothing but a few reads of N ranges (for rocprofv3
--kernel-trace --stats: the resolve kernel's share is read off its table).
One JSON object on stdout (and --out).
"""
import argparse
import json
import os
import random
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen  # noqa: E402

PIECE = 65536


def timed(fn, steps, warmup):
    """device time of an enqueue-only call, ms, best of steps"""
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
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    return best


def walled(fn, steps, warmup):
    """wall clock of a blocking call, ms -> (best, every run)"""
    import torch
    for _ in range(warmup):
        fn()
    runs = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        runs.append((time.perf_counter() - t0) * 1e3)
    return round(min(runs), 3), [round(x, 3) for x in runs]


def make_data(mib):
    n = mib << 20
    seg = b"".join(datagen.text_chunk(65536, 0x5EE4 + i) for i in range(256))
    return (seg * (n // len(seg) + 1))[:n]


def gzip_of(data):
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--large-only", action="store_true")
    ap.add_argument("--reads-only", type=int, default=0)
    ap.add_argument("--spacing", type=int, default=65536)
    ap.add_argument("--out")
    a = ap.parse_args()
    data = make_data(a.mib)
    n = len(data)
    z = gzip_of(data)
    d_z = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    d = api.Decompressor()
    res = {"input_bytes": n, "gzip_bytes": len(z), "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(binding.LIB_PATH)}

    def large():
        r = d.decompress_large("gzip", d_z, out, out_avail=n)
        assert r == (0, len(z), n), r

    if not a.reads_only:
        res["large_ms"], res["large_ms_runs"] = walled(large, a.steps, a.warmup)
        res["large_gb_s_out"] = round(n / res["large_ms"] / 1e6, 2)
        assert binding.stream_stats()["parallel"] == 1
    if a.large_only:
        return emit(res, a.out)

    # the yardstick: the same data as a BGZF file, indexed
    c = api.Compressor(6)
    d_plain = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    bz = torch.empty(c.bgzf_bound(n), dtype=torch.uint8, device="cuda")
    nb = torch.zeros(1, dtype=torch.int64, device="cuda")
    c.compress_bgzf_batch(d_plain, bz, nb)
    bz_n = int(nb.item())
    c.close()
    del d_plain
    mm = bz_n // 28 + 1
    r5 = torch.zeros(5, dtype=torch.int64, device="cuda")
    bidx = torch.zeros(2 * (mm + 1), dtype=torch.int64, device="cuda")
    d.index_bgzf_batch(bz, mm, r5, index=bidx, in_nbytes=bz_n)
    words = r5.cpu().tolist()
    assert words[0] == 0 and words[3] == n, words
    brows = bidx[:2 * (words[1] + 1)].cpu().numpy().astype(np.uint64).reshape(-1, 2)
    del bidx

    rng = random.Random(0x5EE4)
    counts = [a.reads_only] if a.reads_only else [1, 64, 4096]
    ranges = {k: np.array([(rng.randrange(0, n - PIECE + 1), PIECE) for _ in range(k)],
                          dtype=np.uint64) for k in counts}
    kmax = max(counts)
    rout = torch.empty(kmax * PIECE + 64, dtype=torch.uint8, device="cuda")
    rres = torch.zeros(kmax, dtype=torch.int32, device="cuda")

    def check(k):
        assert not rres[:k].any().item()
        j = k // 2
        b0 = int(ranges[k][j][0])
        assert rout[j * PIECE:(j + 1) * PIECE].cpu().numpy().tobytes() == data[b0:b0 + PIECE]

    res["spacings"] = {}
    for spacing in ([a.spacing] if a.reads_only else [65536, 1 << 20]):
        e = {}
        made = {}

        def index():
            made["r"] = d.decompress_large_index("gzip", d_z, out, spacing, n // spacing + 2,
                                                 out_avail=n)
            assert made["r"][:3] == (0, len(z), n), made["r"][:3]
        if a.reads_only:
            index()
        else:
            e["index_ms"], e["index_ms_runs"] = walled(index, a.steps, a.warmup)
            e["index_over_large"] = round(e["index_ms"] / res["large_ms"], 3)
        rows, wins = made["r"][3], made["r"][4]
        e["points"] = len(rows) - 2
        e["points_per_mib"] = round(e["points"] / a.mib, 2)
        e["window_bytes"] = e["points"] * binding.SEEK_WINDOW
        e["reads"] = {}
        for k in counts:
            rk = ranges[k]
            ms = timed(lambda: d.seek_read_batch(d_z, rows, wins, rk, rout, rres), a.steps, a.warmup)
            check(k)
            e["reads"][str(k)] = {"seek_ms": round(ms, 4),
                                  "seek_gb_s": round(k * PIECE / ms / 1e6, 3)}
        res["spacings"][str(spacing)] = e
    if not a.reads_only:
        res["bgzf_reads"] = {}
        for k in counts:
            rk = ranges[k]
            ms = timed(lambda: d.read_bgzf_batch(bz, brows, rk, rout, rres, in_nbytes=bz_n),
                       a.steps, a.warmup)
            check(k)
            res["bgzf_reads"][str(k)] = {"bgzf_ms": round(ms, 4),
                                         "bgzf_gb_s": round(k * PIECE / ms / 1e6, 3)}
            for e in res["spacings"].values():
                e["reads"][str(k)]["seek_over_bgzf"] = round(e["reads"][str(k)]["seek_ms"] / ms, 2)
        # decompress_large once more behind everything: the spread of the first figure
        res["large_ms_2"], res["large_ms_2_runs"] = walled(large, a.steps, a.warmup)
    emit(res, a.out)


def emit(res, path):
    s = json.dumps(res)
    print(s)
    if path:
        open(path, "w").write(s + "\n")


if __name__ == "__main__":
    main()
