"""ZIP archives with a few huge entries read on the device:
libdeflate_amd_zip_read_large against libdeflate_amd_zip_read_batch on the same
binary, the same index rows and the same selection (every entry, directory
order).

    python tools/bench_zip_large.py [--scale 1] [--steps 7] [--out FILE]

Three archives written by Python's zipfile (sizes divided by --scale):
  huge_deflated  one entry of 256 MiB of tests/datagen.py text at level 6 among
                 4095 entries of 64 KiB
  huge_stored    one stored entry of 1 GiB
  small_only     4096 entries of 64 KiB: the guard - nothing here is large, so
                 read_zip_large must cost what read_zip_batch costs
Per archive and call, best of --steps after --warmup, every run kept (*_runs:
the spread): *_ms by HIP events around the call on the default stream, and
*_wall_ms by the host's clock around the call and a synchronize - read_zip_large
blocks while its many-wave entries decode.  Every run's results are checked
(all 0), and the two calls' outputs are compared byte for byte.

sweep: read_zip_large on huge_deflated for large_min = 16 KiB .. 4 MiB in powers
of two.  chosen_large_min is the smallest value whose best run lies within the
spread (max - min of its runs) of the best value's: the library's default
(host_common.h).  guard: small_only's large_ms against batch_ms plus the spread
of batch_ms_runs.

One JSON object on stdout and in --out (default profiles/zip_large_bench.json).
"""
import argparse
import io
import json
import os
import sys
import time
import zipfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen  # noqa: E402

MIB = 1 << 20
NEVER = 1 << 40


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn, steps, warmup):
    """-> (best event ms, every run, best wall ms, every run)"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append(round((time.perf_counter() - t0) * 1e3, 4))
        ev.append(round(a.elapsed_time(b), 4))
    return min(ev), ev, min(wall), wall


def text(n, seed):
    """n bytes of datagen text, made 16 MiB at a time"""
    step = 16 * MIB
    return b"".join(datagen.text_chunk(min(step, n - at), seed + at // step)
                    for at in range(0, n, step))


def build(kind, scale):
    b = io.BytesIO()
    small = [datagen.text_chunk(65536, 0x21B0 + i) for i in range(256)]
    with zipfile.ZipFile(b, "w", zipfile.ZIP_DEFLATED, compresslevel=6) as zf:
        if kind == "huge_deflated":
            n = 4096 // scale
            for i in range(n):
                if i == n // 2:
                    zf.writestr("huge", text(256 * MIB // scale, 0x6000))
                else:
                    zf.writestr(f"e{i:06d}", small[i % len(small)])
        elif kind == "huge_stored":
            one = text(16 * MIB, 0x7000)
            zf.writestr(zipfile.ZipInfo("huge"), one * (64 // scale), zipfile.ZIP_STORED)
        else:
            for i in range(4096 // scale):
                zf.writestr(f"e{i:06d}", small[i % len(small)])
    return b.getvalue()


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the sizes by this (1 .. 64)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "zip_large_bench.json"))
    a = ap.parse_args()
    d = api.Decompressor()
    res = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "steps": a.steps,
           "warmup": a.warmup, "piece": binding.ZIP_PIECE, "archives": {}}

    for kind in ("huge_deflated", "huge_stored", "small_only"):
        say(f"{kind}: building")
        data = build(kind, a.scale)
        n = len(data)
        f = torch.frombuffer(bytearray(data) + bytearray(16), dtype=torch.uint8).cuda()
        with zipfile.ZipFile(io.BytesIO(data)) as zf:
            m = len(zf.infolist())
            sizes = [zi.file_size for zi in zf.infolist()]
        del data
        r5 = torch.zeros(5, dtype=torch.int64, device="cuda")
        idx = torch.zeros(8 * m, dtype=torch.int64, device="cuda")
        per = torch.zeros(m, dtype=torch.int32, device="cuda")
        d.index_zip_batch(f, m, r5, per, index=idx, in_nbytes=n)
        torch.cuda.synchronize()
        words = r5.cpu().tolist()
        total = sum(sizes)
        assert words[:2] == [0, m] and words[3] == total, words
        rows = idx.cpu().numpy().reshape(-1, 8).astype(np.uint64)
        assert rows[:, 6].tolist() == sizes
        sel = np.arange(m, dtype=np.uint64)
        e = {"file_bytes": n, "entries": m, "output_bytes": total,
             "largest_entry_bytes": max(sizes), "largest_entry_csize": int(rows[:, 5].max())}
        out_b = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        out_l = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")

        def keep(where, key, quad):
            where[key + "_ms"], where[key + "_ms_runs"] = quad[0], quad[1]
            where[key + "_wall_ms"], where[key + "_wall_ms_runs"] = quad[2], quad[3]

        def batch():
            d.read_zip_batch(f, rows, sel, out_b, per, in_nbytes=n, out_avail=total)

        def large(large_min=0, out=out_l):
            d.read_zip_large(f, rows, sel, out, per, large_min=large_min, in_nbytes=n,
                             out_avail=total)
        say(f"{kind}: read_zip_batch")
        keep(e, "batch", timed(batch, a.steps, a.warmup))
        assert not per.any().item()
        say(f"{kind}: read_zip_large")
        per.fill_(-7)
        keep(e, "large", timed(large, a.steps, a.warmup))
        assert not per.any().item()
        assert torch.equal(out_b, out_l), "the two calls' outputs differ"
        e["many_wave_answered"] = binding.stream_stats()["parallel"] if kind == "huge_deflated" else None
        e["gb_s_out_batch"] = round(total / e["batch_ms"] / 1e6, 2)
        e["gb_s_out_large"] = round(total / e["large_ms"] / 1e6, 2)
        e["speedup"] = round(e["batch_ms"] / e["large_ms"], 2)
        say(f"{kind}: batch {e['batch_ms']} ms, large {e['large_ms']} ms")
        res["archives"][kind] = e

        if kind == "huge_deflated":
            sweep = {}
            for lm in [16384 << i for i in range(9)]:
                s = {}
                per.fill_(-7)
                keep(s, "large", timed(lambda: large(lm), a.steps, a.warmup))
                assert not per.any().item()
                s["many_wave_entries"] = int((rows[:, 5] >= lm).sum())
                sweep[str(lm)] = s
                say(f"  large_min {lm}: {s['large_ms']} ms, {s['many_wave_entries']} many-wave")
            best = min(sweep, key=lambda k: sweep[k]["large_ms"])
            spread = max(sweep[best]["large_ms_runs"]) - min(sweep[best]["large_ms_runs"])
            chosen = min(int(k) for k in sweep
                         if sweep[k]["large_ms"] <= sweep[best]["large_ms"] + spread)
            res["sweep"] = sweep
            res["sweep_best"], res["sweep_spread_ms"] = int(best), round(spread, 4)
            res["chosen_large_min"] = chosen
        if kind == "small_only":
            spread = max(e["batch_ms_runs"]) - min(e["batch_ms_runs"])
            over = e["large_ms"] - (e["batch_ms"] + spread)
            res["guard"] = {"batch_ms": e["batch_ms"], "batch_spread_ms": round(spread, 4),
                            "large_ms": e["large_ms"], "ok": over <= 0,
                            "over_by_ms": round(max(over, 0), 4)}
        del out_b, out_l, f
        torch.cuda.empty_cache()
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
