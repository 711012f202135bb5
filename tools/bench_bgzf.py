"""BGZF files: the device call on a device-resident buffer at levels 1 and 6,
split into the compress batch and the file assembly, and the host call.

    python tools/bench_bgzf.py [--mib 256] [--levels 1,6] [--steps 5] [--out FILE]

The input is --mib MiB of tests/datagen.py text.  Per level it reports the
device time (HIP events, best of --steps after --warmup) of
  file_ms      libdeflate_amd_bgzf_compress_batch (descriptors, compress
               batch, scans, copy, EOF member): HBM to HBM
  batch_ms     libdeflate_amd_compress_batch_bounded(BGZF) over the same
               blocks alone (what the file costs without its assembly)
and gb_s_in = input bytes / file_ms, ratio = file bytes / input bytes; then
host_ms / host_gb_s of libdeflate_amd_bgzf_compress (pageable host memory in
and out, wall clock).  One JSON object on stdout (and --out).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen  # noqa: E402


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
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    return best


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    n = a.mib << 20
    seg = b"".join(datagen.text_chunk(65536, 0xB62F + i) for i in range(256))
    data = (seg * (n // len(seg) + 1))[:n]
    B = binding.BGZF_BLOCK
    m = -(-n // B)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    res = {"input_bytes": n, "members": m, "device": torch.cuda.get_device_name(0),
           "levels": {}}
    for level in [int(x) for x in a.levels.split(",")]:
        c = api.Compressor(level)
        out = torch.empty(c.bgzf_bound(n), dtype=torch.uint8, device="cuda")
        nb = torch.zeros(1, dtype=torch.int64, device="cuda")
        file_ms = timed(lambda: c.compress_bgzf_batch(d_in, out, nb), a.steps, a.warmup)
        size = int(nb.item())
        assert size, "the file did not fit its bound"
        # the same blocks through the bounded batch alone
        t = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
        offs = t([k * B for k in range(m)])
        lens = t([min(B, n - k * B) for k in range(m)])
        slots = torch.empty(m * 65536, dtype=torch.uint8, device="cuda")
        soff, sav, snb = t([k * 65536 for k in range(m)]), t([65536] * m), t([0] * m)
        batch_ms = timed(lambda: c.compress_batch("bgzf", d_in, offs, lens, slots, soff, sav,
                                                  snb, max_chunk=B), a.steps, a.warmup)
        del slots
        host_ms = None
        for _ in range(max(1, a.steps // 2)):
            t0 = time.perf_counter()
            f = c.compress_bgzf(data)
            dt = (time.perf_counter() - t0) * 1e3
            host_ms = dt if host_ms is None else min(host_ms, dt)
        assert f is not None and len(f) == size
        assert np.array_equal(np.frombuffer(f, dtype=np.uint8), out[:size].cpu().numpy())
        res["levels"][str(level)] = {
            "file_ms": round(file_ms, 3), "batch_ms": round(batch_ms, 3),
            "assembly_ms": round(file_ms - batch_ms, 3),
            "gb_s_in": round(n / file_ms / 1e6, 2), "ratio": round(size / n, 4),
            "host_ms": round(host_ms, 2), "host_gb_s": round(n / host_ms / 1e6, 2)}
        c.close()
    s = json.dumps(res)
    print(s)
    if a.out:
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
