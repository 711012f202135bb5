"""One gzip stream from one buffer: libdeflate_amd_compress_large_batch, device
to device, against the host call and against the bare compress batch.

    python tools/bench_compress_large.py [--mib 16,256] [--levels 1,6] [--steps 15]
        [--parent-lib OLD.so] [--out FILE]   (default profiles/r12_bench_compress_large.json)

Workloads: the text of bench.py's single_stream entry (datagen.text_chunk, seed
0x0E110006) and the 64 KiB mix of tests/datagen.py, 16 MiB of each generated
and, for larger sizes, repeated (the repeats lie 16 MiB apart, beyond any
window), gzip.  Per workload, median / min / max over --steps timed runs (of
each of the four calls) after --warmup, in ms:
  device        the new call on a device-resident buffer (HIP events)
  batch         libdeflate_amd_compress_batch of this build over the same input
                cut into independent chunks of the same S, descriptors made
                beforehand, launched like the new call's segments - the bound
                S, 32 MiB of input per launch - so that both take the same
                kernels (HIP events); assembly = device - batch medians: the
                price of descriptors, priming, combine and assembly
  host          libdeflate_gzip_compress of this build, pageable host memory in
                and out (wall clock)
  parent_host   the same call of the library given with --parent-lib (a build
                of the commit before), run alternately with `host`
The device bytes are compared with the host call's, and the parent's host bytes
with this build's.  One JSON object on stdout and in --out, which is rewritten
after every workload.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen  # noqa: E402


def stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
            "max": round(max(ts), 3)}


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def write(res, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


def seg_bytes(n):
    """the segment size of an n-byte call: lda_large_seg_bytes() of
    libdeflate_amd/csrc/large_plan.h, which is the rule - keep this its copy"""
    env = int(os.environ.get("LDA_SEG_BYTES", "0"))
    return env or (16384 if n <= 4 << 20 else 32768 if n <= 8 << 20 else 65536)


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16,256")
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", help="libdeflate_amd.so built from the commit before")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "r12_bench_compress_large.json"))
    a = ap.parse_args()
    lib = binding.load()
    old = None
    if a.parent_lib:
        old = ctypes.CDLL(os.path.abspath(a.parent_lib))
        P, SZ = ctypes.c_void_p, ctypes.c_size_t
        old.libdeflate_alloc_compressor.restype = P
        old.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
        old.libdeflate_free_compressor.argtypes = [P]
        old.libdeflate_gzip_compress.restype = SZ
        old.libdeflate_gzip_compress.argtypes = [P, P, SZ, P, SZ]
    base = {"text": datagen.text_chunk(16 << 20, 0x0E110006),
            "mix": b"".join(datagen.batch(256, 65536, 0x0E110001))}
    res = {"device": torch.cuda.get_device_name(0), "format": "gzip", "steps": a.steps,
           "warmup": a.warmup, "parent_lib": bool(old), "unit": "ms", "workloads": []}
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for kind, seed_bytes in base.items():
        for mib in [int(x) for x in a.mib.split(",")]:
            n = mib << 20
            data = (seed_bytes * (n // len(seed_bytes) + 1))[:n]
            src = np.frombuffer(data, dtype=np.uint8)
            d_in = torch.from_numpy(src.copy()).cuda()
            S = seg_bytes(n)
            m = -(-n // S)
            for level in [int(x) for x in a.levels.split(",")]:
                c = api.Compressor(level)
                bound = c.bound("gzip", n)
                out = torch.empty(bound, dtype=torch.uint8, device="cuda")
                nb = torch.zeros(1, dtype=torch.int64, device="cuda")
                dev = timed(lambda: c.compress_large_batch("gzip", d_in, out, nb),
                            a.steps, a.warmup)
                size = int(nb.item())
                assert size, "the stream did not fit its bound"
                # the same input as independent chunks of S through the batch
                t = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
                slot = c.bound("gzip", S) + 32
                offs, lens = t([k * S for k in range(m)]), t([min(S, n - k * S) for k in range(m)])
                soff, sav, snb = t([k * slot for k in range(m)]), t([slot] * m), t([0] * m)
                slots = torch.empty(m * slot, dtype=torch.uint8, device="cuda")
                per = max(1, (32 << 20) // S)     # lda_large_per_slice()

                def batch():
                    for lo in range(0, m, per):
                        k = slice(lo, min(m, lo + per))
                        c.compress_batch("gzip", d_in, offs[k], lens[k], slots, soff[k], sav[k],
                                         snb[k], max_chunk=S)
                bat = timed(batch, a.steps, a.warmup)
                assert int((snb == 0).sum()) == 0
                del slots
                # host to host, this build and the parent's alternately
                zout, zold = np.zeros(bound, dtype=np.uint8), np.zeros(bound, dtype=np.uint8)
                co = old.libdeflate_alloc_compressor(level) if old else None
                host, parent = [], []
                for it in range(a.steps + 1):
                    t0 = time.perf_counter()
                    zn = lib.libdeflate_gzip_compress(c._h, ptr(src), n, ptr(zout), bound)
                    t1 = time.perf_counter()
                    zo = old.libdeflate_gzip_compress(co, ptr(src), n, ptr(zold), bound) if old else 0
                    t2 = time.perf_counter()
                    if it:
                        host.append((t1 - t0) * 1e3)
                        parent.append((t2 - t1) * 1e3)
                assert zn == size and np.array_equal(zout[:zn], out[:size].cpu().numpy()), \
                    "device bytes differ from the host call's"
                if old:
                    assert zo == zn and np.array_equal(zold[:zo], zout[:zn]), \
                        "the host call's bytes differ from the parent's"
                    old.libdeflate_free_compressor(co)
                w = {"data": kind, "mib": mib, "level": level, "segment_bytes": S, "segments": m,
                     "ratio": round(size / n, 4), "device": stats(dev), "batch": stats(bat),
                     "assembly": round(statistics.median(dev) - statistics.median(bat), 3),
                     "device_gb_s_in": round(n / statistics.median(dev) / 1e6, 2),
                     "host": stats(host),
                     "parent_host": stats(parent) if old else "not measured",
                     "bytes_equal": "device == host" + (" == parent host" if old else "")}
                res["workloads"].append(w)
                print(json.dumps(w), file=sys.stderr, flush=True)
                write(res, a.out)
                c.close()
            del d_in
    print(json.dumps(res))


if __name__ == "__main__":
    main()
