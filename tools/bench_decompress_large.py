"""One large stream from device memory: libdeflate_amd_decompress_large, device
to device, against the host call of the commit before on the same stream.

    python tools/bench_decompress_large.py [--workloads text16,mix16,text256,stored256,fixed256]
        [--steps 15] [--parent-lib OLD.so] [--out FILE]
        (default profiles/r13_bench_decompress_large.json)

Workloads: 16 MiB of the text of bench.py's single_stream entry
(datagen.text_chunk, seed 0x0E110006) and of the 64 KiB mix of tests/datagen.py
at level 6, 256 MiB of the text at level 6 (the 16 MiB repeated: the repeats lie
beyond any window), the same 256 MiB at level 0 (stored blocks) and as Z_FIXED
(static blocks only), all gzip.  Level 6 by the reference where oracle/_ref is
built, by zlib otherwise; levels 0 and Z_FIXED by zlib.  Per workload, median /
min / max over --steps runs after --warmup, wall clock (every call blocks), ms:
  device        the new call, stream and output in device memory
  host          libdeflate_gzip_decompress of this build, pageable host memory
                in and out
  parent_host   the same call of the library given with --parent-lib (a build
                of the commit before), run alternately with `host`: the host
                form was only refactored, a difference outside the spread of
                the runs is a finding
  one_wave      (text16 only) libdeflate_amd_decompress_batch with one chunk:
                what a caller with a stream in device memory had before
The condition is device < parent_host on every workload ("faster": by how
much).  The device call's bytes are compared with the host call's.  One JSON
object on stdout and in --out, which is rewritten after every workload.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen, oracle_util  # noqa: E402


def stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
            "max": round(max(ts), 3)}


def write(res, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


def zstream(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    return co.compress(data) + co.flush()


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="text16,mix16,text256,stored256,fixed256")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", help="libdeflate_amd.so built from the commit before")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "r13_bench_decompress_large.json"))
    a = ap.parse_args()
    lib = binding.load()
    P, SZ = ctypes.c_void_p, ctypes.c_size_t
    old = None
    if a.parent_lib:
        old = ctypes.CDLL(os.path.abspath(a.parent_lib))
        old.libdeflate_alloc_decompressor.restype = P
        old.libdeflate_free_decompressor.argtypes = [P]
        old.libdeflate_gzip_decompress.restype = ctypes.c_int
        old.libdeflate_gzip_decompress.argtypes = [P, P, SZ, P, SZ, ctypes.POINTER(SZ)]
    ref = oracle_util.load_ref()
    level6 = (lambda d: ref.compress("gzip", 6, d)) if ref is not None else (lambda d: zstream(d, 6))
    text = datagen.text_chunk(16 << 20, 0x0E110006)
    mix = b"".join(datagen.batch(256, 65536, 0x0E110001))
    make = {"text16": lambda: (text, level6(text)),
            "mix16": lambda: (mix, level6(mix)),
            "text256": lambda: (text * 16, level6(text * 16)),
            "stored256": lambda: (text * 16, zstream(text * 16, 0)),
            "fixed256": lambda: (text * 16, zstream(text * 16, 6, zlib.Z_FIXED))}
    res = {"device": torch.cuda.get_device_name(0), "format": "gzip", "steps": a.steps,
           "warmup": a.warmup, "parent_lib": bool(old), "unit": "ms",
           "level6_by": "reference" if ref is not None else "zlib", "workloads": []}
    ptr = lambda arr: arr.ctypes.data_as(P)  # noqa: E731
    d = api.Decompressor()
    do = old.libdeflate_alloc_decompressor() if old else None
    for name in a.workloads.split(","):
        data, z = make[name]()
        n = len(data)
        zin = np.frombuffer(z, dtype=np.uint8)
        d_in = torch.from_numpy(zin.copy()).cuda()
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dev = []
        for it in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            r = d.decompress_large("gzip", d_in, d_out)
            t1 = time.perf_counter()
            assert r == (0, len(z), n), (name, r, binding.stream_stats())
            if it >= a.warmup:
                dev.append((t1 - t0) * 1e3)
        st = binding.stream_stats()
        w = {"workload": name, "bytes_in": len(z), "bytes_out": n, "device": stats(dev),
             "device_gb_s_out": round(n / statistics.median(dev) / 1e6, 2),
             "parallel": st["parallel"], "windows": st["windows"],
             "stored_chunks": st["host_chunks"], "repairs": st["repairs"],
             "us_head": st["us_in"], "us_find": st["us_find"], "us_count": st["us_count"],
             "us_queue": st["us_decode"], "us_wait": st["us_out"]}
        if name == "text16":
            t = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
            one_res = torch.zeros(1, dtype=torch.int32, device="cuda")
            args = (t([0]), t([len(z)]), d_out, t([0]), t([n]), one_res)
            one = []
            for it in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d.decompress_batch("gzip", d_in, *args)
                torch.cuda.synchronize()
                one.append((time.perf_counter() - t0) * 1e3)
            assert int(one_res.item()) == 0
            w["one_wave"] = stats(one)
        # host to host, this build and the parent's alternately
        hout, pout = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        host, parent = [], []
        for it in range(a.warmup + a.steps):
            ao = SZ(0)
            t0 = time.perf_counter()
            r = lib.libdeflate_gzip_decompress(d._h, ptr(zin), zin.size, ptr(hout), n, ctypes.byref(ao))
            t1 = time.perf_counter()
            ro = old.libdeflate_gzip_decompress(do, ptr(zin), zin.size, ptr(pout), n,
                                                ctypes.byref(ao)) if old else 0
            t2 = time.perf_counter()
            assert r == 0 and ro == 0
            if it >= a.warmup:
                host.append((t1 - t0) * 1e3)
                parent.append((t2 - t1) * 1e3)
        assert hout.tobytes() == data, "the host call's bytes are wrong"
        assert np.array_equal(d_out.cpu().numpy(), hout), "device bytes differ from the host call's"
        w["host"] = stats(host)
        w["bytes_equal"] = "device == host"
        if old:
            assert np.array_equal(pout, hout), "the parent's bytes differ"
            w["parent_host"] = stats(parent)
            w["faster_than_parent_host"] = round(statistics.median(parent) / statistics.median(dev), 2)
            w["condition_met"] = statistics.median(dev) < statistics.median(parent)
            w["bytes_equal"] += " == parent host"
        else:
            w["parent_host"] = "not measured"
        res["workloads"].append(w)
        print(json.dumps(w), file=sys.stderr, flush=True)
        write(res, a.out)
        del d_in, d_out
    if old:
        old.libdeflate_free_decompressor(do)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
