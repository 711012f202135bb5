"""PNG files decoded on the device to one pixel format (RGB, 8-bit): the new
call against libdeflate_amd_png_decode_batch on the same files, and its convert
stage alone against a device-to-device copy.

    python tools/bench_png_pixels.py [--scale 1] [--steps 7] [--rounds 3] [--out FILE]

Two geometries built with tests/png_files.py (smooth content with noise,
adaptive filters, one IDAT; --pool distinct images per kind, repeated): `large`,
4096 / scale images of 256 x 256, and `small`, 65536 / scale images of 64 x 64;
each as two shards:
  a  every file 8-bit RGB: every selection is direct, the convert kernel is
     not launched
  b  of every ten files seven 8-bit RGB, one 8-bit palette with a tRNS, one
     8-bit grey, one 8-bit RGBA: three in ten go through the convert kernel
Per shard and round, device times by HIP events around the enqueued work, best
of --steps after --warmup (every run is kept as *_runs: the spread):
  pixels_ms     libdeflate_amd_png_decode_pixels_batch to RGB over all files
  native_ms     libdeflate_amd_png_decode_batch over the same files, run back
                to back with it in every round: in shard a the same work, in
                shard b it leaves the files' own formats
  convert_ms    (b) the call with the convert stage alone queued, on the
                scratch a full call filled; includes the plan's upload, the
                zeroing of the flags and the verdict kernel, as pixels_ms does
                once
  no_stage_ms   (b) the same call with no stage queued: that upload, zeroing
                and verdict kernel alone, the part of convert_ms that is not
                the convert kernel
  memcpy_ms     (b) one device-to-device copy of as many bytes as the converted
                selections' output
Results are checked against tools/models/png_pixels_model.py on a sample of
every kind.  One JSON object on stdout (and --out).
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
from tools.models import png_pixels_model as px  # noqa: E402

FMT = px.RGB
KINDS = {"rgb": (8, 2), "palette": (8, 3), "grey": (8, 0), "rgba": (8, 6)}
MIX_B = ["rgb"] * 7 + ["palette", "grey", "rgba"]


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


def build_pool(side, pool):
    out = {}
    for kind, (depth, colour) in KINDS.items():
        trns = bytes((i * 5) & 0xFF for i in range(200)) if kind == "palette" else None
        out[kind] = [pf.make(side, side, depth, colour, trns=trns,
                             pixels=pf.pixels_smooth(side, side, depth, colour, 0x504E + i)).data
                     for i in range(pool)]
    return out


def build_shard(count, mix, pool):
    """-> (shard bytes, file offsets, file sizes, the kind of every file)"""
    shard, offs, sizes, kinds = bytearray(), [], [], []
    for i in range(count):
        kind = mix[i % len(mix)]
        data = pool[kind][(i // len(mix)) % len(pool[kind])]
        offs.append(len(shard))
        sizes.append(len(data))
        kinds.append(kind)
        shard += data
    return bytes(shard), offs, sizes, kinds


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the image counts by this")
    ap.add_argument("--pool", type=int, default=16, help="distinct images per kind")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    d = api.Decompressor()
    lib = binding.load()
    stages = lib.lda_png_pixels_stages  # the benchmark's hook, not part of the interface
    P, SZ, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    stages.restype = ctypes.c_int
    stages.argtypes = [P, P, SZ, P, SZ, SZ, P, U, P, SZ, SZ, U, P, P, U, P]
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "format": "RGB8",
           "shards": {}}
    for name, count, side in (("large", 4096 // a.scale, 256), ("small", 65536 // a.scale, 64)):
        pool = build_pool(side, a.pool)
        for mix_name, mix in (("a", ["rgb"]), ("b", MIX_B)):
            shard, offs, sizes, kinds = build_shard(count, mix, pool)
            n = len(shard)
            f = torch.frombuffer(bytearray(shard), dtype=torch.uint8).cuda()
            t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
            d_off, d_n = t64(offs), t64(sizes)
            idx = torch.zeros(8 * count, dtype=torch.int64, device="cuda")
            per = torch.zeros(count, dtype=torch.int32, device="cuda")
            sel = np.arange(count, dtype=np.uint64)
            d.index_png_batch(f, d_off, d_n, idx, per)
            torch.cuda.synchronize()
            assert not per.any().item()
            rows = idx.cpu().numpy().view(np.uint64).reshape(-1, 8).copy()
            o_px, total = api.png_pixels_out_sizes(rows, sel, FMT)
            o_nat, total_nat = api.png_out_sizes(rows, sel)
            conv = sum(side * side * 3 for k in kinds if k != "rgb")
            out = torch.empty(max(total, total_nat) + 64, dtype=torch.uint8, device="cuda")
            spare = torch.empty(max(conv, 1), dtype=torch.uint8, device="cuda")
            e = {"file_bytes": n, "images": count, "side": side, "output_bytes": int(total),
                 "native_output_bytes": int(total_nat), "converted_images": len(kinds) -
                 kinds.count("rgb"), "converted_output_bytes": conv, "rounds": []}

            def pixels():
                d.decode_png_pixels_batch(f, rows, sel, out, per, FMT, out_avail=total)

            def native():
                d.decode_png_batch(f, rows, sel, out, per, out_avail=total_nat)

            def part(mask):
                def run():
                    rc = stages(d._h, f.data_ptr(), n, rows.ctypes.data_as(P), count, count,
                                sel.ctypes.data_as(P), FMT, out.data_ptr(), total, 1, 0, None,
                                per.data_ptr(), mask, None)
                    assert rc == 0, binding.last_error()
                return run

            def memcpy():
                spare[:conv].copy_(out[:conv])

            def verify():
                assert not per.any().item()
                seen = set()
                for k in list(range(len(mix))) + [count - 1 - i for i in range(len(mix))]:
                    if (kinds[k], k < len(mix)) in seen:
                        continue
                    seen.add((kinds[k], k < len(mix)))
                    want = px.decode(shard, [int(v) for v in rows[k]], FMT)
                    got = out[int(o_px[k]):int(o_px[k + 1])].cpu().numpy().tobytes()
                    assert want == (0, got), (name, mix_name, k, kinds[k])
            for _ in range(a.rounds):
                r = {}

                def keep(key, pair):
                    r[key], r[key + "_runs"] = pair
                keep("native_ms", timed(native, a.steps, a.warmup))
                assert not per.any().item()
                out.zero_()
                keep("pixels_ms", timed(pixels, a.steps, a.warmup))
                verify()
                if conv:
                    # (on the scratch and the direct rooms of the full calls above)
                    keep("convert_ms", timed(part(8), a.steps, a.warmup))
                    verify()
                    keep("no_stage_ms", timed(part(0), a.steps, a.warmup))
                    keep("memcpy_ms", timed(memcpy, a.steps, a.warmup))
                e["rounds"].append(r)
            for key in e["rounds"][0]:
                if not key.endswith("_runs"):
                    e[key] = min(r[key] for r in e["rounds"])
            e["pixels_over_native"] = round(e["pixels_ms"] / e["native_ms"], 4)
            e["pixels_gb_s"] = round(total / e["pixels_ms"] / 1e6, 2)
            if conv:
                e["convert_over_memcpy"] = round(e["convert_ms"] / e["memcpy_ms"], 4)
                e["convert_kernel_ms"] = round(e["convert_ms"] - e["no_stage_ms"], 4)
                e["convert_gb_s"] = round(conv / e["convert_ms"] / 1e6, 2)
                e["memcpy_gb_s"] = round(conv / e["memcpy_ms"] / 1e6, 2)
            res["shards"][name + "_" + mix_name] = e
            del out, f, spare
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
