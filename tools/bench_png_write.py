"""PNG files written on the device: the encode call, its filter kernel alone,
and two yardsticks that are not the code under test.

    python tools/bench_png_write.py [--scale 1] [--steps 7] [--out FILE]

The two shards of tools/bench_png.py (8-bit RGB, tests/png_files.py's smooth
content with noise; --pool distinct images each, repeated): `large`, 4096 /
scale images of 256 x 256, and `small`, the same pixel count as 65536 / scale
images of 64 x 64; adaptive filters, level 6.  *_ms are DEVICE times by HIP
events, timed as tools/bench_zip_write.py times: a spin kernel of a few
milliseconds is queued in front of the first event, so the host has queued the
whole call before the device reaches that event; the two sides of a pair
alternate inside every step; best of --steps after --warmup, every run kept as
*_runs.
  encode_ms      libdeflate_amd_png_encode_batch over all images (plan upload,
                 filter, checksums, compress, assembly), against
  zlib_batch_ms  (a) libdeflate_amd_compress_batch_bounded in zlib format over
                 the same scanlines, filtered beforehand on the host: what a
                 caller could do before, less the filtering and the framing
  filter_ms      the call with the filter kernel alone queued (it includes the
                 plan's upload, as encode_ms does once), against
  memcpy_ms      (b) one device-to-device copy of the pixel bytes
  compress_ms, assemble_ms
                 the call with only the Adler-32, compress and CRC-32 batches,
                 and with only the assembly kernels queued, each on the scratch
                 a full call filled and each with the plan's upload
  encode_host_ms the host clock around the enqueue-only call: plan, pinned copy,
                 launches
The files are checked: the result words, every pool image's file byte for byte
against the CPU model around the object's own zlib stream of it, and the whole
output decoded again by libdeflate_amd_png_decode_batch to the input pixels.
pil_bytes is the size PIL's save(optimize=False) gives the same images, computed
on the CPU, for information only.  One JSON object on stdout (and --out).
"""
import argparse
import ctypes
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import png_files as pf  # noqa: E402
from tools.bench_zip_write import timed_pair  # noqa: E402
from tools.models import png_write as pw  # noqa: E402

LEVEL = 6


def pil_size(pixels, side):
    try:
        from PIL import Image
    except ImportError:
        return None
    buf = io.BytesIO()
    Image.frombytes("RGB", (side, side), pixels).save(buf, "PNG", optimize=False)
    return buf.tell()


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the image counts by this")
    ap.add_argument("--pool", type=int, default=64, help="distinct images per shard")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    c, d = api.Compressor(LEVEL), api.Decompressor()
    lib = binding.load()
    stages = lib.lda_png_encode_stages  # the benchmark's hook, not part of the interface
    P, SZ, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    stages.restype = ctypes.c_int
    stages.argtypes = [P, SZ, P, P, SZ, P, SZ, P, P, U, U, U, P]
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "level": LEVEL,
           "filter": "adaptive", "shards": {}}
    for name, count, side in (("large", 4096 // a.scale, 256), ("small", 65536 // a.scale, 64)):
        pool = min(a.pool, count)
        npix, raw_n = side * side * 3, side * (1 + side * 3)
        pixels = [pf.pixels_smooth(side, side, 8, 2, 0x504E + i) for i in range(pool)]
        raws = [pw.scanlines(px, side, side * 3, 3, pw.ADAPTIVE)[0] for px in pixels]
        reps = -(-count // pool)
        t8 = lambda parts: torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8) \
            .cuda().repeat(reps)[:count * len(parts[0])].contiguous()  # noqa: E731
        d_pix, d_raw = t8(pixels), t8(raws)
        total = count * npix
        rows = api.png_image_rows([(side, side, 3)] * count, [k * npix for k in range(count)])
        bound = c.png_encode_bound(rows)
        out = torch.empty(bound, dtype=torch.uint8, device="cuda")
        r4 = torch.zeros(4, dtype=torch.int64, device="cuda")
        idx = torch.zeros((count, 8), dtype=torch.int64, device="cuda")
        t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
        slot = c.bound("zlib", raw_n)
        slots = torch.empty(count * slot, dtype=torch.uint8, device="cuda")
        z_io, z_in = t64([k * raw_n for k in range(count)]), t64([raw_n] * count)
        z_oo, z_oa = t64([k * slot for k in range(count)]), t64([slot] * count)
        z_on = torch.zeros(count, dtype=torch.int64, device="cuda")
        copy_to = torch.empty(total, dtype=torch.uint8, device="cuda")

        def encode():
            c.encode_png_batch(rows, d_pix, out, r4, idx)

        def zlib_batch():
            c.compress_batch("zlib", d_raw, z_io, z_in, slots, z_oo, z_oa, z_on, max_chunk=raw_n)

        def stage(mask):
            def run():
                rc = stages(c._h, count, rows.ctypes.data_as(P), d_pix.data_ptr(), total,
                            out.data_ptr(), bound, r4.data_ptr(), idx.data_ptr(), pw.ADAPTIVE, 0,
                            mask, None)
                assert rc == 0, binding.last_error()
            return run

        def memcpy():
            copy_to.copy_(d_pix)

        e = {"images": count, "side": side, "pixel_bytes": total, "scanline_bytes": count * raw_n}
        za, zb = timed_pair(encode, zlib_batch, a.steps, a.warmup)
        e["encode_ms"], e["encode_ms_runs"], e["encode_host_ms"] = za
        e["zlib_batch_ms"], e["zlib_batch_ms_runs"], _ = zb
        words = r4.cpu().tolist()
        assert words[0] == 0 and words[2:] == [total, count] and words[1] <= bound, words
        # (a)'s streams: an image above 128 KiB is one workgroup's there, primed
        # segments here, so the sizes differ a little
        assert z_on.min().item() > 0
        e["zlib_batch_bytes"] = int(z_on.sum().item()) + count * (33 + 12 + 12)
        host = out[:words[1]].cpu().numpy()
        index = idx.cpu().numpy().view(np.uint64)
        for k in range(pool):
            f, _, _ = pw.encode([rows[k]], pixels[k], [c.compress("zlib", raws[k])])
            at, size = int(index[k][0]), int(index[k][1])
            assert bytes(host[at:at + size]) == f[0], "image %d is not the model's file" % k
        per = torch.full((count,), -1, dtype=torch.int32, device="cuda")
        back = torch.empty(total, dtype=torch.uint8, device="cuda")
        d.decode_png_batch(out, index, np.arange(count, dtype=np.uint64), back, per,
                           in_nbytes=words[1])
        assert not per.any().item() and torch.equal(back, d_pix), "the files do not decode back"
        del back
        fa, fb = timed_pair(stage(1), memcpy, a.steps, a.warmup)
        e["filter_ms"], e["filter_ms_runs"], _ = fa
        e["memcpy_ms"], e["memcpy_ms_runs"], _ = fb
        # on the scratch the calls above filled: the rest of the call in its two parts
        fa, fb = timed_pair(stage(2), stage(4), a.steps, a.warmup)
        e["compress_ms"], e["compress_ms_runs"], _ = fa
        e["assemble_ms"], e["assemble_ms_runs"], _ = fb
        e["file_bytes"] = words[1]
        sizes = [pil_size(px, side) for px in pixels]
        e["pil_bytes"] = None if None in sizes else sum(sizes[k % pool] for k in range(count))
        e["encode_over_zlib_batch"] = round(e["encode_ms"] / e["zlib_batch_ms"], 4)
        e["filter_over_memcpy"] = round(e["filter_ms"] / e["memcpy_ms"], 4)
        e["filter_over_encode"] = round(e["filter_ms"] / e["encode_ms"], 4)
        e["encode_gb_s"] = round(total / e["encode_ms"] / 1e6, 2)
        e["filter_gb_s"] = round(total / e["filter_ms"] / 1e6, 2)
        e["memcpy_gb_s"] = round(total / e["memcpy_ms"] / 1e6, 2)
        res["shards"][name] = e
        del out, d_pix, d_raw, slots, copy_to
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
