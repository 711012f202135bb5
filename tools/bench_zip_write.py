"""ZIP archives written on the device: what the assembly - the plan and its
upload, the per-piece CRC-32, the decision, headers, directory and the copy
into place - adds to the compress calls a caller had before.

    python tools/bench_zip_write.py [--scale 1] [--steps 7] [--out FILE]

Cases (sizes divided by --scale), the two sides of a case alternating inside
every step, best of --steps after --warmup (every run is kept as *_runs: the
spread).  *_ms are DEVICE times by HIP events: a spin kernel of a few
milliseconds is queued in front of the first event, so the host has queued the
whole call before the device reaches that event and no host time lies between
the two events.  *_host_ms is the host clock around the enqueue-only call
itself (names, offsets and sizes handed over as prepared numpy arrays): the
plan, its copy into the pinned block and the launches.
  text_l1, text_l6   4096 entries of 64 KiB of tests/datagen.py text at level 1
                     and 6: libdeflate_amd_zip_compress_batch against
                     libdeflate_amd_compress_batch_bounded (DEFLATE) alone on
                     the same bytes into slots of its own
  one_256m_l6        one entry of 256 MiB at level 6 against
                     libdeflate_amd_compress_large_batch (DEFLATE) alone
  store_1g           one entry of 1 GiB under LIBDEFLATE_AMD_ZIP_STORE against
                     a device-to-device copy of the same size
zip_ms - base_ms (added_ms) is the device time the archive adds.  Every
archive's result words are checked, the sizes against the base call's, and the
archive is read back by libdeflate_amd_zip_decompress_batch - every entry's
CRC-32 checked there - and compared with the input byte for byte.  One JSON
object on stdout (and --out).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen  # noqa: E402


SPIN_CYCLES = 20_000_000     # of the device clock: several milliseconds


def timed_pair(fa, fb, steps, warmup):
    """-> per side (best device ms, runs, best host ms of the call), a then b
    in every step"""
    import time
    import torch
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    runs, host = ([], []), ([], [])
    for _ in range(steps):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(SPIN_CYCLES)      # the device is busy while the host queues
            a.record()
            t0 = time.perf_counter()
            fn()
            host[k].append(round((time.perf_counter() - t0) * 1e3, 4))
            b.record()
            b.synchronize()
            runs[k].append(round(a.elapsed_time(b), 4))
    return (min(runs[0]), runs[0], min(host[0])), (min(runs[1]), runs[1], min(host[1]))


def text_on_device(nbytes):
    """nbytes of text on the device: 256 distinct 64 KiB chunks, repeated (the
    compressor's window is 32 KiB: a repeat 16 MiB back is no match)"""
    import torch
    tile = b"".join(datagen.text_chunk(65536, 0x21C0 + i) for i in range(256))
    t = torch.frombuffer(bytearray(tile), dtype=torch.uint8).cuda()
    return t.repeat(-(-nbytes // t.numel()))[:nbytes].contiguous()


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the sizes by this")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "cases": {}}
    r4 = torch.zeros(4, dtype=torch.int64, device="cuda")
    t = lambda v: torch.tensor(np.asarray(v).astype(np.int64), device="cuda")  # noqa: E731

    def case(key, level, names, d_in, offs, sizes, flags, base):
        """base() is the call the archive is set against; it returns the bytes
        of DEFLATE it produced, or None"""
        c = api.Compressor(level)
        bound = c.zip_bound(names, sizes, flags)
        out = torch.empty(bound, dtype=torch.uint8, device="cuda")
        e = {"entries": len(names), "input_bytes": int(sum(sizes)), "level": level}
        fb = base(c)
        pair = c._zip_names(names)      # encoded once, outside the timed call
        offs_a, sizes_a = np.array(offs, dtype=np.uint64), np.array(sizes, dtype=np.uint64)
        za, zb = timed_pair(
            lambda: c.compress_zip_batch(pair, d_in, offs_a, sizes_a, out, r4, flags=flags),
            fb, a.steps, a.warmup)
        e["zip_ms"], e["zip_ms_runs"], e["zip_host_ms"] = za
        e["base_ms"], e["base_ms_runs"], e["base_host_ms"] = zb
        words = r4.cpu().tolist()
        assert words[0] == 0 and words[1] <= bound, words
        overhead = sum(30 + 46 + 2 * len(x) for x in names) + 22
        got = fb.produced()
        if got is not None:     # the archive holds exactly the base call's streams
            assert words[3] == len(names) and words[1] == got + overhead, (words, got)
        else:
            assert words[3] == 0 and words[1] == sum(sizes) + overhead == bound, words
        # the archive read back: every entry's CRC-32 and every byte
        d = api.Decompressor()
        m, total = len(names), int(sum(sizes))
        back = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
        r5 = torch.zeros(5, dtype=torch.int64, device="cuda")
        per = torch.zeros(m, dtype=torch.int32, device="cuda")
        d.decompress_zip_batch(out, m, back, r5, per, in_nbytes=words[1], out_avail=total)
        assert r5.cpu().tolist()[:2] == [0, m] and not per.any().item()
        at = 0
        for o, sz in zip(offs, sizes):
            assert torch.equal(back[at:at + sz], d_in[o:o + sz]), "archive differs from its input"
            at += sz
        d.close()
        del back
        e["archive_bytes"] = words[1]
        e["added_ms"] = round(e["zip_ms"] - e["base_ms"], 4)
        e["gb_s_in"] = round(sum(sizes) / e["zip_ms"] / 1e6, 2)
        res["cases"][key] = e
        c.close()

    # 4096 x 64 KiB
    n = max(4096 // a.scale, 1)
    d_in = text_on_device(n * 65536)
    names = [b"e%06d" % k for k in range(n)]
    offs, sizes = [k * 65536 for k in range(n)], [65536] * n
    for level in (1, 6):
        def batch(c):
            slot = c.bound("deflate", 65536)
            slots = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
            io, inn = t(offs), t(sizes)
            oo, oa = t([k * slot for k in range(n)]), t([slot] * n)
            on = torch.zeros(n, dtype=torch.int64, device="cuda")

            def f():
                c.compress_batch("deflate", d_in, io, inn, slots, oo, oa, on, max_chunk=65536)
            f.produced = lambda: int(on.sum().item())
            return f
        case(f"text_l{level}", level, names, d_in, offs, sizes, 0, batch)
    del d_in

    # one large entry
    big = (256 << 20) // a.scale
    d_in = text_on_device(big)

    def large(c):
        slots = torch.empty(c.bound("deflate", big), dtype=torch.uint8, device="cuda")
        on = torch.zeros(1, dtype=torch.int64, device="cuda")

        def f():
            c.compress_large_batch("deflate", d_in, slots, on)
        f.produced = lambda: int(on.item())
        return f
    case("one_256m_l6", 6, [b"big.txt"], d_in, [0], [big], 0, large)
    del d_in

    # stored
    big = (1 << 30) // a.scale
    d_in = text_on_device(big)

    def copy(c):
        dst = torch.empty(big, dtype=torch.uint8, device="cuda")

        def f():
            dst.copy_(d_in)
        f.produced = lambda: None
        return f
    case("store_1g", 6, [b"big.bin"], d_in, [0], [big], binding.ZIP_STORE, copy)
    s = json.dumps(res)
    print(s)
    if a.out:
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
