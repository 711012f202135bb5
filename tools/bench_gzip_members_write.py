"""Files of gzip members written on the device: what
libdeflate_amd_gzip_members_compress_batch costs beside the approximation a
caller had before it - libdeflate_amd_compress_batch in gzip format into slots
followed by libdeflate_amd_compact_batch, with host-made descriptors.

    python tools/bench_gzip_members_write.py [--scale 1] [--steps 7] [--out FILE]

Two files of tests/datagen.py text at level 6 (counts divided by --scale):
  uniform   4096 records of 64 KiB.  Both sides compress the same chunks with
            the same kernels; the difference is the price of the plan, its
            upload, the per-piece CRC-32 batch, the combine and the assembly.
  mixed     4090 such records and four of 16 MiB.  The old way runs every
            record on one workgroup, so the call lasts as long as a 16 MiB
            record takes on one CU; the new call cuts those into segments.
The sides of a case alternate inside every step, best of --steps after
--warmup (every run is kept as *_runs: the spread).  *_ms are DEVICE times by
HIP events: a spin kernel of a few milliseconds is queued in front of the
first event, so the host has queued the whole call before the device reaches
that event and no host time lies between the two events.  *_host_ms is the
host clock around the enqueue-only call(s).  Sides: members (the new call),
base (compress_batch + compact_batch, as the issue of this feature states it)
and base_bounded (the same with libdeflate_amd_compress_batch_bounded, which
the new call's launches correspond to).  added_ms = members_ms - base_ms.

The uniform file is compared with the compacted slots byte for byte (they are
the same members); both files are read back by Python's gzip and compared with
the input.  One JSON object on stdout (and --out).
"""
import argparse
import gzip
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen  # noqa: E402

SPIN_CYCLES = 20_000_000     # of the device clock: several milliseconds
LEVEL = 6


def timed_sides(fns, steps, warmup):
    """-> per side (best device ms, runs, best host ms of the call), the sides
    one after the other in every step"""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    runs, host = [[] for _ in fns], [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(SPIN_CYCLES)      # the device is busy while the host queues
            a.record()
            t0 = time.perf_counter()
            fn()
            host[k].append(round((time.perf_counter() - t0) * 1e3, 4))
            b.record()
            b.synchronize()
            runs[k].append(round(a.elapsed_time(b), 4))
    return [(min(r), r, min(h)) for r, h in zip(runs, host)]


def text_on_device(nbytes):
    """nbytes of text on the device: 256 distinct 64 KiB chunks, repeated (the
    compressor's window is 32 KiB: a repeat 16 MiB back is no match)"""
    import torch
    tile = b"".join(datagen.text_chunk(65536, 0x2C00 + i) for i in range(256))
    t = torch.frombuffer(bytearray(tile), dtype=torch.uint8).cuda()
    return t.repeat(-(-nbytes // t.numel()))[:nbytes].contiguous()


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the record counts by this")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = binding.load()
    res = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "level": LEVEL,
           "steps": a.steps, "warmup": a.warmup, "cases": {}}
    t = lambda v: torch.tensor(np.asarray(v).astype(np.int64), device="cuda")  # noqa: E731

    def case(key, sizes):
        n, total = len(sizes), int(sum(sizes))
        d_in = text_on_device(total)
        offs = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64)
        sizes_a = np.array(sizes, dtype=np.uint64)
        c, cb = api.Compressor(LEVEL), api.Compressor(LEVEL)
        e = {"records": n, "input_bytes": total}
        # the new call
        bound = c.gzip_members_compress_bound(sizes_a)
        out = torch.empty(bound, dtype=torch.uint8, device="cuda")
        r4 = torch.zeros(4, dtype=torch.int64, device="cuda")
        idx = torch.zeros((n + 1, 2), dtype=torch.int64, device="cuda")

        def members():
            c.gzip_members_compress((d_in, offs, sizes_a), None, 0, out=out, result=r4, index=idx)
        # the old way: slots of the gzip bound, then the compaction
        slot = [-(-cb.bound("gzip", int(s)) // 16) * 16 for s in sizes]
        slot_off = np.concatenate(([0], np.cumsum(slot)[:-1]))
        slots = torch.empty(int(sum(slot)), dtype=torch.uint8, device="cuda")
        packed = torch.empty(int(sum(slot)), dtype=torch.uint8, device="cuda")
        io, inn, oo, oa = t(offs), t(sizes_a), t(slot_off), t(slot)
        on = torch.zeros(n, dtype=torch.int64, device="cuda")
        cmp_off = torch.zeros(int(lib.libdeflate_amd_compact_offsets_len(n)), dtype=torch.int64,
                              device="cuda")

        def compact():
            binding.check(lib.libdeflate_amd_compact_batch(
                n, slots.data_ptr(), oo.data_ptr(), on.data_ptr(), packed.data_ptr(),
                cmp_off.data_ptr(), None), "compact_batch")

        def base():
            cb.compress_batch("gzip", d_in, io, inn, slots, oo, oa, on)
            compact()

        def base_bounded():
            cb.compress_batch("gzip", d_in, io, inn, slots, oo, oa, on, max_chunk=int(max(sizes)))
            compact()
        sides = timed_sides((members, base, base_bounded), a.steps, a.warmup)
        for name, (best, runs, host) in zip(("members", "base", "base_bounded"), sides):
            e[name + "_ms"], e[name + "_ms_runs"], e[name + "_host_ms"] = best, runs, host
        e["added_ms"] = round(e["members_ms"] - e["base_ms"], 4)
        e["base_spread_ms"] = round(max(e["base_ms_runs"]) - min(e["base_ms_runs"]), 4)
        e["gb_s_in"] = round(total / e["members_ms"] / 1e6, 2)
        # what was written
        words = r4.cpu().tolist()
        assert words[0] == 0 and words[1] <= bound and words[2:] == [total, n], words
        base_total = int(cmp_off[n].item())
        e["file_bytes"], e["base_file_bytes"] = words[1], base_total
        if max(sizes) < 131072:     # no record is segmented: the very same members
            assert words[1] == base_total
            assert torch.equal(out[:words[1]], packed[:base_total]), "the two files differ"
            assert torch.equal(idx[:n, 0], cmp_off[:n]), "the index is not the compaction's"
        plain = d_in.cpu().numpy().tobytes()
        assert gzip.decompress(out[:words[1]].cpu().numpy().tobytes()) == plain
        assert gzip.decompress(packed[:base_total].cpu().numpy().tobytes()) == plain
        res["cases"][key] = e
        c.close()
        cb.close()

    n = max(4096 // a.scale, 1)
    case("uniform", [65536] * n)
    big = max(4 // a.scale, 1)
    mixed = [65536] * max(n - 6 // a.scale, 1)
    for k in range(big):        # the large records spread evenly among the small ones
        mixed.insert(k * (len(mixed) // big), 16 << 20)
    case("mixed", mixed)
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
