"""tar archives written on the device: the pack kernel against one
device-to-device memcpy of as many bytes as the archive has, and the .tar.gz
call against compress_large_batch alone on the same archive bytes.

    python tools/bench_tar_write.py [--scale 1] [--steps 7] [--rounds 3] [--out FILE]

The two archives of tools/bench_tar.py: `large`, 4096 / scale files of 64 KiB
(256 MiB of data), and `small`, the same bytes in 65536 / scale files of 4 KiB,
text, named as there.  Every entry is read from bytes of its own: d_in holds
data_bytes, the entries back to back, so the pack kernel reads as much from HBM
as it writes entry data.  Per archive and round, device times by HIP events around
the enqueued work, best of --steps after --warmup (every run is kept as *_runs:
the spread).  The calls plan on the host before they enqueue, so the first
event is recorded behind a blocker of device copies long enough to cover the
host's part; what the events bracket is then the device's work alone.
  write_ms        libdeflate_amd_tar_write_batch: the plan's upload and the
                  pack kernel
  write_host_ms   the host's part of that call (plan, pinned block, launch),
                  by the host's clock
  memcpy_ms       one device-to-device copy of archive_bytes: the yardstick (no
                  ratio is fixed); write_over_memcpy is the ratio, next to the
                  reader's gather over its memcpy from profiles/tar_bench.json
                  (reader_gather_over_memcpy: extract minus index)
  targz_ms        libdeflate_amd_targz_compress_batch, gzip at --level
  large_ms        libdeflate_amd_compress_large_batch alone on the archive's
                  bytes; targz_over_large_ms is the difference
One JSON object on stdout (and --out).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api  # noqa: E402
from tests import datagen  # noqa: E402


def timed(fn, steps, warmup, blocker=None):
    """-> (best ms, every run)"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if blocker:
            blocker()
        a.record()
        fn()
        b.record()
        b.synchronize()
        runs.append(round(a.elapsed_time(b), 4))
    return min(runs), runs


def host_ms(fn, steps):
    import torch
    best = None
    for _ in range(steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t) * 1e3
        best = dt if best is None else min(best, dt)
    torch.cuda.synchronize()
    return round(best, 4)


def reference(names, chunks, size):
    """the archive Python's tarfile writes for the same entries"""
    import io
    import tarfile
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=tarfile.PAX_FORMAT) as tf:
        for i, name in enumerate(names):
            ti = tarfile.TarInfo(name)
            ti.size = size
            ti.mtime = 1700000000
            tf.addfile(ti, io.BytesIO(chunks[i % len(chunks)]))
    return b.getvalue()


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the entry counts by this")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--out")
    a = ap.parse_args()
    c = api.Compressor(a.level)
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "level": a.level,
           "archives": {}}
    reader = {}
    try:
        prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "profiles", "tar_bench.json")
        for k, v in json.load(open(prof))["archives"].items():
            # (the extract call includes the index: the gather is their difference)
            reader[k] = round((v["extract_ms"] - v["index_ms"]) / v["memcpy_ms"], 2)
    except (OSError, KeyError, ValueError):
        pass
    for name, entries, size in (("large", 4096 // a.scale, 65536), ("small", 65536 // a.scale, 4096)):
        chunks = [datagen.text_chunk(size, 0x7A20 + i) for i in range(min(entries, 256))]
        names = [f"data/{i // 1000:03d}/e{i:06d}.txt" for i in range(entries)]
        # every entry has bytes of its own in d_in, back to back: all of data_bytes
        # is read from HBM, as the yardstick's copy reads all of the archive (the
        # CONTENTS repeat every 256 entries, as in tools/bench_tar.py)
        base = torch.frombuffer(bytearray(b"".join(chunks)), dtype=torch.uint8).cuda()
        d_in = base.repeat(-(-entries // len(chunks)))[:entries * size].contiguous()
        del base
        offs = np.arange(entries, dtype=np.uint64) * np.uint64(size)
        sizes = np.full(entries, size, dtype=np.uint64)
        packed = c._zip_names(names)
        total = c.tar_write_size(packed, sizes)
        bound = c.bound("gzip", total)
        arc = torch.empty(total, dtype=torch.uint8, device="cuda")
        other = torch.empty(total, dtype=torch.uint8, device="cuda")
        z = torch.empty(bound, dtype=torch.uint8, device="cuda")
        z_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        e = {"archive_bytes": total, "entries": entries, "data_bytes": entries * size,
             "source_bytes": d_in.numel(),
             "rounds": []}

        def write():
            c.write_tar_batch(packed, d_in, offs, sizes, arc, mtime=1700000000, index=False)

        def memcpy():
            other.copy_(arc)

        def targz():
            c.compress_targz_batch("gzip", packed, d_in, offs, sizes, z, z_n, mtime=1700000000,
                                   index=False)

        def large():
            c.compress_large_batch("gzip", arc, z, z_n)
        arc.fill_(0xA5)
        write()
        torch.cuda.synchronize()
        ref = reference(names, chunks, size)
        assert arc.cpu().numpy().tobytes() == ref, "the archive is not tarfile's"
        del ref
        for _ in range(a.rounds):
            r = {}

            def keep(key, pair):
                r[key], r[key + "_runs"] = pair
            keep("memcpy_ms", timed(memcpy, a.steps, a.warmup))
            r["write_host_ms"] = host_ms(write, 3)
            copies = int(2 * r["write_host_ms"] / r["memcpy_ms"]) + 4

            def blocker():
                for _ in range(copies):
                    other.copy_(arc)
            keep("write_ms", timed(write, a.steps, a.warmup, blocker))
            keep("large_ms", timed(large, a.steps, a.warmup, blocker))
            n_large = int(z_n.item())
            keep("targz_ms", timed(targz, a.steps, a.warmup, blocker))
            assert int(z_n.item()) == n_large and n_large > 0
            e["rounds"].append(r)
        for key in ("write_ms", "write_host_ms", "memcpy_ms", "targz_ms", "large_ms"):
            e[key] = min(r[key] for r in e["rounds"])
        e["compressed_bytes"] = n_large
        e["write_gb_s"] = round(total / e["write_ms"] / 1e6, 2)
        e["memcpy_gb_s"] = round(total / e["memcpy_ms"] / 1e6, 2)
        e["write_over_memcpy"] = round(e["write_ms"] / e["memcpy_ms"], 2)
        e["reader_gather_over_memcpy"] = reader.get(name)
        e["targz_over_large_ms"] = round(e["targz_ms"] - e["large_ms"], 4)
        res["archives"][name] = e
        del arc, other, z, d_in
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
