"""tar archives read on the device: the index against a one-lane serial walk
of the same file, and the extract against one device-to-device memcpy of the
same number of bytes.

    python tools/bench_tar.py [--scale 1] [--steps 7] [--rounds 3] [--out FILE]

Two archives written by Python's tarfile (USTAR_FORMAT): `large`, 4096 / scale
files of 64 KiB (256 MiB of data), and `small`, the same bytes in 65536 / scale
files of 4 KiB.  Per archive and round, device times by HIP events around the
enqueued work, best of --steps after --warmup (every run is kept as *_runs:
the spread):
  index_ms         libdeflate_amd_tar_index_batch: scan, chain, names, rows
  index_serial_ms  the same call with LDA_TAR_SERIAL=1: lda_tar_walk_kernel, one
                   lane and a dependent header per record, in place of the
                   scan and the chain
  extract_ms       libdeflate_amd_tar_extract_batch, HBM to HBM
  memcpy_ms        one device-to-device copy of output_bytes on the same
                   stream: the yardstick of the gather (no ratio is fixed)
One JSON object on stdout (and --out).
"""
import argparse
import io
import json
import os
import sys
import tarfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen  # noqa: E402


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


def build_archive(entries, size):
    """-> (archive bytes, [(offset_data, size)] in file order)"""
    chunks = [datagen.text_chunk(size, 0x7A20 + i) for i in range(min(entries, 256))]
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=tarfile.USTAR_FORMAT) as tf:
        for i in range(entries):
            ti = tarfile.TarInfo(f"data/{i // 1000:03d}/e{i:06d}.txt")
            ti.size = size
            ti.mtime = 1700000000
            tf.addfile(ti, io.BytesIO(chunks[i % len(chunks)]))
    data = b.getvalue()
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:") as tf:
        rows = [(ti.offset_data, ti.size) for ti in tf.getmembers()]
    return data, rows


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the entry counts by this")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    d = api.Decompressor()
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "archives": {}}
    for name, entries, size in (("large", 4096 // a.scale, 65536), ("small", 65536 // a.scale, 4096)):
        data, rows = build_archive(entries, size)
        m, n, total = len(rows), len(data), sum(r[1] for r in rows)
        f = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
        r5 = torch.zeros(5, dtype=torch.int64, device="cuda")
        idx = torch.zeros(8 * m, dtype=torch.int64, device="cuda")
        per = torch.zeros(m, dtype=torch.int32, device="cuda")
        e = {"file_bytes": n, "entries": m, "output_bytes": total, "rounds": []}

        def index():
            d.index_tar_batch(f, m, r5, per, index=idx, in_nbytes=n)

        def extract():
            d.extract_tar_batch(f, m, out, r5, per, index=idx, in_nbytes=n, out_avail=total)

        def memcpy():
            out[:total].copy_(f[:total])

        def verify():
            words = r5.cpu().tolist()
            assert words[:2] == [0, m] and words[3] == total, words
            got = idx.cpu().numpy().reshape(-1, 8)
            assert got[:, 4].tolist() == [r[0] for r in rows]
            assert not per.any().item()
        for _ in range(a.rounds):
            r = {}

            def keep(key, pair):
                r[key], r[key + "_runs"] = pair
            keep("index_ms", timed(index, a.steps, a.warmup))
            verify()
            os.environ["LDA_TAR_SERIAL"] = "1"
            binding.reload_env()
            try:
                keep("index_serial_ms", timed(index, a.steps, a.warmup))
                verify()
            finally:
                os.environ.pop("LDA_TAR_SERIAL", None)
                binding.reload_env()
            out.zero_()
            keep("extract_ms", timed(extract, a.steps, a.warmup))
            verify()
            k = m // 2
            got = out[k * size:(k + 1) * size].cpu().numpy().tobytes()
            assert got == data[rows[k][0]:rows[k][0] + size]
            keep("memcpy_ms", timed(memcpy, a.steps, a.warmup))
            e["rounds"].append(r)
        for key in ("index_ms", "index_serial_ms", "extract_ms", "memcpy_ms"):
            e[key] = min(r[key] for r in e["rounds"])
        e["extract_gb_s"] = round(total / e["extract_ms"] / 1e6, 2)
        e["memcpy_gb_s"] = round(total / e["memcpy_ms"] / 1e6, 2)
        res["archives"][name] = e
        del out, f
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
