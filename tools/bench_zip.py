"""ZIP archives read on the device: what the directory finder costs on top of
the decode and the CRC batch it feeds, against the calls a caller had before.

    python tools/bench_zip.py [--scale 1] [--steps 7] [--out FILE]

Two archives of tests/datagen.py text written by Python's zipfile at level 6:
`large`, 4096 / scale entries of 64 KiB, and `small`, 65536 / scale entries of
4 KiB (more than 65 535 entries: a ZIP64 end record at scale 1).  Per archive,
device times by HIP events, best of --steps after --warmup (every run is kept
as *_runs: the spread):
  index_ms     libdeflate_amd_zip_index_batch: end record, directory walk,
               local headers, rows - everything but the decode
  zip_ms       libdeflate_amd_zip_decompress_batch, HBM to HBM, with
               max_entries = the entry count (zip_ms_x16: 16 times that)
  batch_ms     libdeflate_amd_decompress_batch(DEFLATE, exact fill) plus
               libdeflate_amd_crc32_batch over the same streams and slots with
               descriptors prepared on the host: the same work with the
               entries given.  zip_ms - batch_ms (finder_ms) is what the
               finder costs
One JSON object on stdout (and --out).
"""
import argparse
import io
import json
import os
import struct
import sys
import zipfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api  # noqa: E402
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
    """-> (archive bytes, [(data_off, csize, usize, crc)] in directory order)"""
    chunks = [datagen.text_chunk(size, 0x21B0 + i) for i in range(min(entries, 256))]
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w", zipfile.ZIP_DEFLATED, compresslevel=6) as zf:
        for i in range(entries):
            zf.writestr(f"e{i:06d}", chunks[i % len(chunks)])
        infos = zf.infolist()
    data = b.getvalue()
    rows = []
    for zi in infos:
        n, x = struct.unpack_from("<HH", data, zi.header_offset + 26)
        rows.append((zi.header_offset + 30 + n + x, zi.compress_size, zi.file_size, zi.CRC))
    return data, rows


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1, help="divide the entry counts by this")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    d = api.Decompressor()
    res = {"device": torch.cuda.get_device_name(0), "archives": {}}
    t = lambda v: torch.tensor(np.asarray(v).astype(np.int64), device="cuda")  # noqa: E731
    for name, entries, size in (("large", 4096 // a.scale, 65536), ("small", 65536 // a.scale, 4096)):
        data, rows = build_archive(entries, size)
        m, n, total = len(rows), len(data), sum(r[2] for r in rows)
        f = torch.frombuffer(bytearray(data) + bytearray(16), dtype=torch.uint8).cuda()
        e = {"file_bytes": n, "entries": m, "output_bytes": total}
        out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
        r5 = torch.zeros(5, dtype=torch.int64, device="cuda")

        def keep(key, pair):
            e[key], e[key + "_runs"] = pair

        # the entries given: decode + CRC with host-known descriptors
        in_off, in_n = t([r[0] for r in rows]), t([r[1] for r in rows])
        out_av = t([r[2] for r in rows])
        out_off = t(np.concatenate([[0], np.cumsum([r[2] for r in rows])[:-1]]))
        results = torch.zeros(m, dtype=torch.int32, device="cuda")
        ain = torch.zeros(m, dtype=torch.int64, device="cuda")
        crcs = torch.zeros(m, dtype=torch.int32, device="cuda")

        def batch():
            d.decompress_batch("deflate", f, in_off, in_n, out, out_off, out_av, results,
                               actual_in=ain)
            api.checksum_batch("crc32", out, out_off, out_av, crcs)
        keep("batch_ms", timed(batch, a.steps, a.warmup))
        assert not results.any().item()
        assert (crcs.cpu().numpy().astype(np.uint32) == np.array([r[3] for r in rows],
                                                                 dtype=np.uint32)).all()
        # the archive calls
        for mult in (1, 16):
            mm = m * mult
            idx = torch.zeros(8 * mm, dtype=torch.int64, device="cuda")
            per = torch.zeros(mm, dtype=torch.int32, device="cuda")
            out.zero_()
            key = "zip_ms" if mult == 1 else f"zip_ms_x{mult}"
            keep(key, timed(lambda: d.decompress_zip_batch(f, mm, out, r5, per, index=idx,
                                                           in_nbytes=n, out_avail=total),
                            a.steps, a.warmup))
            words = r5.cpu().tolist()
            assert words[:2] == [0, m] and words[3] == total, words
            assert not per.any().item()
            got = idx[:8 * m].cpu().numpy().reshape(-1, 8)
            assert got[:, 4].tolist() == [r[0] for r in rows]
            assert got[:, 7].tolist() == out_off.cpu().tolist()
        idx = torch.zeros(8 * m, dtype=torch.int64, device="cuda")
        per = torch.zeros(m, dtype=torch.int32, device="cuda")
        keep("index_ms", timed(lambda: d.index_zip_batch(f, m, r5, per, index=idx, in_nbytes=n),
                               a.steps, a.warmup))
        assert r5.cpu().tolist()[:2] == [0, m]
        keep("batch_ms_2", timed(batch, a.steps, a.warmup))
        floor = min(e["batch_ms"], e["batch_ms_2"])
        e["finder_ms"] = round(e["zip_ms"] - floor, 4)
        e["gb_s_out"] = round(total / e["zip_ms"] / 1e6, 2)
        res["archives"][name] = e
        del out, f
    s = json.dumps(res)
    print(s)
    if a.out:
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
