"""Files of concatenated gzip members read on the device: what the member
finder costs on top of the decode it feeds, against the calls a caller had
before.

    python tools/bench_gzip_members.py [--mib 256] [--steps 7] [--out FILE]

Two files of the same --mib MiB of tests/datagen.py text, compressed at level
6 by libdeflate_amd_compress_batch(GZIP) and packed back to back: `small`,
members of 8 - 24 KiB of input (the WARC / BAM-record shape), and `large`,
members of 256 KiB.  Per file, device times by HIP events, best of --steps
after --warmup (every run is kept as *_runs: the spread):
  file_ms_x1/2/16  (a) libdeflate_amd_gzip_members_decompress_batch, HBM to
                   HBM, with max_members = the member count, 2 x and 16 x it
  batch_ms         (b) libdeflate_amd_decompress_batch(GZIP) over exact
                   descriptors prepared on the host, exact fill: the same
                   decode with the members given - the floor
  packed_ms        (c) libdeflate_amd_decompress_batch_packed over offsets
                   prepared on the host: count + decode without the finder.
                   (a) - (c) is what the finder costs, (c) - (b) what a count
                   pass costs
  index_ms         libdeflate_amd_gzip_members_index_batch: (a) less the decode
  host_ms          (d) libdeflate_amd_gzip_decompress_members on the same
                   bytes from host memory, wall clock: the member-after-member
                   loop
  scan_ms          (e) the candidate scan's count pass alone, and scan_gb_s:
                   input bytes per second, scan_hbm_share: of the 6.29 TB/s a
                   copy kernel reaches on this device
One JSON object on stdout (and --out).
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen  # noqa: E402

HBM_COPY_TB_S = 6.29    # measured float4 copy on an MI355X


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


def build_file(d_in, n, cuts, level=6):
    """the ranges `cuts` of d_in as gzip members back to back -> (file as a
    uint8 CUDA tensor with 16 spare bytes, its size, member offsets[m + 1])"""
    import torch
    c = api.Compressor(level)
    m = len(cuts)
    slot = (c.bound("gzip", max(b for _, b in cuts)) + 15) & ~15
    t = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    slots = torch.empty(m * slot, dtype=torch.uint8, device="cuda")
    snb = t([0] * m)
    soff = t([i * slot for i in range(m)])
    c.compress_batch("gzip", d_in, t([a for a, _ in cuts]), t([b for _, b in cuts]), slots,
                     soff, t([slot] * m), snb)
    torch.cuda.synchronize()
    assert snb.min().item() > 0, "a member did not fit its slot"
    packed, offs = api.compact_batch(slots, soff, snb)
    torch.cuda.synchronize()
    offs = offs.cpu().tolist()
    size = offs[m]
    f = torch.cat([packed[:size], torch.zeros(16, dtype=torch.uint8, device="cuda")])
    c.close()
    return f, size, offs


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    n = a.mib << 20
    seg = b"".join(datagen.text_chunk(65536, 0x62F0 + i) for i in range(256))
    data = (seg * (n // len(seg) + 1))[:n]
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    rng, small, k = random.Random(0x62F0), [], 0
    while k < n:
        size = min(rng.randrange(8192, 24577), n - k)
        small.append((k, size))
        k += size
    large = [(k, min(262144, n - k)) for k in range(0, n, 262144)]
    lib = binding.load()
    scan = getattr(lib, "lda_gzm_scan_bench")
    scan.restype, scan.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t,
                                                 ctypes.c_void_p, ctypes.c_void_p]
    d = api.Decompressor()
    res = {"input_bytes": n, "device": torch.cuda.get_device_name(0), "files": {}}
    t = lambda v: torch.tensor(np.asarray(v).astype(np.int64), device="cuda")  # noqa: E731
    for name, cuts in (("small", small), ("large", large)):
        f, nbytes, offs = build_file(d_in, n, cuts)
        m = len(cuts)
        e = {"file_bytes": nbytes, "members": m}
        out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        r5 = torch.zeros(5, dtype=torch.int64, device="cuda")
        in_off, in_n = t(offs[:-1]), t(np.diff(offs))
        out_off, out_av = t([c[0] for c in cuts]), t([c[1] for c in cuts])
        results = torch.zeros(m, dtype=torch.int32, device="cuda")
        ain = torch.zeros(m, dtype=torch.int64, device="cuda")
        aout = torch.zeros(m, dtype=torch.int64, device="cuda")
        poffs = torch.zeros(m + 1, dtype=torch.int64, device="cuda")

        def keep(key, pair):
            e[key], e[key + "_runs"] = pair

        # (b) the floor: the decode with the members given
        batch = lambda: d.decompress_batch("gzip", f, in_off, in_n, out, out_off, out_av,  # noqa: E731
                                           results, actual_in=ain)
        keep("batch_ms", timed(batch, a.steps, a.warmup))
        assert not results.any().item()
        # (a) the file call
        for mult in (1, 2, 16):
            mm = m * mult
            idx = torch.zeros(2 * (mm + 1), dtype=torch.int64, device="cuda")
            out.zero_()
            keep(f"file_ms_x{mult}",
                 timed(lambda: d.decompress_gzip_members_batch(f, mm, out, r5, index=idx,
                                                               in_nbytes=nbytes, out_avail=n),
                       a.steps, a.warmup))
            assert r5.cpu().tolist() == [0, m, nbytes, n, 0], r5.cpu().tolist()
            got = idx[:2 * (m + 1)].cpu().numpy().reshape(-1, 2)
            assert got[:, 0].tolist() == offs and got[:-1, 1].tolist() == [c[0] for c in cuts]
        assert out[:n].cpu().numpy().tobytes() == data
        idx = torch.zeros(2 * (m + 1), dtype=torch.int64, device="cuda")
        keep("index_ms", timed(lambda: d.index_gzip_members_batch(f, m, r5, index=idx,
                                                                  in_nbytes=nbytes),
                               a.steps, a.warmup))
        assert r5.cpu().tolist() == [0, m, nbytes, n, 0]
        # (c) count + decode without the finder
        out.zero_()
        keep("packed_ms",
             timed(lambda: d.decompress_batch_packed("gzip", f, in_off, in_n, out, poffs, results,
                                                     aout, out_align=1, out_capacity=n),
                   a.steps, a.warmup))
        assert not results.any().item() and poffs[m].item() == n
        assert out[:n].cpu().numpy().tobytes() == data
        keep("batch_ms_2", timed(batch, a.steps, a.warmup))
        # (e) the scan's count pass alone
        counts = torch.zeros((nbytes + 16383) // 16384, dtype=torch.int64, device="cuda")
        keep("scan_ms", timed(lambda: binding.check(scan(f.data_ptr(), nbytes, counts.data_ptr(),
                                                         None), "scan"), a.steps, a.warmup))
        e["candidates"] = int(counts.sum().item())
        e["scan_gb_s"] = round(nbytes / e["scan_ms"] / 1e6, 1)
        e["scan_hbm_share"] = round(e["scan_gb_s"] / (HBM_COPY_TB_S * 1e3), 3)
        floor = min(e["batch_ms"], e["batch_ms_2"])
        e["finder_ms"] = round(e["file_ms_x1"] - e["packed_ms"], 4)
        e["count_ms"] = round(e["packed_ms"] - floor, 4)
        e["gb_s_out"] = round(n / e["file_ms_x1"] / 1e6, 2)
        # (d) the host loop
        fh = f[:nbytes].cpu().numpy().tobytes()
        runs = []
        for _ in range(a.host_runs):
            t0 = time.perf_counter()
            r = d.gzip_decompress_members(fh, n)
            runs.append(round((time.perf_counter() - t0) * 1e3, 2))
            assert r[:4] == (0, nbytes, n, m)
        e["host_ms"], e["host_ms_runs"] = min(runs), runs
        res["files"][name] = e
        del out, f
    s = json.dumps(res)
    print(s)
    if a.out:
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
