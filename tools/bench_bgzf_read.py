"""BGZF files read on the device: what the reader costs on top of the decode
it feeds, the member finder against the serial walk, ranged reads, the host
call.

    python tools/bench_bgzf_read.py [--mib 256] [--steps 5] [--out FILE]

Two files of the same --mib MiB of tests/datagen.py text: `own`, written by
libdeflate_amd_bgzf_compress_batch at level 6 (members of 65 280 bytes), and
`cut`, members of 8 - 24 KiB cut by the caller (the BAM shape) through
libdeflate_amd_compress_batch(BGZF).  Per file, device times by HIP events,
best of --steps after --warmup:
  file_ms      libdeflate_amd_bgzf_decompress_batch, HBM to HBM, with
               max_members = the member count, 2 x and 16 x it
  batch_ms     libdeflate_amd_decompress_batch(GZIP) over descriptors that
               were prepared on the host, exact fill, same output placement:
               what the library could do before once somebody had told it
               where the members are.  Measured twice (batch_ms, batch_ms_2):
               their difference is the spread file_ms - batch_ms is read against
  index_ms     libdeflate_amd_bgzf_index_batch alone - the parallel finder and
               the serial walk (LDA_BGZF_SERIAL), each in a process of its own
  read_ms      1000 random ranges of 1 MiB in one libdeflate_amd_bgzf_read_batch
               (read_gb_s: output bytes per second)
  host_ms      libdeflate_amd_bgzf_decompress beside
               libdeflate_amd_gzip_decompress_members on the same file,
               alternating, wall clock (best, and every run as *_runs)
One JSON object on stdout (and --out).
"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen  # noqa: E402


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    return best


def build_files(mib):
    """-> (plain bytes, {name: file as a uint8 CUDA tensor})"""
    import torch
    n = mib << 20
    seg = b"".join(datagen.text_chunk(65536, 0xB62F + i) for i in range(256))
    data = (seg * (n // len(seg) + 1))[:n]
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    c = api.Compressor(6)
    out = torch.empty(c.bgzf_bound(n), dtype=torch.uint8, device="cuda")
    nb = torch.zeros(1, dtype=torch.int64, device="cuda")
    c.compress_bgzf_batch(d_in, out, nb)
    own = out[:int(nb.item())].clone()
    del out
    # members of 8 - 24 KiB, packed with the compact call, then the EOF member
    rng, cuts, k = random.Random(0xB62F), [], 0
    while k < n:
        size = min(rng.randrange(8192, 24577), n - k)
        cuts.append((k, size))
        k += size
    m = len(cuts)
    t = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    slots = torch.empty(m * 32768, dtype=torch.uint8, device="cuda")
    snb = t([0] * m)
    c.compress_batch("bgzf", d_in, t([a for a, _ in cuts]), t([b for _, b in cuts]), slots,
                     t([i * 32768 for i in range(m)]), t([32768] * m), snb, max_chunk=24576)
    sizes = snb.cpu().tolist()
    assert all(sizes), "a member did not fit its slot"
    import numpy as np
    h = slots.cpu().numpy()
    eof = np.frombuffer(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"),
                        dtype=np.uint8)
    cut = np.concatenate([h[i * 32768:i * 32768 + s] for i, s in enumerate(sizes)] + [eof])
    del slots, h
    c.close()
    pad = lambda x: torch.cat([x, torch.zeros(16, dtype=torch.uint8, device="cuda")])  # noqa: E731
    return data, {"own": (pad(own), own.numel()),
                  "cut": (pad(torch.from_numpy(cut).cuda()), int(cut.size))}


def index_of(d, f, nbytes):
    """(result words, host rows) by the index call with the worst-case bound"""
    import numpy as np
    import torch
    mm = nbytes // 28 + 1
    res = torch.zeros(5, dtype=torch.int64, device="cuda")
    idx = torch.zeros(2 * (mm + 1), dtype=torch.int64, device="cuda")
    d.index_bgzf_batch(f, mm, res, index=idx, in_nbytes=nbytes)
    words = res.cpu().tolist()
    assert words[0] == 0, words
    return words, idx[:2 * (words[1] + 1)].cpu().numpy().astype(np.uint64).reshape(-1, 2)


def child(a):
    """index_ms of both files with the finder this process's environment
    selects; one JSON line"""
    import torch
    _, files = build_files(a.mib)
    d = api.Decompressor()
    out = {"serial": "LDA_BGZF_SERIAL" in os.environ}
    for name, (f, nbytes) in files.items():
        words, _ = index_of(d, f, nbytes)
        m = words[1]
        res = torch.zeros(5, dtype=torch.int64, device="cuda")
        idx = torch.zeros(2 * (m + 1), dtype=torch.int64, device="cuda")
        out[name] = round(timed(lambda: d.index_bgzf_batch(f, m, res, index=idx, in_nbytes=nbytes),
                                a.steps, a.warmup), 4)
        assert res.cpu().tolist()[:2] == [0, m]
    print(json.dumps(out))


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ranges", type=int, default=1000)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a)
    data, files = build_files(a.mib)
    n = len(data)
    d = api.Decompressor()
    res = {"input_bytes": n, "device": torch.cuda.get_device_name(0), "files": {}}
    t = lambda v: torch.tensor(np.asarray(v).astype(np.int64), device="cuda")  # noqa: E731
    for name, (f, nbytes) in files.items():
        words, rows = index_of(d, f, nbytes)
        m = words[1]
        assert words[3] == n
        out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        r5 = torch.zeros(5, dtype=torch.int64, device="cuda")
        e = {"file_bytes": nbytes, "members": m}
        # the yardstick: the batch over descriptors the host prepared
        in_off, in_n = t(rows[:-1, 0]), t(rows[1:, 0] - rows[:-1, 0])
        out_off, out_av = t(rows[:-1, 1]), t(rows[1:, 1] - rows[:-1, 1])
        results = torch.zeros(m, dtype=torch.int32, device="cuda")
        ain = torch.zeros(m, dtype=torch.int64, device="cuda")
        batch = lambda: d.decompress_batch("gzip", f, in_off, in_n, out, out_off, out_av,  # noqa: E731
                                           results, actual_in=ain)
        e["batch_ms"] = round(timed(batch, a.steps, a.warmup), 4)
        assert not results.any().item()
        for mult in (1, 2, 16):
            mm = m * mult
            idx = torch.zeros(2 * (mm + 1), dtype=torch.int64, device="cuda")
            out.zero_()
            ms = timed(lambda: d.decompress_bgzf_batch(f, mm, out, r5, index=idx, in_nbytes=nbytes,
                                                       out_avail=n), a.steps, a.warmup)
            assert r5.cpu().tolist()[:4] == [0, m, nbytes, n]
            e[f"file_ms_x{mult}"] = round(ms, 4)
        assert out[:n].cpu().numpy().tobytes() == data
        e["batch_ms_2"] = round(timed(batch, a.steps, a.warmup), 4)
        e["feature_ms"] = round(e["file_ms_x1"] - min(e["batch_ms"], e["batch_ms_2"]), 4)
        e["gb_s_out"] = round(n / e["file_ms_x1"] / 1e6, 2)
        # ranged reads
        rng = random.Random(0xB62F + 1)
        piece = min(1 << 20, n)
        ranges = np.array([(rng.randrange(0, n - piece + 1), piece) for _ in range(a.ranges)],
                          dtype=np.uint64)
        rout = torch.empty(a.ranges * piece + 64, dtype=torch.uint8, device="cuda")
        rres = torch.zeros(a.ranges, dtype=torch.int32, device="cuda")
        e["read_ms"] = round(timed(lambda: d.read_bgzf_batch(f, rows, ranges, rout, rres,
                                                             in_nbytes=nbytes), a.steps, a.warmup), 4)
        assert not rres.any().item()
        b0 = int(ranges[7][0])
        assert rout[7 * piece:8 * piece].cpu().numpy().tobytes() == data[b0:b0 + piece]
        e["read_gb_s"] = round(a.ranges * piece / e["read_ms"] / 1e6, 2)
        del rout
        # the host calls, alternating
        fh = f[:nbytes].cpu().numpy().tobytes()
        runs = {"host_ms": [], "host_members_ms": []}
        for _ in range(max(3, a.steps // 2)):
            for key, fn in (("host_ms", lambda: d.decompress_bgzf(fh, n)[0]),
                            ("host_members_ms", lambda: d.gzip_decompress_members(fh, n)[0])):
                t0 = time.perf_counter()
                assert fn() == 0
                runs[key].append((time.perf_counter() - t0) * 1e3)
        for key, v in runs.items():     # best, and every run: the spread
            e[key] = round(min(v), 2)
            e[key + "_runs"] = [round(x, 2) for x in v]
        res["files"][name] = e
        del out
    # the finder alone: each variant in a process of its own
    for key, extra in (("index_ms", {}), ("index_serial_ms", {"LDA_BGZF_SERIAL": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "LDA_BGZF_SERIAL"}
        env.update(extra)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--mib",
                            str(a.mib), "--steps", str(a.steps), "--warmup", str(a.warmup)],
                           env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        got = json.loads(p.stdout.strip().splitlines()[-1])
        assert got["serial"] == bool(extra)
        for name in res["files"]:
            res["files"][name][key] = got[name]
    s = json.dumps(res)
    print(s)
    if a.out:
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
