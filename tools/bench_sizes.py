"""The size query against the decode a caller without it has to run to learn
the sizes, and what the packed decompress costs on top of its parts.

    python tools/bench_sizes.py [--parent LIB] [--variant NAME=LIB ...]
                                [--steps 7] [--quick] [--out FILE]

Workloads (device to device, HIP events around the enqueued work, best of
--steps after --warmup, every run kept as *_runs):
  bench       4096 x 64 KiB of the benchmark mix, gzip, level 6
  bench65536  65 536 such streams
  zlib4k      262 144 x 4 KiB, zlib, level 9
  kind0..7    4096 streams of one chunk kind of the mix each
              (tools/microbench.py inflate --kind K)
Per workload:
  decode_ms   libdeflate_amd_decompress_batch into slots of the known size -
              measured twice (decode_ms, decode_ms_2): their difference is the
              run-to-run noise the other figures are read against
  sizes_ms    libdeflate_amd_decompress_sizes_batch, NULL limits
  packed_ms   libdeflate_amd_decompress_batch_packed (out_align 16)
  parts_ms    the size query, then the decode with descriptors made on the
              host, queued back to back: packed_ms - parts_ms is the scan, the
              descriptor kernels and the result merge
--parent LIB: the same decode through another build of the library (the parent
commit's, built side by side as tools/ab.sh does) in a process of its own:
parent_decode_ms, the yardstick - ratio = sizes_ms / parent_decode_ms.
--variant NAME=LIB[:ENV=VALUE]: the size query of another build / setting (the
kernel built for more waves per SIMD, LDA_SIZES_WAVES_PER_CU=...), the same way.
One JSON object on stdout (and --out).
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tests import datagen, oracle_util, streams  # noqa: E402

DISTINCT = 64


def timed(fn, steps, warmup):
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


def workloads(quick):
    w = [("bench", 4096, 65536, "gzip", 6, -1), ("bench65536", 65536, 65536, "gzip", 6, -1),
         ("zlib4k", 262144, 4096, "zlib", 9, -1)]
    w += [(f"kind{k}", 4096, 65536, "gzip", 6, k) for k in range(8)]
    return [x for x in w if not quick or x[1] <= 4096][:3 if quick else None]


def build(n, size, fmt, level, kind):
    """-> (data tensor, in_off, in_n, total compressed bytes): DISTINCT
    different streams, repeated; every stream has its own bytes in the blob"""
    import torch
    ref = oracle_util.load_ref()
    mix = datagen.MIX4K if size <= 4096 else datagen.MIX64K
    if kind >= 0:
        chunks = [datagen.chunk(kind + 8 * (i % 8), size, 0x0E110004) for i in range(DISTINCT)]
    else:
        chunks = [datagen.chunk(i, size, 0x0E110004, mix) for i in range(DISTINCT)]
    comp = [ref.compress(fmt, level, c) if ref else streams._zcompress(fmt, min(level, 9), c)
            for c in chunks]
    offs, tile = [], bytearray()
    for c in comp:
        offs.append(len(tile))
        tile += c
        tile += bytes(-len(tile) % 16)
    reps = (n + DISTINCT - 1) // DISTINCT
    t = torch.frombuffer(tile, dtype=torch.uint8).cuda()
    data = torch.cat([t.repeat(reps), torch.zeros(64, dtype=torch.uint8, device="cuda")])
    base = torch.arange(reps, dtype=torch.int64, device="cuda").repeat_interleave(DISTINCT) * len(tile)
    in_off = (base + torch.tensor(offs, dtype=torch.int64, device="cuda").repeat(reps))[:n]
    in_n = torch.tensor([len(c) for c in comp], dtype=torch.int64, device="cuda").repeat(reps)[:n]
    return data, in_off.contiguous(), in_n.contiguous(), int(in_n.sum().item())


def measure(a, what):
    """what: subset of {"decode", "sizes", "packed"} -> {workload: figures}"""
    import torch
    d = api.Decompressor()
    out = {}
    for name, n, size, fmt, level, kind in workloads(a.quick):
        data, in_off, in_n, cbytes = build(n, size, fmt, level, kind)
        e = {"streams": n, "size": size, "fmt": fmt, "level": level, "in_bytes": cbytes}
        slot = (size + 15) // 16 * 16
        dst = torch.empty(n * slot + 64, dtype=torch.uint8, device="cuda")
        out_off = torch.arange(n, dtype=torch.int64, device="cuda") * slot
        out_av = torch.full((n,), size, dtype=torch.int64, device="cuda")
        res = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ain = torch.zeros(n, dtype=torch.int64, device="cuda")
        aout = torch.zeros(n, dtype=torch.int64, device="cuda")
        nbytes = torch.zeros(n, dtype=torch.int64, device="cuda")
        poff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        decode = lambda: d.decompress_batch(fmt, data, in_off, in_n, dst, out_off, out_av,  # noqa: E731
                                            res, ain, aout)
        sizes = lambda: d.decompress_sizes_batch(fmt, data, in_off, in_n, res, nbytes,  # noqa: E731
                                                 actual_in=ain)
        packed = lambda: d.decompress_batch_packed(fmt, data, in_off, in_n, dst, poff, res,  # noqa: E731
                                                   aout, actual_in=ain, out_align=16)

        def parts():
            sizes()
            decode()
        if "decode" in what:
            e["decode_ms"], e["decode_ms_runs"] = timed(decode, a.steps, a.warmup)
            assert not res.any().item() and bool((aout == size).all().item())
        if "sizes" in what:
            e["sizes_ms"], e["sizes_ms_runs"] = timed(sizes, a.steps, a.warmup)
            assert not res.any().item() and bool((nbytes == size).all().item())
        if "packed" in what:
            e["packed_ms"], e["packed_ms_runs"] = timed(packed, a.steps, a.warmup)
            assert not res.any().item() and int(poff[n].item()) == n * slot
            e["parts_ms"], e["parts_ms_runs"] = timed(parts, a.steps, a.warmup)
            e["packed_over_parts_ms"] = round(e["packed_ms"] - e["parts_ms"], 4)
        if "decode" in what and "sizes" in what:
            e["decode_ms_2"], e["decode_ms_2_runs"] = timed(decode, a.steps, a.warmup)
        out[name] = e
        del data, dst
        torch.cuda.empty_cache()
    d.close()
    return out


def child(a, lib, what, env_extra=None):
    env = dict(os.environ)
    env["LIBDEFLATE_AMD_LIB"] = os.path.abspath(lib)
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--steps", str(a.steps),
           "--warmup", str(a.warmup)] + (["--quick"] if a.quick else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="the 4096-stream workloads only")
    ap.add_argument("--parent", help="the parent commit's build of the library")
    ap.add_argument("--variant", action="append", default=[], help="NAME=LIB[:ENV=VALUE]")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a, set(a.child.split(",")))))
        return
    res = {"device": torch.cuda.get_device_name(0), "lib": binding.LIB_PATH,
           "workloads": measure(a, {"decode", "sizes", "packed"})}
    if a.parent:
        got = child(a, a.parent, "decode")
        for name, e in res["workloads"].items():
            e["parent_decode_ms"] = got[name]["decode_ms"]
            e["parent_decode_ms_runs"] = got[name]["decode_ms_runs"]
            e["sizes_over_parent_decode"] = round(e["sizes_ms"] / e["parent_decode_ms"], 4)
            e["decode_over_parent_decode"] = round(e["decode_ms"] / e["parent_decode_ms"], 4)
    for spec in a.variant:
        name, rest = spec.split("=", 1)
        lib, _, env = rest.partition(":")
        got = child(a, lib, "sizes", dict([env.split("=", 1)]) if env else None)
        for w, e in res["workloads"].items():
            e[f"sizes_ms[{name}]"] = got[w]["sizes_ms"]
            e[f"sizes_ms_runs[{name}]"] = got[w]["sizes_ms_runs"]
    s = json.dumps(res)
    print(s)
    if a.out:
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
