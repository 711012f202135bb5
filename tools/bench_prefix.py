"""The prefix decompress against the full decode of the same streams.

    python tools/bench_prefix.py [--parent LIB] [--rounds 3] [--steps 7]
                                 [--out profiles/prefix_bench.json]

The bench batch: 4096 gzip streams of 64 KiB of the benchmark mix, level 6,
device to device, HIP events around the enqueued work.  Per round every
configuration is timed once after the other (best of --steps after --warmup,
every run kept), so that a drift of the machine lands on all of them alike:
  decode_ms        libdeflate_amd_decompress_batch into slots of the known size
  prefix256_ms     libdeflate_amd_decompress_prefix_batch, every limit 256
  prefix4096_ms    ... 4096
  prefix65536_ms   ... 65 536: nothing is cut, the same work as decode_ms
--parent LIB: libdeflate_amd_decompress_batch through another build of the
library (the parent commit's, built side by side) - a process per measurement,
this build's and the parent's alternating, --rounds times each.
The figures to read (best of all rounds each):
  prefix256_over_decode     the 256-byte prefix as a share of the full decode
  prefix65536_over_decode   the uncut prefix against the decode
  decode_over_parent        this build's decode against the parent's
  decode_spread             (max - min) / min of this build's decode over the
                            rounds: what a ratio is read against
One JSON object on stdout (and --out).
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from libdeflate_amd import api, binding  # noqa: E402
from tools.bench_sizes import build, timed  # noqa: E402

N, SIZE, FMT, LEVEL = 4096, 65536, "gzip", 6
LIMITS = (256, 4096, 65536)


def measure(a, what):
    """what: "all" or "decode" -> {config: [best per round]}, all runs"""
    import torch
    d = api.Decompressor()
    data, in_off, in_n, cbytes = build(N, SIZE, FMT, LEVEL, -1)
    slot = SIZE
    dst = torch.empty(N * slot + 64, dtype=torch.uint8, device="cuda")
    out_off = torch.arange(N, dtype=torch.int64, device="cuda") * slot
    out_av = torch.full((N,), SIZE, dtype=torch.int64, device="cuda")
    res = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    ain = torch.zeros(N, dtype=torch.int64, device="cuda")
    aout = torch.zeros(N, dtype=torch.int64, device="cuda")
    cfg = {"decode": (lambda: d.decompress_batch(FMT, data, in_off, in_n, dst, out_off, out_av,
                                                 res, ain, aout), 0, SIZE)}
    if what == "all":
        for lim in LIMITS:
            lims = torch.full((N,), lim, dtype=torch.int64, device="cuda")
            cfg[f"prefix{lim}"] = (
                lambda lims=lims: d.decompress_prefix_batch(FMT, data, in_off, in_n, dst, out_off,
                                                            lims, res, aout, actual_in=ain),
                binding.PREFIX if lim < SIZE else 0, lim)
    best = {k: [] for k in cfg}
    runs = {k: [] for k in cfg}
    for _ in range(a.rounds if what == "all" else 1):
        for k, (fn, want, nout) in cfg.items():
            b, r = timed(fn, a.steps, a.warmup)
            assert bool((res == want).all().item()) and bool((aout == nout).all().item()), k
            best[k].append(b)
            runs[k].append(r)
    d.close()
    return {"in_bytes": cbytes, "best": best, "runs": runs}


def child(a, lib):
    env = dict(os.environ, LIBDEFLATE_AMD_LIB=os.path.abspath(lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps),
           "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", help="the parent commit's build of the library")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a, "decode")))
        return
    m = measure(a, "all")
    res = {"device": torch.cuda.get_device_name(0), "lib": binding.LIB_PATH, "streams": N,
           "size": SIZE, "fmt": FMT, "level": LEVEL, "in_bytes": m["in_bytes"]}
    for k in m["best"]:
        res[f"{k}_ms"] = min(m["best"][k])
        res[f"{k}_ms_rounds"] = m["best"][k]
        res[f"{k}_ms_runs"] = m["runs"][k]
    dec = m["best"]["decode"]
    res["decode_spread"] = round((max(dec) - min(dec)) / min(dec), 4)
    for lim in LIMITS:
        res[f"prefix{lim}_over_decode"] = round(res[f"prefix{lim}_ms"] / res["decode_ms"], 4)
    if a.parent:
        this, parent = [], []
        for _ in range(a.rounds):      # alternating, a fresh process each
            this.append(child(a, binding.LIB_PATH)["best"]["decode"][0])
            parent.append(child(a, a.parent)["best"]["decode"][0])
        res["ab_decode_ms_rounds"], res["ab_parent_decode_ms_rounds"] = this, parent
        res["parent_decode_ms"] = min(parent)
        res["decode_over_parent"] = round(min(this) / min(parent), 4)
    s = json.dumps(res)
    print(s)
    if a.out:
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
