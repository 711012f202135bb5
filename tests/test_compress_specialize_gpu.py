"""The LZ77 stage of the split compress path built once per level
(lda_deflate_batch_kernel_l1 ... _l9: deflate_kernel.hip, policy_level;
host_compress.hip, lz77_kernel_of()) writes the bytes of the kernel that serves
every level (LDA_COMPRESS_SPECIALIZE=0): every level 1-9 as raw DEFLATE, zlib
and gzip, one BGZF batch and one batch with a preset dictionary, each batch
compressed in two fresh processes, with and without the switch; every stream
goes back to its input through zlib in both; and the call says which kernel ran.

The batches have LDA_SPLIT_MIN_PER_CU x CUs + 5 buffers under a bound of 64 KiB,
so they take the split path (no tail: the kernel is the same on both streams,
tests/test_compress_overlap_gpu.py has the schedules).  Buffer i is the first
SIZES[i mod 15] bytes of chunk i mod 64 of tests/datagen.py's 64 KiB mix, so
every size meets every kind of bytes (15 and 8 have no common factor): text,
counters, the 16-symbol text, random bytes (stored blocks).  The sizes: 0, 1,
both sides of the stored-only rule (n <= 55 - 4 x level: 53 ... 56 - 4 x level),
the tile (4095, 4096, 4097), the split statistics' threshold (4999, 5000), two
tiles and a byte, and the bound itself.

The preset dictionary's batch does not take the split path (compress_plan.h:
a dictionary keeps the fused kernel, which has no instances), so what that
case can assert is that the switch changes neither the kernel nor the bytes."""
import hashlib
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WBITS = {"deflate": -15, "zlib": 15, "gzip": 31, "bgzf": 31}
BOUND = 65536
BGZF_BLOCK = 65280
LEVELS = tuple(range(1, 10))
FORMATS = ("deflate", "zlib", "gzip")
# (format, level, with the dictionary)
CASES = [(fmt, level, False) for level in LEVELS for fmt in FORMATS] + \
        [("bgzf", 6, False), ("zlib", 6, True)]
GENERIC = "lda_deflate_batch_kernel"
# the levels whose instance the split path uses (host_compress.hip, k_lz77_level)
INSTANCES = set(LEVELS)


def min_per_cu():
    hdr = open(os.path.join(ROOT, "libdeflate_amd", "csrc", "compress_plan.h")).read()
    return int(re.search(r"#define LDA_SPLIT_MIN_PER_CU (\d+)", hdr).group(1))


def sizes_of(level, top):
    edge = 54 - 4 * level
    return (0, 1, edge - 1, edge, edge + 1, edge + 2, 4095, 4096, 4097, 4999, 5000, 8193, top,
            2 * 4096, 33)


_POOL = []


def batch_of(n, level, top=BOUND):
    if not _POOL:
        _POOL.extend(datagen.batch(64, BOUND, 0x5EC1A115))
    sizes = sizes_of(level, top)
    assert len(sizes) == 15 and min(sizes) >= 0
    return [_POOL[i % 64][:sizes[i % 15]] for i in range(n)]


def want_kernel(level, dictionary, specialize):
    if dictionary:
        return "lda_deflate_fused_kernel"
    return f"{GENERIC}_l{level}" if specialize and level in INSTANCES else GENERIC


def run_cases():
    """every case's batch compressed and decoded in this process -> lines of
    `fmt level dict sha256 kernel split`"""
    import torch
    from libdeflate_amd import api
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = min_per_cu() * cus + 5
    zdict = datagen.text_chunk(20000, 0x5EC1D1C7)
    lines = []
    for fmt, level, with_dict in CASES:
        chunks = batch_of(n, level, BGZF_BLOCK if fmt == "bgzf" else BOUND)
        c = api.Compressor(level)
        sizes = np.array([len(x) for x in chunks], dtype=np.int64)
        in_off = np.concatenate(([0], np.cumsum((sizes + 15) // 16 * 16)))
        blob = np.zeros(int(in_off[-1]) + 16, dtype=np.uint8)
        for i, x in enumerate(chunks):
            blob[in_off[i]:in_off[i] + len(x)] = np.frombuffer(x, dtype=np.uint8)
        slots = np.array([(c.bound(fmt, len(x)) + 4 + 15) // 16 * 16 for x in chunks],
                         dtype=np.int64)
        out_off = np.concatenate(([0], np.cumsum(slots)))
        dev = "cuda"
        data = torch.from_numpy(blob).to(dev)
        d_in_off = torch.from_numpy(in_off[:-1].copy()).to(dev)
        d_in_n = torch.from_numpy(sizes).to(dev)
        d_out_off = torch.from_numpy(out_off[:-1].copy()).to(dev)
        d_avail = torch.from_numpy(slots).to(dev)
        comp = torch.zeros(int(out_off[-1]) + 16, dtype=torch.uint8, device=dev)
        d_n = torch.full((n,), -1, dtype=torch.int64, device=dev)
        if with_dict:
            c.compress_batch_dict(fmt, torch.from_numpy(np.frombuffer(zdict, dtype=np.uint8).copy())
                                  .to(dev), data, d_in_off, d_in_n, comp, d_out_off, d_avail, d_n)
        else:
            c.compress_batch(fmt, data, d_in_off, d_in_n, comp, d_out_off, d_avail, d_n,
                             max_chunk=BOUND)
        kernel, split = c.last_kernel(), c.last_schedule()["split"]
        torch.cuda.synchronize()
        got = d_n.cpu().numpy()
        cb = comp.cpu().numpy()
        h = hashlib.sha256(got.tobytes())
        for i, x in enumerate(chunks):
            assert got[i] > 0, (fmt, level, i, len(x), got[i])
            z = cb[out_off[i]:out_off[i] + got[i]].tobytes()
            h.update(z)
            d = zlib.decompressobj(WBITS[fmt], zdict=zdict) if with_dict else \
                zlib.decompressobj(WBITS[fmt])
            assert d.decompress(z) + d.flush() == x and d.eof and not d.unused_data, \
                (fmt, level, i, len(x))
        lines.append(f"{fmt} {level} {int(with_dict)} {h.hexdigest()} {kernel} {split}")
        c.close()
    return lines


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests import test_compress_specialize_gpu as T
for line in T.run_cases():
    print("case", line)
"""


def _child(specialize):
    env = dict(os.environ)
    env.pop("LDA_COMPRESS_SPECIALIZE", None)
    if not specialize:
        env["LDA_COMPRESS_SPECIALIZE"] = "0"
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    rows = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("case ")]
    assert len(rows) == len(CASES)
    return {(row[0], int(row[1]), bool(int(row[2]))): row[3:] for row in rows}


@pytest.fixture(scope="module")
def runs():
    """the two processes, once for all cases: (generic, specialised); a child
    has already decoded every stream of every case when it returns"""
    return _child(False), _child(True)


@pytest.mark.parametrize("fmt,level,with_dict", CASES,
                         ids=[f"{f}-l{l}" + ("-dict" if d else "") for f, l, d in CASES])
def test_same_bytes_as_the_generic_kernel(runs, fmt, level, with_dict):
    generic, special = runs
    g, s = generic[fmt, level, with_dict], special[fmt, level, with_dict]
    print(fmt, level, with_dict, g, s)
    assert g[1] == want_kernel(level, with_dict, False), g
    assert s[1] == want_kernel(level, with_dict, True), s
    assert g[2] == s[2] == ("0" if with_dict else "1"), (g, s)     # the split path
    assert g[0] == s[0], (fmt, level, "the kernels' bytes differ")
