"""The split compress path as a head on the caller's stream and a tail on the
compressor's own (host_compress.hip, compress_plan.h): the bytes are those of
the serial schedule (LDA_COMPRESS_OVERLAP=0, in a fresh process each), every
stream decodes, the rule's boundary cases schedule as the plan's model says,
the call keeps the stream contract with no synchronisation in between, and
the side stream and its events go with the object.

Buffers of 4097 ... 12 288 bytes under max_chunk = 12288 (above the
small-buffer kernel's 4 KiB, so the 64 KiB kernels run), n = 6 x CUs + 5 unless
stated.  The four odd buffers - empty, larger than max_chunk (the fused kernel
behind the split launch), an output slot too small (size 0), incompressible
bytes - sit at 0, head_n - 1, head_n and n - 1, rotated with the case so that
each kind meets each place."""
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
WBITS = {"deflate": -15, "zlib": 15, "gzip": 31}
MAX_CHUNK = 12288
CASES = [(fmt, level) for fmt in ("gzip", "zlib", "deflate") for level in (1, 6, 9)]
KINDS = ("empty", "over_bound", "short_out", "random")
# csrc/compress_plan.h and deflate_kernel.hip (TILE): what the model below restates
TILE, SPLIT_SCRATCH, BLK_WORDS, MIN_PER_CU = 4096, 1280 << 20, 328, 4


def tail_rounds():
    """R: LDA_COMPRESS_TAIL_ROUNDS of the environment, else the header's"""
    e = os.environ.get("LDA_COMPRESS_TAIL_ROUNDS")
    if e and 1 <= int(e) <= 16:
        return int(e)
    hdr = open(os.path.join(ROOT, "libdeflate_amd", "csrc", "compress_plan.h")).read()
    return int(re.search(r"#define LDA_COMPRESS_TAIL_ROUNDS (\d+)", hdr).group(1))


def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def model(n, max_in, cus, R):
    """tools/test_compress_plan.cpp's serial model, levels 0-9 without a
    dictionary or segments -> what compress_last_schedule reports"""
    tok = (max_in + 15) // 16 * 16
    blk = max(1, (tok + TILE - 1) // TILE)
    per_buf = tok * 4 + blk * BLK_WORDS * 4 + 4
    split = max_in > 4096 and n >= MIN_PER_CU * cus and per_buf <= SPLIT_SCRATCH
    per_slice = max(min(n, SPLIT_SCRATCH // per_buf) if split else n, 1)
    heads = tails = 0
    for lo in range(0, n, per_slice):
        nk = min(per_slice, n - lo)
        t = R * cus if split and R and nk >= (MIN_PER_CU + R) * cus else 0
        heads, tails = heads + nk - t, tails + t
    return {"split": int(split), "overlapped": int(tails > 0), "head": heads, "tail": tails,
            "nslices": -(-n // per_slice)}


_POOL = []


def plain_chunks(n, lo=4097, hi=MAX_CHUNK, seed=0x0E111500):
    """n buffers of lo ... hi bytes, cut from 64 generated ones"""
    if not _POOL:
        _POOL.extend(datagen.batch(64, MAX_CHUNK, seed))
    return [_POOL[i % 64][:lo + (i * 2731) % (hi - lo + 1)] for i in range(n)]


def odd_batch(n, head_n, rot):
    """the batch of a case -> (buffers, {index: kind})"""
    chunks = plain_chunks(n)
    places = (0, head_n - 1, head_n, n - 1)
    kinds = {}
    for j, at in enumerate(places):
        kind = KINDS[(j + rot) % 4]
        kinds[at] = kind
        if kind == "empty":
            chunks[at] = b""
        elif kind == "over_bound":
            chunks[at] = (_POOL[at % 64] + _POOL[(at + 1) % 64])[:20000 + at % 97]
        elif kind == "random":
            chunks[at] = np.random.default_rng(at + 1).integers(
                0, 256, MAX_CHUNK - at % 5, dtype=np.uint8).tobytes()
    return chunks, kinds


class Run:
    """one device batch through Compressor.compress_batch: made (uploads, waited
    for), then queued by launch(), which waits for nothing"""

    def __init__(self, c, fmt, chunks, kinds=None, max_chunk=MAX_CHUNK, stream=None,
                 launch=True):
        import torch
        n = len(chunks)
        sizes = np.array([len(x) for x in chunks], dtype=np.int64)
        in_off = np.concatenate(([0], np.cumsum((sizes + 15) // 16 * 16)))
        blob = np.zeros(int(in_off[-1]) + 16, dtype=np.uint8)
        for i, x in enumerate(chunks):
            blob[in_off[i]:in_off[i] + len(x)] = np.frombuffer(x, dtype=np.uint8)
        slots = np.array([(c.bound(fmt, len(x)) + 15) // 16 * 16 for x in chunks], dtype=np.int64)
        avail = slots.copy()
        for at, kind in (kinds or {}).items():
            if kind == "short_out":
                avail[at] = 24
        out_off = np.concatenate(([0], np.cumsum(slots)))
        self.n, self.out_off = n, out_off
        dev = "cuda"
        self.data = torch.from_numpy(blob).to(dev)
        self.in_off = torch.from_numpy(in_off[:-1].copy()).to(dev)
        self.in_n = torch.from_numpy(sizes).to(dev)
        self.c_off = torch.from_numpy(out_off[:-1].copy()).to(dev)
        self.c_av = torch.from_numpy(avail).to(dev)
        self.comp = torch.zeros(int(out_off[-1]) + 16, dtype=torch.uint8, device=dev)
        self.c_n = torch.full((n,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()    # (all of that ran on the default stream)
        self.args = (c, fmt, max_chunk, stream)
        if launch:
            self.launch()

    def launch(self):
        c, fmt, max_chunk, stream = self.args
        c.compress_batch(fmt, self.data, self.in_off, self.in_n, self.comp, self.c_off, self.c_av,
                         self.c_n, stream=stream, max_chunk=max_chunk)
        self.schedule = c.last_schedule()

    def streams(self, comp=None, c_n=None):
        """after a synchronise: the sizes and the streams' bytes"""
        sizes = (self.c_n if c_n is None else c_n).cpu().numpy()
        cb = (self.comp if comp is None else comp).cpu().numpy()
        return sizes, [cb[self.out_off[i]:self.out_off[i] + sizes[i]].tobytes()
                       for i in range(self.n)]


def check_decodes(fmt, chunks, sizes, zs, kinds=None, ref=None, tag=""):
    kinds = kinds or {}
    for i, (x, z) in enumerate(zip(chunks, zs)):
        if kinds.get(i) == "short_out":
            assert sizes[i] == 0, (tag, i, "a slot of 24 bytes held", sizes[i])
            continue
        assert sizes[i] > 0, (tag, i, kinds.get(i))
        assert zlib.decompress(z, WBITS[fmt]) == x, (tag, i, kinds.get(i))
        if ref is not None and i in kinds:
            r, ain, aout, out = ref.decompress_ex(fmt, z, len(x))
            assert (r, ain, out) == (0, len(z), x), (tag, i, kinds[i], "reference")


def digest_cases():
    """every case's batch compressed in this process -> lines of
    `fmt level sha256 split overlapped head tail`"""
    import torch
    from libdeflate_amd import api
    cus, R = num_cus(), tail_rounds()
    n = 6 * cus + 5
    head_n = model(n, MAX_CHUNK, cus, R)["head"]
    lines = []
    for rot, (fmt, level) in enumerate(CASES):
        chunks, kinds = odd_batch(n, head_n, rot)
        c = api.Compressor(level)
        run = Run(c, fmt, chunks, kinds)
        torch.cuda.synchronize()
        sizes, zs = run.streams()
        h = hashlib.sha256(sizes.tobytes())
        for z in zs:
            h.update(z)
        s = run.schedule
        lines.append(f"{fmt} {level} {h.hexdigest()} {s['split']} {s['overlapped']} "
                     f"{s['head']} {s['tail']}")
        c.close()
    return lines


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests import test_compress_overlap_gpu as T
for line in T.digest_cases():
    print("case", line)
"""


def _child(overlap):
    env = dict(os.environ)
    env.pop("LDA_COMPRESS_OVERLAP", None)
    if not overlap:
        env["LDA_COMPRESS_OVERLAP"] = "0"
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    rows = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("case ")]
    assert len(rows) == len(CASES)
    return rows


def test_same_bytes_as_the_serial_schedule():
    """gzip, zlib and raw DEFLATE at levels 1, 6 and 9, each batch with the four
    odd buffers: SHA-256 over every size and every stream's bytes, in two fresh
    processes one after the other"""
    cus, R = num_cus(), tail_rounds()
    n = 6 * cus + 5
    want = model(n, MAX_CHUNK, cus, R)
    assert want["overlapped"] == 1 and want["tail"] == R * cus
    serial, over = _child(False), _child(True)
    for (fmt, level), a, b in zip(CASES, serial, over):
        print(fmt, level, a[2][:16], b[2][:16], a[3:], b[3:])
        assert a[:2] == b[:2] == [fmt, str(level)]
        assert [int(v) for v in a[3:]] == [1, 0, n, 0], (fmt, level, "serial run", a)
        assert [int(v) for v in b[3:]] == [1, 1, want["head"], want["tail"]], (fmt, level, b)
        assert a[2] == b[2], (fmt, level, "the schedules' bytes differ")


def test_every_stream_decodes():
    """the default schedule: every stream of every case's batch back to its
    input through zlib, the odd buffers through the reference as well (where
    it is built)"""
    import torch
    from libdeflate_amd import api
    from tests import oracle_util
    ref = oracle_util.load_ref()
    cus, R = num_cus(), tail_rounds()
    n = 6 * cus + 5
    want = model(n, MAX_CHUNK, cus, R)
    for rot, (fmt, level) in enumerate(CASES):
        chunks, kinds = odd_batch(n, want["head"], rot)
        c = api.Compressor(level)
        run = Run(c, fmt, chunks, kinds)
        torch.cuda.synchronize()
        assert run.schedule == {k: want[k] for k in run.schedule}, (fmt, level)
        sizes, zs = run.streams()
        assert all(len(z) <= c.bound(fmt, len(x)) for x, z in zip(chunks, zs))
        check_decodes(fmt, chunks, sizes, zs, kinds, ref, (fmt, level))
        c.close()


def test_boundary_cases_of_the_rule():
    """4 x CUs (split, too few for a tail), one buffer short of a tail, the first
    batch with one; then two batches of several scratch slices: a bound of 1 MiB
    at the first n that needs more than one (its slices are too short for a
    tail on a device whose slice holds fewer than (4 + R) buffers per CU), and a
    bound of 200 000 bytes, whose two slices both have one.  Each decodes, and
    compress_last_schedule says what the plan test's model says."""
    import torch
    from libdeflate_amd import api
    cus, R = num_cus(), tail_rounds()
    cases = [(4 * cus, MAX_CHUNK), ((4 + R) * cus - 1, MAX_CHUNK), ((4 + R) * cus, MAX_CHUNK)]
    big, mid = 1 << 20, 200000

    def first_of_two(bound):
        return next(n for n in range(1, 1 << 16) if model(n, bound, cus, R)["nslices"] >= 2)
    cases.append((first_of_two(big), big))
    # a whole slice and a second one of (4 + R) x CUs
    cases.append((first_of_two(mid) - 1 + (4 + R) * cus, mid))
    if cus <= 256 and R <= 1:
        assert model(cases[-1][0], mid, cus, R)["tail"] == 2 * R * cus
    assert model((4 + R) * cus, MAX_CHUNK, cus, R)["tail"] == R * cus
    assert model((4 + R) * cus - 1, MAX_CHUNK, cus, R)["overlapped"] == 0
    c = api.Compressor(6)
    for n, bound in cases:
        want = model(n, bound, cus, R)
        chunks = plain_chunks(n, 4097, 6144)
        run = Run(c, "gzip", chunks, max_chunk=bound)
        torch.cuda.synchronize()
        print(n, bound, want, run.schedule)
        assert run.schedule == {k: want[k] for k in run.schedule}, (n, bound)
        sizes, zs = run.streams()
        check_decodes("gzip", chunks, sizes, zs, tag=(n, bound))
    c.close()


def _contract_make(c, stream, seed):
    n = 6 * num_cus() + 5
    a_chunks = plain_chunks(n)
    b_chunks = plain_chunks(n, 4200 + seed, 9000)[::-1]
    return (Run(c, "gzip", a_chunks, stream=stream, launch=False), a_chunks,
            Run(c, "zlib", b_chunks, stream=stream, launch=False), b_chunks)


def _contract(made, stream):
    """compress A; zero A's input; copy A's sizes and output away; compress B
    with the same object into other buffers - all on `stream`, nothing waited for"""
    import torch
    a, a_chunks, b, b_chunks = made
    a.launch()
    assert a.schedule["overlapped"] == 1
    with torch.cuda.stream(stream):
        a.data.zero_()
        a_n, a_comp = a.c_n.clone(), a.comp.clone()
        a.comp.zero_()
    b.launch()
    assert b.schedule["overlapped"] == 1
    return (a, a_chunks, a_comp, a_n), (b, b_chunks)


def _contract_check(held, tag):
    (a, a_chunks, a_comp, a_n), (b, b_chunks) = held
    sizes, zs = a.streams(a_comp, a_n)
    check_decodes("gzip", a_chunks, sizes, zs, tag=(tag, "A"))
    sizes, zs = b.streams()
    check_decodes("zlib", b_chunks, sizes, zs, tag=(tag, "B"))


def test_stream_contract_without_synchronisation():
    """on a stream that is not the default one, then two objects on two streams
    at once: one synchronise at the end, A read from its copy"""
    import torch
    from libdeflate_amd import api
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c1, c2 = api.Compressor(6), api.Compressor(6)
    held = _contract(_contract_make(c1, s1, 0), s1)
    torch.cuda.synchronize()
    _contract_check(held, "one stream")
    made1, made2 = _contract_make(c1, s1, 1), _contract_make(c2, s2, 2)
    held1 = _contract(made1, s1)
    held2 = _contract(made2, s2)
    torch.cuda.synchronize()
    _contract_check(held1, "two streams, first")
    _contract_check(held2, "two streams, second")
    c1.close()
    c2.close()


def test_object_lifetime():
    """32 compressors in a row, each with one overlapped call: a stream or an
    event that stayed behind would add up; every call succeeds and the last
    object's streams decode"""
    import torch
    from libdeflate_amd import api
    cus, R = num_cus(), tail_rounds()
    n = (4 + R) * cus
    chunks = plain_chunks(n, 4097, 4608)
    for k in range(32):
        c = api.Compressor(1)
        run = Run(c, "deflate", chunks, max_chunk=4608)
        assert run.schedule["overlapped"] == 1 and run.schedule["tail"] == R * cus, k
        torch.cuda.synchronize()
        if k == 31:
            sizes, zs = run.streams()
            check_decodes("deflate", chunks, sizes, zs, tag="last object")
        c.close()
