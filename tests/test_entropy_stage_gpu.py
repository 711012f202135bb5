"""The split compress path: the LZ77 stage (lda_deflate_batch_kernel) leaves
tokens and block descriptors, lda_deflate_entropy_kernel writes the streams.
It is taken by calls with a size bound (compress_batch_bounded, the host
batch, the segmented single-buffer path) and at least four buffers per CU;
unbounded device batches keep the fused kernel, and both must write the same
bytes.  The inputs are repeated up to that count; every distinct stream is
decoded by the reference library (the oracle where it is not built) and by
zlib, and every copy of an input must come out the same.  The segmented path
has at most 512 segments per launch at its own segment sizes, fewer than
four per CU on a full MI355X: it is driven onto the split path here with
LDA_SEG_BYTES in a child process."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from libdeflate_amd import api
from tests import datagen, oracle_util

pytestmark = pytest.mark.gpu

WB = {"deflate": -15, "zlib": 15, "gzip": 31}


def _decoder():
    return oracle_util.load_ref() or oracle_util.load_oracle()


def _fill(chunks):
    """the chunks repeated to four buffers per CU (what takes the split path)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    k = -(-4 * cus // len(chunks))
    return chunks * k


def _inputs():
    """buffers that span several blocks, and the shortest ones"""
    rng = np.random.default_rng(0x5E1175)
    text = datagen.text_chunk(1 << 18, 31)
    rnd = rng.integers(0, 256, 300000, dtype=np.uint8).tobytes()
    return [
        text[:40000] + rnd[:40000] + text[40000:80000],   # content switches: retro splits
        text[:200000],                                     # MAX_BLOCK_LEN ends
        # literals only: stored blocks, MAX_BLOCK_LEN ends (the token cap never
        # ends a block first: a block has no more tokens than bytes)
        rnd[:150000],
        bytes(70000) + text[:30000],                       # long matches, then text
        datagen.binary_chunk(65536, 5),
        b"", b"a", b"ab", b"abc",
        text[:4097], text[:65535], text[:65537],
    ]


def _run(fmt, level, chunks, bound, avail=None):
    """one device batch; bound None = the unbounded (fused) call"""
    c = api.Compressor(level)
    n = len(chunks)
    offs, pos = [], 0
    for x in chunks:
        offs.append(pos)
        pos += (len(x) + 15) // 16 * 16
    blob = bytearray(pos + 64)
    for o, x in zip(offs, chunks):
        blob[o:o + len(x)] = x
    data = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    in_off = torch.tensor(offs, dtype=torch.int64).cuda()
    in_n = torch.tensor([len(x) for x in chunks], dtype=torch.int64).cuda()
    av = [c.bound(fmt, len(x)) if avail is None else avail(x) for x in chunks]
    slot = [(a + 15) // 16 * 16 + 16 for a in av]
    out_off = torch.tensor(np.cumsum([0] + slot[:-1]), dtype=torch.int64).cuda()
    out = torch.zeros(sum(slot) + 64, dtype=torch.uint8, device="cuda")
    out_av = torch.tensor(av, dtype=torch.int64).cuda()
    out_n = torch.zeros(n, dtype=torch.int64, device="cuda")
    c.compress_batch(fmt, data, in_off, in_n, out, out_off, out_av, out_n, max_chunk=bound)
    torch.cuda.synchronize()
    host, sizes, offv = out.cpu().numpy(), out_n.cpu().tolist(), out_off.cpu().tolist()
    c.close()
    return [bytes(host[o:o + s]) if s else None for o, s in zip(offv, sizes)]


def _check(fmt, chunks, comps):
    ref = _decoder()
    first = {}
    for x, z in zip(chunks, comps):
        assert first.setdefault(bytes(x), z) == z
    for x, z in first.items():
        assert z is not None, len(x)
        assert zlib.decompress(z, WB[fmt]) == x
        r, ain, _, got = ref.decompress_ex(fmt, z, len(x))
        assert (r, ain, got) == (0, len(z), x)


@pytest.mark.parametrize("level", [0, 1, 6, 9])
@pytest.mark.parametrize("fmt", ["deflate", "zlib", "gzip"])
def test_split_path_decodes_and_matches_fused(fmt, level):
    chunks = _fill(_inputs())
    bound = max(len(x) for x in chunks)
    split = _run(fmt, level, chunks, bound)
    _check(fmt, chunks, split)
    # the unbounded call runs the fused kernel: the same decisions, the same bytes
    assert split == _run(fmt, level, chunks, None)


@pytest.mark.parametrize("fmt", ["deflate", "gzip"])
def test_split_path_out_avail(fmt):
    chunks = _fill(_inputs()[:5] + [b"abc"])
    bound = max(len(x) for x in chunks)
    exact = _run(fmt, 6, chunks, bound)
    _check(fmt, chunks, exact)
    sizes = {bytes(x): len(z) for x, z in zip(chunks, exact)}
    assert _run(fmt, 6, chunks, bound, avail=lambda x: sizes[bytes(x)]) == exact
    short = _run(fmt, 6, chunks, bound, avail=lambda x: sizes[bytes(x)] - 1)
    assert short == [None] * len(chunks)


def test_split_path_in_slices():
    """a bound large enough that the token lists of a few buffers fill the
    scratch of one launch: the batch runs as several slices"""
    rng = np.random.default_rng(7)
    chunks = _fill([datagen.chunk(i, int(rng.integers(1000, 70000)), 0x5E11) for i in range(13)])
    bound = 64 << 20
    comps = _run("gzip", 6, chunks, bound)
    _check("gzip", chunks, comps)
    assert comps == _run("gzip", 6, chunks, None)


def test_bounded_equals_unbounded_on_the_digest_inputs():
    """tools/digest_deflate.py's mixed set, levels 1-9: the split path makes
    the fused kernel's decisions"""
    from tests.test_deflate_gpu import _weird_chunk
    rng = np.random.default_rng(0x0D16E57)
    edges = [0, 1, 3, 52, 53, 4095, 4096, 4097, 8190, 8194, 12288, 20480, 24576,
             65534, 65536, 65538, 69632, 131072, 131073, 200000]
    chunks = [_weird_chunk(rng, n) for n in edges]
    chunks += datagen.batch(16, 65536, 0x0E110003)
    chunks = _fill(chunks)
    bound = max(len(x) for x in chunks)
    for level in range(1, 10):
        fmt = ("deflate", "zlib", "gzip")[level % 3]
        split = _run(fmt, level, chunks, bound)
        assert split == _run(fmt, level, chunks, None), level
        _check(fmt, chunks, split)


@pytest.mark.parametrize("level", [1, 6])
def test_split_path_chunks_above_the_bound(level):
    """the bound is a promise the host cannot check: a chunk above it (every
    input here over 64 KiB) is compressed all the same, by the fused kernel
    behind the split launch, into the fused kernel's bytes - and the
    chunks around it are untouched"""
    chunks = _fill(_inputs())
    assert any(len(x) > 65536 for x in chunks)
    split = _run("gzip", level, chunks, 65536)
    _check("gzip", chunks, split)
    assert split == _run("gzip", level, chunks, None)


_SEG_CHILD = r"""
import sys, zlib
sys.path.insert(0, sys.argv[1])
from libdeflate_amd import api
from tests import datagen, oracle_util
ref = oracle_util.load_ref() or oracle_util.load_oracle()
data = datagen.text_chunk(12 << 20, 41) + datagen.binary_chunk(4 << 20, 42)
dic = datagen.text_chunk(40000, 43)
for level in (1, 6):
    c = api.Compressor(level)
    z = c.compress("gzip", data)
    assert z is not None and zlib.decompress(z, 31) == data
    r, ain, _, got = ref.decompress_ex("gzip", z, len(data))
    assert (r, ain, got) == (0, len(z), data)
    z = c.compress_dict("zlib", dic, data)
    d = zlib.decompressobj(15, zdict=dic)
    assert z is not None and d.decompress(z) + d.flush() == data
    c.close()
print("ok")
"""


def test_split_path_segmented():
    """16 MiB in 8 KiB segments: 2048 segments in one launch, so the split
    path with dictionary tiles in front of every segment but the first, the
    empty stored block behind every segment but the last, and a preset
    dictionary in front of the first"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LDA_SEG_BYTES="8192")
    r = subprocess.run([sys.executable, "-c", _SEG_CHILD, root], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]
