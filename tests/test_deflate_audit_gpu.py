"""Every block the GPU compressor emits, audited (tests/deflate_audit.py).

Each path's streams are walked block by block and checked against exact
references: the code lengths against restated_make_code() and the optimal
costs (huffman_cost, package_merge), the header fields and precode items
against the greedy run-length coding, the emitted bits against the block
end's cost model, the block type against the costs of the other two types,
stored and empty blocks against their documented shapes, and every match
against its canonical length and distance symbols.  The paths:

  batch   the 64 KiB kernel (compress_batch_host, LDA_NO_SMALL set)
  small   the small-buffer kernel (every input <= lda_deflate_small_max(),
          levels <= 9)
  dict    the preset-dictionary batch (raw DEFLATE and zlib)
  seg     the segmented single-buffer path (inputs >= 128 KiB)

Inputs built to drive make_code() to its edges ride along with ordinary
data, and per-path counters assert that the edges were reached: clamped
litlen, precode and distance codes, alphabets below and from 24 used symbols
(the serial and the round merge), fewer than two used distance symbols,
static and stored blocks (WANT lists, per path, the edges these inputs
reach there).  Out of scope: the MERGE_ROUNDS serial takeover of
the round merge (it needs weights near 2^22 within one block, which no input
of a block's size can produce) and the decompressor (fuzzed against the
oracle elsewhere).

Last, one batch per path is run again with out_avail set to each stream's
exact size (slots back to back at odd offsets, canary bytes between them):
every stream comes back byte-identical; with one byte less every one
returns 0 and no byte outside the slots changes.
"""
import hashlib
import random

import numpy as np
import pytest

from tests import datagen
from tests import deflate_audit as A

pytestmark = pytest.mark.gpu

FMTS = ("deflate", "zlib", "gzip")
LEVELS = (0, 1, 6, 9, 10, 12)
SMALL_LEVELS = (0, 1, 6, 9)
SEG_LEVELS = (1, 6, 12)
COVERAGE = {}           # path -> deflate_audit.Coverage
_WALKED = {}            # digest of (raw DEFLATE, dictionary) -> audited already


# ------------------------------------------------------------ edge inputs

def fib_bytes(k, seed, top=None):
    """k byte values with Fibonacci counts 1, 1, 2, 3, 5, ... (the largest
    cut to `top`), shuffled: a litlen tree k - 1 deep"""
    rng = random.Random(seed)
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    if top is not None:
        f[-1] = top
    b = bytearray()
    for v, c in zip(rng.sample(range(256), k), f):
        b += bytes([v]) * c
    rng.shuffle(b)
    return bytes(b)


def geo_bytes(n, ratio, seed):
    """bytes drawn with probabilities ratio^v: code lengths that grow by
    log2(1/ratio) per value, into the clamp"""
    rng = np.random.default_rng(seed)
    p = ratio ** np.arange(256)
    return bytes(rng.choice(256, n, p=p / p.sum()).astype(np.uint8))


def dist_chain(seed, ncodes=24, chain=17, mlen=(4, 5)):
    """32 KiB of random bytes, then matches into them: the farthest distance
    codes get Fibonacci counts (code 29 the most), the next nearer ones one
    match each - a distance alphabet of >= 24 symbols for the round merge,
    whose code lengths spread over the whole precode"""
    rng = random.Random(seed)
    f = [1, 1]
    while len(f) < chain:
        f.append(f[-1] + f[-2])
    counts = {29 - i: f[chain - 1 - i] for i in range(chain)}
    for c in range(30 - ncodes, 30 - chain):
        counts[c] = 1
    pool = [c for c, k in counts.items() for _ in range(k)]
    rng.shuffle(pool)
    out = bytearray(rng.randbytes(32768 + 64))
    for c in pool:
        out += rng.randbytes(1)
        d = rng.randint(A.DIST_BASE[c], A.DIST_BASE[c] + (1 << A.DIST_EXTRA[c]) - 1)
        for _ in range(rng.randint(*mlen)):
            out.append(out[-d])
    return bytes(out)


def few_symbols(n, k, seed):
    """random bytes over k values with no repeat of 3: literal-only blocks
    (fewer than two used distance symbols) - short enough that no trigram
    recurs, so only for small n"""
    rng = random.Random(seed)
    vals = rng.sample(range(256), k)
    out, seen, tries = bytearray(), set(), 0
    while len(out) < n and tries < 1000:
        c = rng.choice(vals)
        if len(out) >= 2 and (out[-2], out[-1], c) in seen:
            tries += 1
            continue
        if len(out) >= 2:
            seen.add((out[-2], out[-1], c))
        out.append(c)
        tries = 0
    return bytes(out)


def ties(n, k, seed):
    """k values, each exactly n // k times, shuffled: equal frequencies"""
    rng = random.Random(seed)
    b = bytearray()
    for v in rng.sample(range(256), k):
        b += bytes([v]) * (n // k)
    rng.shuffle(b)
    return bytes(b)


def edge_inputs(maxn):
    """(name, bytes) of at most maxn bytes each"""
    e = []
    for k in (18, 20, 22):
        e.append(("fib%d" % k, fib_bytes(k, k)))
    e.append(("fib17cut", fib_bytes(17, 17, top=1500)))
    for i, r in enumerate((0.5, 0.6, 0.7, 0.8)):
        e.append(("geo%.1f" % r, geo_bytes(min(maxn, 60000), r, i)))
    e.append(("distchain", dist_chain(1)))
    e.append(("distchain26", dist_chain(2, ncodes=26)))
    e.append(("lit22", few_symbols(4000, 22, 3)))
    e.append(("lit12", few_symbols(1500, 12, 4)))
    for k in (1, 4, 7, 15):
        e.append(("zeros%d" % k, bytes(1 + 258 * k)))
    e.append(("ab", bytes([97, 98]) * 700))
    e.append(("ties24", ties(min(maxn, 24 * 1500), 24, 5)))
    e.append(("ties200", ties(min(maxn, 200 * 150), 200, 6)))
    e.append(("random", datagen.random_chunk(min(maxn, 40000), 7)))
    return [(n, d[:maxn]) for n, d in e]


def plain_inputs(count, n, seed, mix=datagen.MIX64K):
    return [("mix%d" % i, datagen.chunk(i, n, seed, mix)) for i in range(count)]


# ------------------------------------------------------------ audit

def seg_bytes(n):
    """the segment size compress_large() (host_compress.hip) cuts n into"""
    return 16384 if n <= 4 << 20 else 32768 if n <= 8 << 20 else 65536


def audit(path, fmt, stream, data, dictionary=b"", seg=None):
    """walk one stream (a raw DEFLATE body that was audited once already is
    only checked for its round trip), add to the path's counters, fail on a
    violation"""
    assert stream is not None, (path, fmt, len(data))
    cov = COVERAGE.setdefault(path, A.Coverage())
    raw = A.strip_container(stream, fmt)
    key = hashlib.sha1(raw + b"|" + hashlib.sha1(dictionary).digest()).digest()
    if key in _WALKED:
        assert A.zlib_control(stream, fmt, dictionary) == data, (path, fmt)
        return
    out, blocks = A.walk(stream, fmt, dictionary)
    assert out == data, (path, fmt, len(data), "walk does not reproduce the input")
    assert A.zlib_control(stream, fmt, dictionary) == data, (path, fmt)
    bad = A.audit_blocks(blocks, cov, seg)
    assert not bad, (path, fmt, len(data), bad[:5])
    _WALKED[key] = True


def _batch_inputs():
    return (plain_inputs(8, 65536, 0x0E1100C0) + edge_inputs(65536) +
            [(n + "4k", d) for n, d in edge_inputs(4096)[4:10]])


def _small_inputs():
    lim = _small_max()
    sizes = [0, 1, 30, 52, 53, 100, 1000, 2047, 2048, 2049, 4000, lim]
    plain = [("mix4k%d" % i, datagen.chunk(i, n, 0x0E1100C1, datagen.MIX4K))
             for i, n in enumerate(sizes)]
    return plain + edge_inputs(lim)


def _small_max():
    return 4096         # lda_deflate_small_max(): RING of deflate_small.hip


DICT = datagen.text_chunk(32768, 0x0E1100C2)


def _dict_inputs():
    body = datagen.text_chunk(65536, 0x0E1100C3)
    return ([("text", body[:60000]), ("dictcopy", DICT[5000:9000] + body[:3000]),
             ("empty", b""), ("tiny", DICT[:40])] + plain_inputs(4, 50000, 0x0E1100C4) +
            edge_inputs(65536)[::2])


def _seg_inputs():
    lens = [131072, 200001]
    out = []
    for i, n in enumerate(lens):
        d = b"".join(datagen.chunk(i + k, 65536, 0x0E1100C5 + k) for k in range(4))[:n]
        out.append(("seg%d" % n, d))
    out.append(("segzeros", bytes(3 * 65536 + 7)))
    edge = b"".join(d for _, d in edge_inputs(65536)[:10])
    out.append(("segedge", edge))
    return out


@pytest.mark.timeout(600)
@pytest.mark.parametrize("level", LEVELS)
def test_batch_kernel_blocks(level, monkeypatch):
    from libdeflate_amd import api, binding
    monkeypatch.setenv("LDA_NO_SMALL", "1")
    binding.reload_env()
    c = api.Compressor(level)
    inputs = _batch_inputs()
    for fmt in FMTS:
        comps = c.compress_batch_host(fmt, [d for _, d in inputs])
        for (name, d), z in zip(inputs, comps):
            audit("batch", fmt, z, d)
    c.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("level", SMALL_LEVELS)
def test_small_kernel_blocks(level):
    from libdeflate_amd import api
    c = api.Compressor(level)
    inputs = _small_inputs()
    assert max(len(d) for _, d in inputs) <= _small_max()
    for fmt in FMTS:
        comps = c.compress_batch_host(fmt, [d for _, d in inputs])
        for (name, d), z in zip(inputs, comps):
            audit("small", fmt, z, d)
    c.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("level", LEVELS)
def test_dictionary_batch_blocks(level):
    from libdeflate_amd import api
    c = api.Compressor(level)
    inputs = _dict_inputs()
    for fmt in ("deflate", "zlib"):
        comps = _dict_batch(c, fmt, [d for _, d in inputs])
        for (name, d), z in zip(inputs, comps):
            audit("dict", fmt, z, d, DICT)
    c.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("level", SEG_LEVELS)
def test_segmented_blocks(level, monkeypatch):
    from libdeflate_amd import api
    c = api.Compressor(level)
    for name, d in _seg_inputs():
        for fmt in FMTS:
            audit("seg", fmt, c.compress(fmt, d), d, seg=seg_bytes(len(d)))
    c.close()


def _coverage_gate(path, want):
    cov = COVERAGE.get(path)
    assert cov is not None, (path, "no stream audited: run the whole module")
    print("\n%s coverage: %r" % (path, cov))
    missing = [k for k in want if cov[k] == 0]
    assert not missing, (path, "edges never reached", missing, cov)


# the edges each path reaches with the inputs above, as measured on the GPU.
# Not reached on any path: a clamped distance code (the kernel's parse
# spreads the Fibonacci counts of dist_chain() too evenly); a clamped precode
# only on the small-buffer kernel; litlen alphabets of 2-3 symbols not on the
# small-buffer kernel or the dictionary batch
_ALL = ["litlen:m<24", "litlen:m>=24", "dist:m<24", "dist:m>=24", "dist:m<2",
        "litlen:m=22-26", "type0", "type1", "type2"]
WANT = {
    "batch": _ALL + ["litlen:clamped", "litlen:m=2-3"],
    "small": _ALL + ["precode:clamped"],
    "dict": _ALL + ["litlen:clamped"],
    "seg": _ALL + ["litlen:clamped", "litlen:m=2-3", "join"],
}


@pytest.mark.parametrize("path", sorted(WANT))
def test_edges_were_reached(path):
    _coverage_gate(path, WANT[path])


# ------------------------------------------------------------ tight output

def _pack(chunks, dev):
    import torch
    offs, blob = [], bytearray()
    for c in chunks:
        offs.append(len(blob))
        blob += c
        blob += bytes(-len(blob) % 16)
    data = torch.frombuffer(bytearray(blob) + bytearray(64), dtype=torch.uint8).to(dev)
    return (data, torch.tensor(offs, dtype=torch.int64, device=dev),
            torch.tensor([len(c) for c in chunks], dtype=torch.int64, device=dev))


def _dict_tensor(d, dev):
    import torch
    return torch.frombuffer(bytearray(d) + bytearray(1), dtype=torch.uint8)[:len(d)].to(dev)


CANARY = 0xA5
GAP = 13


def _run_slots(c, fmt, chunks, avail, kind, dictionary=b""):
    """one device batch into slots of `avail` bytes packed back to back from
    offset 1 (odd offsets), GAP canary bytes after each; -> (sizes, host
    bytes of the whole output buffer, slot offsets)"""
    import torch
    dev = torch.device("cuda:0")
    data, off, n = _pack(chunks, dev)
    offs, pos = [], 1
    for a in avail:
        offs.append(pos)
        pos += a + GAP
    out = torch.full((pos + 64,), CANARY, dtype=torch.uint8, device=dev)
    ooff = torch.tensor(offs, dtype=torch.int64, device=dev)
    oav = torch.tensor(avail, dtype=torch.int64, device=dev)
    on = torch.full((len(chunks),), -1, dtype=torch.int64, device=dev)
    if kind == "dict":
        c.compress_batch_dict(fmt, _dict_tensor(dictionary, dev), data, off, n, out,
                              ooff, oav, on)
    elif kind == "small":
        c.compress_batch(fmt, data, off, n, out, ooff, oav, on,
                         max_chunk=max(len(x) for x in chunks))
    else:
        c.compress_batch(fmt, data, off, n, out, ooff, oav, on)
    torch.cuda.synchronize()
    return on.cpu().tolist(), out.cpu().numpy(), offs


def _dict_batch(c, fmt, chunks):
    sizes, buf, offs = _run_slots(c, fmt, chunks, [c.bound(fmt, len(x)) + 4 for x in chunks],
                                  "dict", DICT)
    return [buf[o:o + s].tobytes() if s > 0 else None for o, s in zip(offs, sizes)]


def _tight(c, fmt, chunks, kind, dictionary=b""):
    extra = 4 if kind == "dict" else 0
    gen = [c.bound(fmt, len(x)) + extra for x in chunks]
    sizes, buf, offs = _run_slots(c, fmt, chunks, gen, kind, dictionary)
    assert all(s > 0 for s in sizes), (kind, fmt, sizes)
    ref = [buf[o:o + s].tobytes() for o, s in zip(offs, sizes)]
    for z, d in zip(ref, chunks):
        assert A.zlib_control(z, fmt, dictionary) == d
    # exact fit: identical bytes, canaries intact
    got, buf, offs = _run_slots(c, fmt, chunks, sizes, kind, dictionary)
    assert got == sizes, (kind, fmt, got, sizes)
    assert [buf[o:o + s].tobytes() for o, s in zip(offs, sizes)] == ref, (kind, fmt)
    _canaries(buf, offs, sizes, (kind, fmt, "exact"))
    # one byte short: 0 for every buffer, nothing written outside its slot
    short = [s - 1 for s in sizes]
    got, buf, offs = _run_slots(c, fmt, chunks, short, kind, dictionary)
    assert got == [0] * len(chunks), (kind, fmt, got)
    _canaries(buf, offs, short, (kind, fmt, "short"))


def _canaries(buf, offs, sizes, tag):
    assert buf[0] == CANARY, tag
    for o, s in zip(offs, sizes):
        assert (buf[o + s:o + s + GAP] == CANARY).all(), (tag, o, s)
    end = offs[-1] + sizes[-1] + GAP
    assert (buf[end:] == CANARY).all(), tag


@pytest.mark.timeout(300)
def test_tight_output_batch(monkeypatch):
    from libdeflate_amd import api, binding
    monkeypatch.setenv("LDA_NO_SMALL", "1")
    binding.reload_env()
    chunks = [d for _, d in _batch_inputs()[:12] if d]
    for fmt, level in (("deflate", 1), ("zlib", 6), ("gzip", 12)):
        c = api.Compressor(level)
        _tight(c, fmt, chunks, "batch")
        c.close()


@pytest.mark.timeout(300)
def test_tight_output_small():
    from libdeflate_amd import api
    chunks = [d for _, d in _small_inputs()]
    for fmt, level in (("deflate", 0), ("zlib", 6), ("gzip", 9)):
        c = api.Compressor(level)
        _tight(c, fmt, chunks, "small")
        c.close()


@pytest.mark.timeout(300)
def test_tight_output_dictionary():
    from libdeflate_amd import api
    chunks = [d for _, d in _dict_inputs()]
    for fmt, level in (("deflate", 6), ("zlib", 12)):
        c = api.Compressor(level)
        _tight(c, fmt, chunks, "dict", DICT)
        c.close()


@pytest.mark.timeout(300)
def test_tight_output_segmented():
    from libdeflate_amd import api
    c = api.Compressor(6)
    d = _seg_inputs()[1][1]
    for fmt in FMTS:
        z = c.compress(fmt, d)
        assert c.compress(fmt, d, len(z)) == z, fmt
        assert c.compress(fmt, d, len(z) - 1) is None, fmt
    c.close()
