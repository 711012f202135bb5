"""Every device batch call with rows at device offsets at and beyond 4 GiB.

Each test builds its call's small case as that call's near-offset test does,
and tests/far_buffers.py places it three times in ONE call: across 2^31,
across 2^32 and at FAR = 2^32 + 2^31 + 5, the input side in another order than
the written sides.  The tensors are a little over 6 GiB each, filled on the
device.  No tolerance anywhere: every result word and every byte of every
window equal what zlib or the call's CPU model state, and every other byte of
every written tensor - all 6 GiB of it - still is the canary.  That scan is
what catches a write whose offset lost its high word, and
tests/test_far_buffers.py shows on the CPU that it does.

Out of scope: the file walkers that would need more than 4 GiB of real
compressed bytes to get far (ZIP, BGZF, gzip members, the seek index and
.tar.gz - tar alone is walked here, over a sparse archive); the scratch areas
internal to a call; and batches whose TOTAL size exceeds 2^32.
"""
import random
import time
import zlib

import numpy as np
import pytest

from tests import datagen, deflate_synth
from tests import far_buffers as fb
from tests.prefix_expect import _lits, static_stream

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE, PREFIX = 0, 1, 2, 3, 19
UNSET = -7          # the caller's result tensors where nothing was written
ANY = None          # a word nothing is said about


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def api():
    from libdeflate_amd import api
    return api


@pytest.fixture(scope="module")
def dec(api):
    d = api.Decompressor()
    yield d
    d.close()


@pytest.fixture
def far(torch, request):
    """far(tensors): skips only where the card has less free memory than the
    test's far tensors need; frees them afterwards, and prints the free memory
    the test saw and its wall time"""
    held, t0, seen = [], time.time(), []

    def need(tensors):
        free, want = fb.free_memory(torch, tensors)
        seen.append(free)
        if free < want:
            pytest.skip("%.1f GiB free, %.1f GiB needed" % (free / 2**30, want / 2**30))

    need.keep = lambda mem: held.append(mem) or mem
    yield need
    for mem in held:
        mem.free()
    torch.cuda.empty_cache()
    print("\nfar-offsets %s: %.1f GiB free, %.2f s" % (
        request.node.name, (seen[0] if seen else 0) / 2**30, time.time() - t0))


def pack(blobs, seed):
    """the stored bytes at unaligned offsets with junk between them
    -> (buf, spans)"""
    rng = random.Random(seed)
    buf, spans = bytearray(), []
    for b in blobs:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 8)))
        spans.append((len(buf), len(b)))
        buf += b
    buf += b"\x78\x9c" * 5      # behind the last row: never read as part of it
    return bytes(buf), spans


def rooms(sizes, seed):
    """rooms at unaligned offsets with canary gaps in front -> (total, spans)"""
    rng = random.Random(seed)
    at, spans = 0, []
    for n in sizes:
        at += rng.randrange(0, 4)
        spans.append((at, n))
        at += n
    return at, spans


class Batch:
    """The input and output sides of a call whose offsets are int64 tensors:
    three copies of `blobs` read, three copies of `room_sizes` written."""

    def __init__(self, torch, far, blobs, room_sizes, seed=0, out=True):
        self.torch, self.n = torch, len(blobs)
        far(2 if out else 1)
        self.buf, in_spans = pack(blobs, seed)
        pick = None
        if out:
            self.total, self.out_spans = rooms(room_sizes, seed + 1)
            pick = fb.common_row(in_spans, self.out_spans)
        self.inp = fb.Side("in", len(self.buf), in_spans, "ABC", ("mid", "access"), pick)
        self.in_off = self.t64(self.inp.column([o for o, _ in in_spans]))
        self.in_n = self.t64([n for _, n in in_spans] * 3)
        if out:
            self.out = fb.Side("out", self.total, self.out_spans, "CAB", ("access", "mid"), pick)
            fb.assert_placed(self.inp, self.out)
            self.out_off = self.t64(self.out.column([o for o, _ in self.out_spans]))
            self.out_av = self.t64(list(room_sizes) * 3)
            self.d_out = far.keep(fb.device_output(torch, self.out))
        else:
            fb.assert_placed(self.inp)
        self.d_in = far.keep(fb.device_input(torch, self.inp, self.buf))

    def t64(self, v):
        return self.torch.tensor(v, dtype=self.torch.int64, device="cuda")

    def words(self, dtype=None):
        """a result tensor of the caller's: one word per row and a spare one"""
        return self.torch.full((3 * self.n + 1,), UNSET, dtype=dtype or self.torch.int64,
                               device="cuda")

    def results(self):
        return self.words(self.torch.int32)

    def check_words(self, name, t, want, spare=1):
        """want: one per row of the small case (ANY: not said), the same in
        every copy; the spare words behind stay unset"""
        got = t.cpu().tolist()
        assert got[len(got) - spare:] == [UNSET] * spare, (name, "the spare word was written")
        for c in range(3):
            for k, w in enumerate(want):
                assert w is ANY or got[c * self.n + k] == w, (
                    name, "copy %d row %d" % (c, k), got[c * self.n + k], w)

    def check_out(self, plains, written):
        """plains[k] in row k's room where written[k], an undefined room where
        it is None, a room left alone where it is False"""
        want = np.full(self.total, fb.CANARY, dtype=np.uint8)
        defined = np.ones(self.total, dtype=bool)
        for (o, n), p, w in zip(self.out_spans, plains, written):
            if w is None:
                defined[o:o + n] = False
            elif w:
                want[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
                defined[o + len(p):o + n] = False       # room the row did not need
        fb.check_windows(self.d_out, self.out.windows(want, defined))


# ---- the streams of the decompress tests ----

def _fixed(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    return c.compress(data) + c.flush()


def stream_cases():
    """(name, zlib stream, plain, room, result): stored, static and dynamic
    blocks, a match at distance 32768 that reaches the first byte of its room,
    a corrupt stream and a room one byte short"""
    text = datagen.text_chunk(20000, 0x0FA40001)
    rnd = bytes(_lits(3000, 0x0FA4))
    raw, far_plain = static_stream(_lits(32768, 8) + [(20, 32768), 1, 2, (258, 32768)])
    bad = bytearray(zlib.compress(text[:5000], 6))
    bad[-2] ^= 0x40
    return [
        ("stored", zlib.compress(rnd, 0), rnd, len(rnd), SUCCESS),
        ("static", _fixed(text[:2000]), text[:2000], 2000, SUCCESS),
        ("footer", bytes(bad), text[:5000], 5000, BAD_DATA),
        ("dynamic", zlib.compress(text, 6), text, len(text), SUCCESS),
        ("dist32768", deflate_synth.zlib_wrap(raw, far_plain), far_plain, len(far_plain), SUCCESS),
        ("short-room", zlib.compress(text[:4097], 9), text[:4097], 4096, INSUFFICIENT_SPACE),
        ("one", zlib.compress(b"a", 6), b"a", 1, SUCCESS),
    ]


@pytest.fixture(scope="module")
def cases():
    out = stream_cases()
    for name, s, plain, room, want in out:
        if want != BAD_DATA:
            assert zlib.decompress(s) == plain, name
    assert out[0][1][2] & 6 == 0 and out[1][1][2] & 6 == 2 and out[3][1][2] & 6 == 4
    return out


def test_decompress_batch(torch, far, dec, cases):
    b = Batch(torch, far, [c[1] for c in cases], [c[3] for c in cases], seed=1)
    res, ain, aout = b.results(), b.words(), b.words()
    dec.decompress_batch("zlib", b.d_in.t, b.in_off, b.in_n, b.d_out.t, b.out_off, b.out_av, res,
                         ain, aout)
    torch.cuda.synchronize()
    ok = [c[4] == SUCCESS for c in cases]
    b.check_words("results", res, [c[4] for c in cases])
    b.check_words("actual_in", ain, [len(c[1]) if g else ANY for c, g in zip(cases, ok)])
    b.check_words("actual_out", aout, [len(c[2]) if g else ANY for c, g in zip(cases, ok)])
    b.check_out([c[2] for c in cases], [True if g else None for g in ok])


def test_decompress_sizes_batch(torch, far, dec, cases):
    """nothing is written but the words: the footer's checksum is not the
    query's to check, and a stream cut in half is BAD_DATA"""
    blobs = [c[1] for c in cases]
    blobs[5] = blobs[3][:len(blobs[3]) // 2]
    b = Batch(torch, far, blobs, None, seed=2, out=False)
    res, size, ain = b.results(), b.words(), b.words()
    dec.decompress_sizes_batch("zlib", b.d_in.t, b.in_off, b.in_n, res, size, actual_in=ain)
    torch.cuda.synchronize()
    want = [SUCCESS] * len(cases)
    want[5] = BAD_DATA
    b.check_words("results", res, want)
    b.check_words("out_nbytes", size, [len(c[2]) if w == SUCCESS else ANY
                                       for c, w in zip(cases, want)])
    b.check_words("actual_in", ain, [len(s) if w == SUCCESS else ANY for s, w in zip(blobs, want)])


def test_decompress_prefix_batch(torch, far, dec, cases):
    """limits below, at and above the streams' sizes; a cut inside the match
    at distance 32768"""
    limits = [1500, 2000, 5000, 20001, 32790, 4096, 1]
    b = Batch(torch, far, [c[1] for c in cases], limits, seed=3)
    res, ain, aout = b.results(), b.words(), b.words()
    dec.decompress_prefix_batch("zlib", b.d_in.t, b.in_off, b.in_n, b.d_out.t, b.out_off, b.out_av,
                                res, aout, actual_in=ain)
    torch.cuda.synchronize()
    want = [PREFIX, SUCCESS, BAD_DATA, SUCCESS, PREFIX, PREFIX, SUCCESS]
    got = [min(lim, len(c[2])) for c, lim in zip(cases, limits)]
    b.check_words("results", res, want)
    b.check_words("actual_out", aout, [g if w != BAD_DATA else ANY for g, w in zip(got, want)])
    b.check_words("actual_in", ain, [len(c[1]) if w == SUCCESS else 0 if w == PREFIX else ANY
                                     for c, w in zip(cases, want)])
    b.check_out([c[2][:g] for c, g in zip(cases, got)],
                [None if w == BAD_DATA else True for w in want])


def test_decompress_batch_packed(torch, far, dec, cases):
    """the input is far; the call packs the output itself, so it is near"""
    good = [c for c in cases if c[4] != BAD_DATA]
    blobs = [c[1] for c in good]
    cut = 2
    blobs.insert(cut, blobs[2][:len(blobs[2]) // 2])       # BAD_DATA: takes no room
    plains = [c[2] for c in good]
    plains.insert(cut, b"")
    b = Batch(torch, far, blobs, None, seed=4, out=False)
    sizes = [len(p) for p in plains] * 3
    off = [0]
    for n in sizes:
        off.append(off[-1] + (n + 15) // 16 * 16)
    out = torch.full((off[-1] + 256,), fb.CANARY, dtype=torch.uint8, device="cuda")
    res, ain, aout = b.results(), b.words(), b.words()
    offs = torch.full((3 * b.n + 2,), UNSET, dtype=torch.int64, device="cuda")
    dec.decompress_batch_packed("zlib", b.d_in.t, b.in_off, b.in_n, out, offs, res, aout,
                                actual_in=ain, out_align=16, out_capacity=off[-1])
    torch.cuda.synchronize()
    want = [SUCCESS] * b.n
    want[cut] = BAD_DATA
    b.check_words("results", res, want)
    b.check_words("actual_in", ain, [len(s) if w == SUCCESS else 0 for s, w in zip(blobs, want)])
    b.check_words("actual_out", aout, [len(p) for p in plains])
    assert offs.cpu().tolist() == off + [UNSET]
    host = out.cpu().numpy()
    expect = np.full(host.size, fb.CANARY, dtype=np.uint8)
    defined = np.ones(host.size, dtype=bool)
    for k, p in enumerate(plains * 3):
        expect[off[k]:off[k] + len(p)] = np.frombuffer(p, dtype=np.uint8)
        defined[off[k] + len(p):off[k + 1]] = False         # the slots' padding
    bad = np.nonzero((host != expect) & defined)[0]
    assert not bad.size, ("first wrong byte", int(bad[0]))


def _dictionary():
    return datagen.text_chunk(32768, 0x0FA40002)


def _dict_cases():
    """zlib streams with a preset dictionary (Python's zdict): matches into the
    dictionary from the first byte on, a stream longer than a window, one byte,
    a corrupt stream and a room one byte short"""
    d = _dictionary()
    text = datagen.text_chunk(40000, 0x0FA40003)
    plains = [d[100:3100], text, b"z", d[-5000:] + text[:64], text[:4097], text[:9000]]

    def comp(p):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=d)
        return c.compress(p) + c.flush()
    blobs = [comp(p) for p in plains]
    bad = bytearray(blobs[3])
    bad[-1] ^= 1
    blobs[3] = bytes(bad)
    room = [len(p) for p in plains]
    room[4] -= 1
    return d, blobs, plains, room, [SUCCESS, SUCCESS, SUCCESS, BAD_DATA, INSUFFICIENT_SPACE, SUCCESS]


def test_decompress_batch_dict(torch, far, dec):
    d, blobs, plains, room, want = _dict_cases()
    b = Batch(torch, far, blobs, room, seed=5)
    d_dict = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    res, ain, aout = b.results(), b.words(), b.words()
    dec.decompress_batch_dict("zlib", d_dict, b.d_in.t, b.in_off, b.in_n, b.d_out.t, b.out_off,
                              b.out_av, res, ain, aout)
    torch.cuda.synchronize()
    ok = [w == SUCCESS for w in want]
    b.check_words("results", res, want)
    b.check_words("actual_in", ain, [len(s) if g else ANY for s, g in zip(blobs, ok)])
    b.check_words("actual_out", aout, [len(p) if g else ANY for p, g in zip(plains, ok)])
    b.check_out(plains, [True if g else None for g in ok])


def test_decompress_prefix_batch_dict(torch, far, dec):
    d, blobs, plains, room, _ = _dict_cases()
    limits = [1000, 40000, 1, 5064, 4096, 9500]
    b = Batch(torch, far, blobs, limits, seed=6)
    d_dict = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    res, aout = b.results(), b.words()
    dec.decompress_prefix_batch_dict("zlib", d_dict, b.d_in.t, b.in_off, b.in_n, b.d_out.t,
                                     b.out_off, b.out_av, res, aout)
    torch.cuda.synchronize()
    want = [PREFIX, SUCCESS, SUCCESS, BAD_DATA, PREFIX, SUCCESS]
    got = [min(lim, len(p)) for p, lim in zip(plains, limits)]
    b.check_words("results", res, want)
    b.check_words("actual_out", aout, [g if w != BAD_DATA else ANY for g, w in zip(got, want)])
    b.check_out([p[:g] for p, g in zip(plains, got)], [None if w == BAD_DATA else True for w in want])


# ---- compress ----

def _chunks(sizes, seed):
    return [datagen.chunk(i, n, seed) for i, n in enumerate(sizes)]


def _check_compressed(b, c, fmt, chunks, o_n, avail, decode):
    """every chunk's bytes in its room decode to the chunk and fit bound();
    the rooms themselves are the call's to fill, every byte outside them is
    still the canary"""
    b.check_out(chunks, [None] * len(chunks))
    got = o_n.cpu().tolist()
    assert got[-1] == UNSET
    for cp in range(3):
        for k, d in enumerate(chunks):
            n = got[cp * b.n + k]
            where = "copy %d row %d" % (cp, k)
            if avail[k] < c.bound(fmt, len(d)) and n == 0:
                continue        # a room below the bound may be refused
            assert 0 < n <= min(avail[k], c.bound(fmt, len(d))), (where, n)
            at = b.out.at(cp, b.out_spans[k][0])
            assert decode(b.d_out.get(at, at + n).tobytes()) == d, where


@pytest.mark.parametrize("level, bound, kernel", [(6, 4096, "lda_deflate_small_kernel"),
                                                  (1, None, None), (9, None, None)])
def test_compress_batch(torch, far, api, level, bound, kernel):
    """the small-chunk kernel (a bound of 4096) and the 64 KiB kernel: chunks
    of 1, a few, 4096 and 65536 bytes"""
    sizes = [1, 5, 4096, 33, 4095] if bound else [1, 5, 4096, 65536, 33, 65535]
    chunks = _chunks(sizes, 0x0FA40010 + level)
    c = api.Compressor(level)
    try:
        avail = [c.bound("zlib", n) for n in sizes]
        b = Batch(torch, far, chunks, avail, seed=7)
        o_n = b.words()
        c.compress_batch("zlib", b.d_in.t, b.in_off, b.in_n, b.d_out.t, b.out_off, b.out_av, o_n,
                         max_chunk=bound)
        torch.cuda.synchronize()
        if kernel:
            assert c.last_kernel() == kernel
        else:
            assert c.last_kernel() != "lda_deflate_small_kernel"
        _check_compressed(b, c, "zlib", chunks, o_n, avail, zlib.decompress)
    finally:
        c.close()


def test_compress_batch_dict(torch, far, api):
    d = _dictionary()
    chunks = [d[500:2500], datagen.text_chunk(70001, 0x0FA40011), b"q", d[-40:] * 3]
    c = api.Compressor(6)
    try:
        avail = [c.bound("zlib", len(x)) + 4 for x in chunks]
        b = Batch(torch, far, chunks, avail, seed=8)
        o_n = b.words()
        d_dict = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
        c.compress_batch_dict("zlib", d_dict, b.d_in.t, b.in_off, b.in_n, b.d_out.t, b.out_off,
                              b.out_av, o_n)
        torch.cuda.synchronize()

        def decode(z):
            o = zlib.decompressobj(15, zdict=d)
            return o.decompress(z) + o.flush()
        b.check_out(chunks, [None] * len(chunks))
        got = o_n.cpu().tolist()
        assert got[-1] == UNSET
        for cp in range(3):
            for k, x in enumerate(chunks):
                n = got[cp * b.n + k]
                assert 0 < n <= avail[k], (cp, k, n)
                at = b.out.at(cp, b.out_spans[k][0])
                assert decode(b.d_out.get(at, at + n).tobytes()) == x, (cp, k)
    finally:
        c.close()


# ---- checksums and compaction ----

@pytest.mark.parametrize("kind", ["crc32", "adler32"])
def test_checksum_batch(torch, far, api, kind):
    sizes = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1025, 4096, 5552, 5553, 65535, 65536, 65537]
    chunks = _chunks(sizes, 0x0FA40020) + [b"\xff" * 5553]
    b = Batch(torch, far, chunks, None, seed=9, out=False)
    rng = np.random.default_rng(9)
    lo, hi = rng.integers(0, 65521, 3 * b.n), rng.integers(0, 65521, 3 * b.n)
    inits = ((hi << 16) | lo).astype(np.uint32)
    init_t = torch.from_numpy(inits.view(np.int32)).cuda()
    f = zlib.crc32 if kind == "crc32" else zlib.adler32
    for init in (None, init_t):
        out = b.results()
        api.checksum_batch(kind, b.d_in.t, b.in_off, b.in_n, out, init=init)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got[-1] == UNSET
        got = got[:-1].view(np.uint32).tolist()
        for k in range(3 * b.n):
            d = chunks[k % b.n]
            assert got[k] == (f(d) if init is None else f(d, int(inits[k]))), (
                kind, "copy %d row %d" % divmod(k, b.n), len(d))


def test_compact_batch(torch, far, api):
    """the used parts of far slots back to back in a near buffer"""
    sizes = [0, 1, 15, 16, 17, 4096, 65537, 33, 1000]
    chunks = _chunks(sizes, 0x0FA40021)
    b = Batch(torch, far, chunks, None, seed=10, out=False)
    n = 3 * b.n
    lib = api.binding.load()
    cap = int(lib.libdeflate_amd_compact_offsets_len(n))
    total = 3 * sum(sizes)
    offs = torch.full((cap,), UNSET, dtype=torch.int64, device="cuda")
    packed = torch.full((total + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
    api.check(lib.libdeflate_amd_compact_batch(
        n, b.d_in.t.data_ptr(), b.in_off.data_ptr(), b.in_n.data_ptr(), packed.data_ptr(),
        offs.data_ptr(), None), "compact_batch")
    torch.cuda.synchronize()
    want = np.cumsum([0] + sizes * 3).tolist()
    assert offs[:n + 1].cpu().tolist() == want
    assert packed.cpu().numpy().tobytes() == b"".join(chunks) * 3 + bytes([fb.CANARY]) * 64


# ---- the chunk codecs, reading ----

BIG_PITCH = fb.S31 + 3      # row * pitch itself crosses 2^32 at row 2
BIG_AT = fb.S31 // 2        # where that segment's line 0 stands: clear of the three copies


def far_decode(torch, far, items, row_of, lines_of, call, seed, big=None):
    """One decode call of a chunk codec over three far copies of `items`, and
    over `big` - one more row, whose stored bytes lie in the input's copy at
    FAR and whose three lines lie BIG_PITCH apart.  row_of(item, stored_off,
    raw_off) -> the row's words; lines_of(item, row) -> [(offset behind word 2,
    the bytes the CPU model states)]; item.want: the result; item.room: "any"
    (undefined) or "canary" (not written) where the lines are not expected."""
    far(2)
    buf, in_spans = pack([i.stored for i in items] + ([big.stored] if big else []), seed)
    rng = random.Random(seed + 1)
    at, raw_at, extent, near = 0, [], [], []
    for it in items:
        at += rng.randrange(0, 4)
        lines = lines_of(it, row_of(it, 0, 0))
        raw_at.append(at)
        near.append(lines)
        extent.append(max((rel + len(b) for rel, b in lines), default=0))
        at += extent[-1]
    total = at
    out_spans = list(zip(raw_at, extent)) + ([None] if big else [])
    pick = fb.common_row(in_spans, out_spans)
    inp = fb.Side("in", len(buf), in_spans, "ABC", ("mid", "access"), pick)
    out = fb.Side("out", total, out_spans, "CAB", ("access", "mid"), pick)
    fb.assert_placed(inp, out)
    want = np.full(total, fb.CANARY, dtype=np.uint8)
    defined = np.ones(total, dtype=bool)
    for it, a, lines in zip(items, raw_at, near):
        for rel, b in lines:
            if it.room == "any":
                defined[a + rel:a + rel + len(b)] = False
            elif it.room != "canary":
                want[a + rel:a + rel + len(b)] = np.frombuffer(b, dtype=np.uint8)
    rows = [row_of(it, inp.at(c, in_spans[k][0]), out.at(c, raw_at[k]))
            for c in range(3) for k, it in enumerate(items)]
    windows, avail = out.windows(want, defined), out.end
    if big:
        rows.append(row_of(big, inp.at(2, in_spans[-1][0]), BIG_AT))
        lines = lines_of(big, rows[-1])
        assert len(lines) == 3 and lines[2][0] == 2 * BIG_PITCH > fb.S32
        for y, (rel, b) in enumerate(lines):
            windows.append(fb.Window(BIG_AT + rel, b, None, "big pitch line %d" % y, [(0, len(b))]))
        avail = max(avail, windows[-1].end)
    d_in = far.keep(fb.device_input(torch, inp, buf))
    d_out = far.keep(fb.device_output(torch, out))
    assert avail <= d_out.nbytes
    per = torch.full((len(rows) + 1,), UNSET, dtype=torch.int32, device="cuda")
    got_rows = call(rows, d_in.t, d_out.t, per, in_nbytes=inp.end, out_avail=avail)
    assert got_rows.tolist() == rows
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [it.want for it in items] * 3 + ([big.want] if big else []) + [UNSET]
    fb.check_windows(d_out, windows)
    return rows, d_out, inp, out


def test_decompress_shuffle_batch(torch, far, dec):
    """element sizes of the register path (2, 4, 8) and of the LDS path (3,
    16, 255), chunks with trailing bytes, the masks, and the failures"""
    from tests.test_shuffle_read_gpu import Chunk
    from tools.models import shuffle_model as sm
    t4, t3 = sm.tile_elems(4), sm.tile_elems(3)
    items = [Chunk("zlib", 4, (t4 + 1) * 4 + 3), Chunk("zlib", 8, 8 * 17), Chunk("zlib", 1, 50),
             Chunk("zlib", 2, 2 * (2 * sm.tile_elems(2) + 1) + 1), Chunk("zlib", 3, (t3 + 1) * 3 + 2),
             Chunk("zlib", 16, 16 * 17 + 15), Chunk("zlib", 255, 255 * 17 + 1), Chunk("zlib", 4, 0),
             Chunk("zlib", 5, 5 * 33 + 4, sm.NO_DEFLATE), Chunk("zlib", 4, 4 * 1000 + 1, sm.NO_SHUFFLE),
             Chunk("zlib", 1, 77, sm.NO_DEFLATE)]
    bad = Chunk("zlib", 4, 4 * 300 + 2)
    s = bytearray(bad.stored)
    s[-1] ^= 0x10
    bad.stored, bad.want, bad.room = bytes(s), BAD_DATA, "any"
    items.insert(3, bad)
    long = Chunk("zlib", 8, 8 * 100 + 1)
    long.raw_n, long.want, long.room = 8 * 100, INSUFFICIENT_SPACE, "any"
    items.insert(6, long)
    assert {sm.classify([0, len(c.stored), 0, c.raw_n, c.es, c.mask]) for c in items} >= {
        sm.DECODE_DIRECT, sm.DECODE_UNSHUFFLE, sm.STORED_UNSHUFFLE, sm.STORED_COPY}
    far_decode(torch, far, items,
               lambda c, so, ro: [so, len(c.stored), ro, c.raw_n, c.es, c.mask],
               lambda c, r: [(0, c.raw[:c.raw_n])],
               lambda *a, **kw: dec.decompress_shuffle_batch("zlib", *a, **kw), seed=11)


def _tiff_lines(s, r):
    from tools.models import tiff_model as tm
    return [(y * int(r[3]), line) for y, line in enumerate(tm.expected(r, s.pixels))]


def test_decode_tiff_batch(torch, far, dec):
    """predictors 1, 2 and 3, register and generic pixel sizes, kept
    rectangles smaller than the coded ones, pitch gaps, a failure - and a
    segment of three rows BIG_PITCH apart"""
    from tests.test_tiff_read_gpu import Seg
    from tools.models import tiff_model as tm
    items = [Seg(3, 1, 1, (40, 5), (33, 4), 0, seed=1), Seg(1, 2, 1, (700, 3), (700, 3), 7, seed=2),
             Seg(1, 1, 1, (100, 4), seed=3),                    # direct
             Seg(3, 1, 2, (65, 17), (60, 16), 5, seed=4), Seg(4, 2, 2, (129, 3), None, 16, seed=5),
             Seg(5, 1, 2, (33, 2), (32, 2), 1, seed=6), Seg(1, 1, 2, (4097, 2), seed=7),
             Seg(1, 4, 3, (70, 9), (64, 8), 3, seed=8), Seg(3, 2, 3, (17, 65), None, 0, seed=9),
             Seg(1, 8, 3, (513, 2), (512, 1), 0, seed=10)]
    bad = Seg(2, 2, 2, (50, 6), None, 2, seed=11)
    s = bytearray(bad.stored)
    s[-1] ^= 0x10
    bad.stored, bad.want, bad.room = bytes(s), BAD_DATA, "any"
    items.insert(4, bad)
    assert {tm.classify(s.row(0, 0)) for s in items} == {tm.DIRECT, tm.SCAN, tm.SCAN_GATHER}
    big = Seg(3, 1, 2, (47, 4), (45, 3), BIG_PITCH - 45 * 3, seed=12)
    far_decode(torch, far, items, lambda s, so, ro: s.row(so, ro), _tiff_lines, dec.decode_tiff_batch,
               seed=12, big=big)


def _exr_lines(c, r):
    from tools.models import exr_model as em
    return [(y * int(r[3]), line) for y, line in enumerate(em.expected(r, c.raw))]


def test_decode_exr_batch(torch, far, dec):
    """LINES and PIXELS, zlib chunks and raw ones, HALF and FLOAT channels,
    pitch gaps, a failure - and a chunk of three lines BIG_PITCH apart"""
    from tests import exr_chunks as ec
    from tools.models import exr_model as em
    H, F = ec.H, ec.F
    items = [ec.Chunk([H], (em.TILE // 2 + 1, 1), few=True, seed=1),
             ec.Chunk([H], (33, 2), em.LINES, extra=5, few=False, seed=2),
             ec.Chunk([H], (32, 1), em.LINES, few=False, seed=3),
             ec.Chunk([H, H, H], (31, 17), em.PIXELS, [2, 1, 0], extra=7, few=True, seed=4),
             ec.Chunk([F, F, F, F], (9, 16), em.LINES, extra=16, few=True, seed=5),
             ec.Chunk([H, H, H, H, F], (64, 15), em.PIXELS, [4, 3, 2, 1, 0], few=True, seed=6),
             ec.Chunk([H] * 5, (7, 2), em.PIXELS, None, extra=3, few=False, seed=7),
             ec.Chunk([H] * 4, (64, 64), em.PIXELS, [3, 2, 1, 0], extra=24, few=True, seed=8)]
    bad = ec.Chunk([H, H, H], (40, 4), em.PIXELS, [0, 1, 2], few=True, seed=9)
    s = bytearray(bad.stored)
    s[-1] ^= 0x10
    bad.stored, bad.want, bad.room = bytes(s), BAD_DATA, "any"
    items.insert(2, bad)
    assert {em.classify(c.row(0, 0)) for c in items} == {em.RAW_DIRECT, em.RAW_LAYOUT, em.ZLIB}
    big = ec.Chunk([H] * 4, (40, 3), em.PIXELS, [3, 2, 1, 0], extra=BIG_PITCH - 320, few=True, seed=10)
    assert big.pitch == BIG_PITCH and em.classify(big.row(0, 0)) == em.ZLIB
    far_decode(torch, far, items, lambda c, so, ro: c.row(so, ro), _exr_lines, dec.decode_exr_batch,
               seed=13, big=big)


# ---- Parquet ----

def far_parquet(torch, far, dec, pages, seed, strings):
    """One call over three far copies of the pages: d_out and d_valid far too,
    and every dictionary-coded page names the dictionary row of ANOTHER copy
    (the dictionary rows go first: a dictionary is an earlier row).  The
    expectation is the CPU model's of the same rows over three near copies.
    strings: parquet_decode_batch_ex behind its sizing call; d_bytes is packed
    by the call and stays near."""
    from tests import parquet_pages as pp
    from tests import parquet_string_pages as psp
    from tools.models import parquet_model as pm
    from tools.models import parquet_strings_model as sm
    far(3)
    buf, rows, out_n, valid_n = (psp if strings else pp).lay_out(pages, random.Random(seed))
    n, size, step = len(rows), len(buf), (out_n + 7) // 8 * 8
    f = [(sm if strings else pm).unpack(r) for r in rows]
    is_dict = [x["kind"] == pm.DICT for x in f]
    order = [(c, k) for c in range(3) for k in range(n) if is_dict[k]] + \
            [(c, k) for c in range(3) for k in range(n) if not is_dict[k]]
    index = {ck: i for i, ck in enumerate(order)}

    def build(in_at, out_at, valid_at):
        res = []
        for c, k in order:
            r = [int(x) for x in rows[k]]
            r[0] = in_at(c, r[0])
            if not is_dict[k]:
                r[5] = out_at(c, r[5])
                if f[k]["max_def"]:
                    r[6] = valid_at(c, r[6])
                if f[k]["enc"] != pm.PLAIN:
                    r[7] = index[(c + 1) % 3, r[7]]
            res.append(r)
        return np.array(res, dtype=np.uint64).reshape(-1, pm.WORDS)
    near = build(lambda c, o: o + c * size, lambda c, o: o + c * step, lambda c, o: o + c * valid_n)
    if strings:
        room = sm.decode(near, buf * 3, "gzip", 3 * step, 3 * valid_n, 0)["total"]
        m = sm.decode(near, buf * 3, "gzip", 3 * step, 3 * valid_n, room, fb.CANARY)
        m = (m["results"], m["out"], m["valid"], m["out_defined"], m["valid_defined"], m)
    else:
        m = pm.decode(near, buf * 3, "gzip", 3 * step, 3 * valid_n, fb.CANARY)
    assert set(m[0]) == {SUCCESS, BAD_DATA}

    in_spans = [(int(r[0]), int(r[1])) for r in rows]
    out_spans = [None if is_dict[k] else
                 (int(r[5]), (f[k]["count"] + 1) * 8 if strings and f[k].get("byte_array")
                  else f[k]["count"] * f[k]["width"]) for k, r in enumerate(rows)]
    valid_spans = [(int(r[6]), f[k]["count"]) if not is_dict[k] and f[k]["max_def"] else None
                   for k, r in enumerate(rows)]
    pick = fb.common_row(in_spans, out_spans, valid_spans)
    inp = fb.Side("in", size, in_spans, "ABC", ("mid", "access"), pick)
    out = fb.Side("out", out_n, out_spans, "CAB", ("access", "mid"), pick, align=8 if strings else 1)
    valid = fb.Side("valid", valid_n, valid_spans, "CAB", ("access", "mid"), pick)
    fb.assert_placed(inp, out, valid)
    far_rows = build(inp.at, out.at, valid.at)
    d_in = far.keep(fb.device_input(torch, inp, buf))
    d_out = far.keep(fb.device_output(torch, out))
    d_valid = far.keep(fb.device_output(torch, valid))
    per = torch.full((3 * n + 1,), UNSET, dtype=torch.int32, device="cuda")
    kw = dict(in_nbytes=inp.end, out_avail=out.end, valid_avail=valid.end)
    if strings:
        total = torch.full((3,), UNSET, dtype=torch.int64, device="cuda")
        dec.parquet_decode_batch_ex("gzip", far_rows, d_in.t, d_out.t, d_valid.t, None, total[1:2],
                                    per, bytes_avail=0, **kw)
        torch.cuda.synchronize()
        assert total.cpu().tolist() == [UNSET, room, UNSET]
        d_bytes = torch.full((room + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
        got = dec.parquet_decode_batch_ex("gzip", far_rows, d_in.t, d_out.t, d_valid.t, d_bytes,
                                          total[1:2], per, bytes_avail=room, **kw)
    else:
        got = dec.parquet_decode_batch("gzip", far_rows, d_in.t, d_out.t, d_valid.t, per, **kw)
    torch.cuda.synchronize()
    assert (got == far_rows).all()
    assert per.cpu().tolist() == list(m[0]) + [UNSET]
    fb.check_windows(d_out, out.windows([m[1][c * step:c * step + out_n] for c in range(3)],
                                        [m[3][c * step:c * step + out_n] for c in range(3)]))
    fb.check_windows(d_valid, valid.windows(
        [m[2][c * valid_n:(c + 1) * valid_n] for c in range(3)],
        [m[4][c * valid_n:(c + 1) * valid_n] for c in range(3)]))
    if strings:
        assert total.cpu().tolist() == [UNSET, room, UNSET]
        host = d_bytes.cpu().numpy()
        assert not (host[room:] != fb.CANARY).any(), "bytes written behind bytes_avail"
        bad = np.nonzero((host[:room] != m[5]["data"]) & m[5]["data_defined"])[0]
        assert not bad.size, ("d_bytes: first wrong byte", int(bad[0]))


def test_parquet_decode_batch(torch, far, dec):
    """PLAIN and dictionary pages, V1 and V2, with nulls and without, a page
    that is not compressed and one that fails"""
    from tests import parquet_pages as pp
    from tests.test_parquet_pages_gpu import T, entries_of, mask_of
    rng = random.Random(21)
    entries = entries_of(rng, 300, 4)
    d = pp.dict_page(entries)
    bad = pp.data_page(rng, 1, 4, mask=mask_of(rng, 40))[0]
    bad.stored = bad.stored[:-5] + bytes([bad.stored[-5] ^ 0x10]) + bad.stored[-4:]
    pages = [d, pp.data_page(rng, 1, 4, n=65)[0],
             pp.data_page(rng, 2, 8, mask=mask_of(rng, T + 1))[0],
             pp.data_page(rng, 1, 4, mask=mask_of(rng, 2 * T + 3), dictionary=d, entries=entries,
                          shape="alt", level_shape="alt")[0], bad,
             pp.data_page(rng, 2, 4, n=T - 1, dictionary=d, entries=entries)[0],
             pp.data_page(rng, 2, 2, mask=mask_of(rng, 9), compress=False)[0],
             pp.data_page(rng, 2, 4, mask=mask_of(rng, 63), dictionary=d, entries=entries)[0],
             pp.data_page(rng, 1, 16, mask=mask_of(rng, 64))[0]]
    far_parquet(torch, far, dec, pages, 21, strings=False)


def test_parquet_decode_batch_ex(torch, far, dec):
    """BYTE_ARRAY pages, PLAIN and dictionary, V1 and V2, required and with
    nulls, next to a fixed-width page: far input, far offsets rooms, far
    validity"""
    from tests import parquet_pages as pp
    from tests import parquet_string_pages as psp
    from tests.test_parquet_pages_gpu import T, mask_of
    from tests.test_parquet_strings_pages_gpu import with_nulls, words
    rng = random.Random(22)
    entries = words(rng, 7, 1, 9)
    d = psp.dict_page(entries)
    long = bytes(rng.randrange(256) for _ in range(3000))
    bad = psp.data_page(rng, 2, with_nulls(rng, words(rng, 30)))
    bad.stored = bad.stored[:-5] + bytes([bad.stored[-5] ^ 0x10]) + bad.stored[-4:]
    pages = [d, psp.data_page(rng, 1, with_nulls(rng, words(rng, T + 1))),
             psp.data_page(rng, 2, [entries[rng.randrange(7)] for _ in range(T)], d, required=True),
             pp.data_page(rng, 1, 4, mask=mask_of(rng, 65))[0], bad,
             psp.data_page(rng, 1, with_nulls(rng, [entries[rng.randrange(7)] for _ in range(T - 1)]),
                           d, shape="alt", level_shape="alt"),
             psp.data_page(rng, 2, with_nulls(rng, [b"a", b"", long, b"c"] * 3)),
             psp.data_page(rng, 1, [b"only"], required=True, compress=False)]
    far_parquet(torch, far, dec, pages, 22, strings=True)


# ---- the chunk codecs, writing ----

def far_encode(torch, far, words, result_words, items, row_of, lines_of, encode, model_lines,
               decode, seed, big=None):
    """One encode call of a chunk codec over raw bytes at far offsets and
    pitches: three copies of `items` and `big`, whose three lines lie BIG_PITCH
    apart.  The call packs its output itself, so that is near.  The index must
    echo every word from 2 on, high words intact; the streams it names are
    read back by the CPU model (model_lines(item, index row, stored bytes) ->
    the lines) and by the matching decode call into a near buffer."""
    far(1)
    rng = random.Random(seed)
    at, raw_at, extent, near = 0, [], [], []
    for it in items:
        at += rng.randrange(1, 8)
        lines = lines_of(it, row_of(it, 0))
        raw_at.append(at)
        near.append(lines)
        extent.append(max(rel + len(b) for rel, b in lines))
        at += extent[-1]
    buf = bytearray(rng.randrange(256) for _ in range(at + 4))      # junk in every gap
    for a, lines in zip(raw_at, near):
        for rel, b in lines:
            buf[a + rel:a + rel + len(b)] = b
    inp = fb.Side("raw", len(buf), list(zip(raw_at, extent)), "ABC", ("mid", "access"))
    fb.assert_placed(inp)
    d_in = far.keep(fb.device_input(torch, inp, bytes(buf)))
    rows = [row_of(it, inp.at(c, raw_at[k])) for c in range(3) for k, it in enumerate(items)]
    every = [(it, lines) for _ in range(3) for it, lines in zip(items, near)]
    avail = inp.end
    if big:
        rows.append(row_of(big, BIG_AT))
        lines = lines_of(big, rows[-1])
        assert len(lines) == 3 and lines[2][0] == 2 * BIG_PITCH > fb.S32
        for rel, b in lines:
            d_in.put(BIG_AT + rel, b)
        every.append((big, lines))
        avail = max(avail, BIG_AT + lines[2][0] + len(lines[2][1]))
    assert avail <= d_in.nbytes
    n = len(rows)
    rows = np.array(rows, dtype=np.uint64).reshape(n, words)
    bound = encode.bound(rows)
    d_out = torch.full((bound + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
    result = torch.full((result_words + 1,), UNSET, dtype=torch.int64, device="cuda")
    index = torch.full((words * n + 1,), UNSET, dtype=torch.int64, device="cuda")
    got_rows = encode(rows, d_in.t, d_out, result, index, in_avail=avail, out_avail=bound)
    torch.cuda.synchronize()
    assert (got_rows == rows).all()
    res, host = result.cpu().tolist(), d_out.cpu().numpy()
    idx = index.cpu().numpy()
    assert res[result_words] == UNSET and idx[words * n] == UNSET
    idx = idx[:words * n].view(np.uint64).reshape(n, words)
    raw_total = sum(len(b) for _, lines in every for _, b in lines)
    assert res[0] == SUCCESS and res[2:4] == [raw_total, n] and 0 < res[1] <= bound
    assert not (host[res[1]:] != fb.CANARY).any(), "bytes written behind the streams"
    assert idx[:, 2:].tolist() == rows[:, 2:].tolist(), "the index does not echo the rows"
    at = 0
    for k, (it, lines) in enumerate(every):
        a, size = int(idx[k, 0]), int(idx[k, 1])
        assert at <= a and a + size <= res[1], ("row %d" % k, a, size)
        at = a + size
        assert model_lines(it, idx[k], host[a:a + size].tobytes()) == [b for _, b in lines], \
            "row %d: the CPU model reads other bytes back" % k
    # the matching decode call, the lines packed into a near buffer
    back_rows, want, at = idx.copy(), bytearray(), 0
    for k, (it, lines) in enumerate(every):
        back_rows[k, 2] = at
        if len(lines) > 1:
            back_rows[k, 3] = len(lines[0][1])
        for _, b in lines:
            want += b
        at += sum(len(b) for _, b in lines)
    back = torch.full((at + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((n + 1,), UNSET, dtype=torch.int32, device="cuda")
    decode(back_rows, d_out, back, per, in_nbytes=res[1], out_avail=at)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [SUCCESS] * n + [UNSET]
    assert back.cpu().numpy().tobytes() == bytes(want) + bytes([fb.CANARY]) * 64


def _encoder(call, bound):
    """the encode call with its bound call beside it"""
    def run(*a, **kw):
        return call(*a, **kw)
    run.bound = bound
    return run


def test_compress_shuffle_batch(torch, far, api, dec):
    from tests.shuffle_chunks import raw_bytes
    from tools.models import shuffle_model as sm
    t4, t3 = sm.tile_elems(4), sm.tile_elems(3)
    items = [(4, (t4 + 1) * 4 + 3, 0), (8, 8 * 17, 0), (1, 50, 0), (2, 2 * (2 * sm.tile_elems(2) + 1) + 1, 0),
             (3, (t3 + 1) * 3 + 2, 0), (16, 16 * 17 + 15, 0), (255, 255 * 17 + 1, 0),
             (4, 4 * 1000 + 1, sm.NO_SHUFFLE), (5, 1, 0)]

    def model_lines(it, r, stored):
        body = zlib.decompress(stored)
        return [body if sm.identity(it[1], it[0], it[2]) else sm.unshuffle(body, it[0])]
    c = api.Compressor(6)
    try:
        far_encode(torch, far, sm.WORDS, sm.RESULT_WORDS, items,
                   lambda it, ro: [0, 0, ro, it[1], it[0], it[2]],
                   lambda it, r: [(0, raw_bytes(it[0], it[1]))],
                   _encoder(lambda *a, **kw: c.compress_shuffle_batch("zlib", *a, **kw),
                            lambda rows: c.shuffle_compress_bound("zlib", rows)),
                   model_lines, lambda *a, **kw: dec.decompress_shuffle_batch("zlib", *a, **kw),
                   seed=31)
    finally:
        c.close()


def test_encode_tiff_batch(torch, far, api, dec):
    from tests.test_tiff_write_gpu import Case
    from tools.models import tiff_model as tm
    items = [Case(3, 1, 1, (40, 5), (33, 4), 0, seed=1), Case(1, 2, 1, (700, 3), (700, 3), 7, seed=2),
             Case(3, 1, 2, (65, 17), (60, 16), 5, seed=3, smooth=True),
             Case(4, 2, 2, (129, 3), (129, 3), 16, seed=4), Case(5, 1, 2, (33, 2), (32, 2), 1, seed=5),
             Case(1, 1, 2, (4097, 2), (4097, 2), 0, seed=6, smooth=True),
             Case(1, 4, 3, (70, 9), (64, 8), 3, seed=7), Case(3, 2, 3, (17, 65), (17, 65), 0, seed=8),
             Case(1, 8, 3, (513, 2), (512, 1), 0, seed=9)]
    big = Case(3, 1, 2, (47, 4), (45, 3), BIG_PITCH - 45 * 3, seed=10, smooth=True)

    def lines_of(c, r):
        return [(y * (c.kept_rb + c.extra), c.pixels[y * c.kept_rb:(y + 1) * c.kept_rb])
                for y in range(c.kept[1])]

    def model_lines(c, r, stored):
        pix = tm.crop(tm.undo(zlib.decompress(stored), c.coded[1], c.coded[0], c.spp, c.bps, c.pred),
                      c.kept, c.coded, c.spp, c.bps)
        return [pix[y * c.kept_rb:(y + 1) * c.kept_rb] for y in range(c.kept[1])]
    c = api.Compressor(6)
    try:
        far_encode(torch, far, tm.WORDS, tm.RESULT_WORDS, items,
                   lambda s, ro: tm.row(0, 0, ro, s.kept_rb + s.extra, s.coded, s.kept, s.spp, s.bps,
                                        s.pred),
                   lines_of, _encoder(c.encode_tiff_batch, c.tiff_encode_bound), model_lines,
                   dec.decode_tiff_batch, seed=32, big=big)
    finally:
        c.close()


def test_encode_exr_batch(torch, far, api, dec):
    from tests import exr_chunks as ec
    from tools.models import exr_model as em
    H, F = ec.H, ec.F
    items = [ec.Chunk([H], (em.TILE // 2 + 1, 1), few=True, seed=1),
             ec.Chunk([H], (33, 2), em.LINES, extra=5, few=False, seed=2),
             ec.Chunk([H, H, H], (31, 17), em.PIXELS, [2, 1, 0], extra=7, few=True, seed=3),
             ec.Chunk([F, F, F, F], (9, 16), em.LINES, extra=16, few=True, seed=4, head=(7,)),
             ec.Chunk([H, H, H, H, F], (64, 15), em.PIXELS, [4, 3, 2, 1, 0], few=True, seed=5),
             ec.Chunk([H] * 5, (7, 2), em.PIXELS, None, extra=3, few=False, seed=6),
             ec.Chunk([H] * 4, (64, 64), em.PIXELS, [3, 2, 1, 0], extra=24, few=True, seed=7,
                      head=(1, 2, 0, 0))]
    big = ec.Chunk([H] * 4, (40, 3), em.PIXELS, [3, 2, 1, 0], extra=BIG_PITCH - 320, few=True, seed=8)

    def model_lines(c, r, data):
        raw = em.undo(zlib.decompress(data)) if len(data) < c.n else data
        return em.expected(r, raw)
    c = api.Compressor(6)
    try:
        far_encode(torch, far, em.WORDS, em.RESULT_WORDS, items,
                   lambda ch, ro: ch.row(0, ro, 0),
                   lambda ch, r: [(y * ch.pitch, line) for y, line in enumerate(ch.lines())],
                   _encoder(c.encode_exr_batch, c.exr_encode_bound), model_lines,
                   dec.decode_exr_batch, seed=33, big=big)
    finally:
        c.close()


# ---- the writers that take records ----

def _records(torch, far):
    """records at far offsets, host columns: sizes 1, 33, 4096, 70001 and 0"""
    chunks = [datagen.text_chunk(n, 0x0FA40030 + n) for n in (1, 33, 4096, 70001)] + [b""]
    b = Batch(torch, far, chunks, None, seed=41, out=False)
    offs = np.array(b.inp.column([o for o, _ in b.inp.spans]), dtype=np.uint64)
    sizes = np.array([len(c) for c in chunks] * 3, dtype=np.uint64)
    names = ["copy%d/record%d.txt" % (c, k) for c in range(3) for k in range(len(chunks))]
    return b, chunks * 3, names, offs, sizes


def test_compress_zip_batch(torch, far, api):
    import io
    import zipfile
    b, records, names, offs, sizes = _records(torch, far)
    n = len(records)
    c = api.Compressor(6)
    try:
        bound = c.zip_bound(names, sizes)
        out = torch.full((bound + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
        result = torch.full((api.binding.ZIPW_RESULT_WORDS + 1,), UNSET, dtype=torch.int64,
                            device="cuda")
        index = torch.full((api.binding.ZIP_WORDS * n + 1,), UNSET, dtype=torch.int64, device="cuda")
        c.compress_zip_batch(names, b.d_in.t, offs, sizes, out, result, index, in_avail=b.inp.end,
                             out_avail=bound)
        torch.cuda.synchronize()
    finally:
        c.close()
    res, host = result.cpu().tolist(), out.cpu().numpy()
    assert res[0] == SUCCESS and 0 < res[1] <= bound and res[-1] == UNSET
    assert index.cpu().tolist()[-1] == UNSET
    assert not (host[res[1]:] != fb.CANARY).any(), "bytes written behind the archive"
    z = zipfile.ZipFile(io.BytesIO(host[:res[1]].tobytes()))
    assert z.testzip() is None and z.namelist() == names
    assert [z.read(name) for name in names] == records


def test_gzip_members_compress(torch, far, api):
    import gzip
    b, records, names, offs, sizes = _records(torch, far)
    n = len(records)
    c = api.Compressor(6)
    try:
        bound = c.gzip_members_compress_bound(sizes, names)
        out = torch.full((bound + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
        result = torch.full((api.binding.GZMW_RESULT_WORDS + 1,), UNSET, dtype=torch.int64,
                            device="cuda")
        index = torch.full((2 * (n + 1) + 1,), UNSET, dtype=torch.int64, device="cuda")
        c.gzip_members_compress((b.d_in.t, offs, sizes), names, out=out, result=result, index=index,
                                in_avail=b.inp.end, out_avail=bound)
        torch.cuda.synchronize()
    finally:
        c.close()
    res, host = result.cpu().tolist(), out.cpu().numpy()
    idx = index.cpu().tolist()
    assert res[0] == SUCCESS and 0 < res[1] <= bound and res[2:4] == [int(sizes.sum()), n]
    assert res[-1] == UNSET and idx[-1] == UNSET
    assert not (host[res[1]:] != fb.CANARY).any(), "bytes written behind the file"
    data = host[:res[1]].tobytes()
    assert gzip.decompress(data) == b"".join(records)
    pairs = np.array(idx[:-1]).reshape(n + 1, 2)
    assert pairs[:, 1].tolist() == np.cumsum([0] + [len(r) for r in records]).tolist()
    assert pairs[0, 0] == 0 and pairs[n, 0] == res[1]
    for k, r in enumerate(records):     # every member alone
        assert gzip.decompress(data[pairs[k, 0]:pairs[k + 1, 0]]) == r, k


def _check_tar(blob, names, records):
    import io
    import tarfile
    with tarfile.open(fileobj=io.BytesIO(blob)) as t:
        members = t.getmembers()
        assert [m.name for m in members] == names
        assert [t.extractfile(m).read() for m in members] == records


def test_write_tar_batch(torch, far, api):
    b, records, names, offs, sizes = _records(torch, far)
    c = api.Compressor(6)
    try:
        size = c.tar_write_size(names, sizes)
        out = torch.full((size + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
        rows = c.write_tar_batch(names, b.d_in.t, offs, sizes, out, in_avail=b.inp.end,
                                 out_avail=size)
        torch.cuda.synchronize()
    finally:
        c.close()
    host = out.cpu().numpy()
    assert not (host[size:] != fb.CANARY).any(), "bytes written behind the archive"
    _check_tar(host[:size].tobytes(), names, records)
    assert rows[:, 5].tolist() == sizes.tolist()
    for r, rec in zip(rows, records):   # the index names the bodies
        assert host[int(r[4]):int(r[4]) + int(r[5])].tobytes() == rec


def test_compress_targz_batch(torch, far, api):
    import gzip
    b, records, names, offs, sizes = _records(torch, far)
    c = api.Compressor(6)
    try:
        bound = c.bound("gzip", c.tar_write_size(names, sizes))
        out = torch.full((bound + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
        o_n = torch.full((2,), UNSET, dtype=torch.int64, device="cuda")
        rows = c.compress_targz_batch("gzip", names, b.d_in.t, offs, sizes, out, o_n,
                                      in_avail=b.inp.end, out_avail=bound)
        torch.cuda.synchronize()
    finally:
        c.close()
    n, spare = o_n.cpu().tolist()
    host = out.cpu().numpy()
    assert 0 < n <= bound and spare == UNSET
    assert not (host[n:] != fb.CANARY).any(), "bytes written behind the stream"
    _check_tar(gzip.decompress(host[:n].tobytes()), names, records)
    assert rows[:, 5].tolist() == sizes.tolist()


# ---- one file reader ----

def test_tar_reader_over_a_sparse_archive(torch, far, dec):
    """index_tar_batch and read_tar_batch on an archive whose first entry
    declares a body of 2^32 + 12345 bytes - zeros on the device, never built
    on the host - with five small entries behind it.  One of them straddles
    the next 2^31 boundary, 2^32 + 2^31: a second body of zeros in front of it
    takes the walk there.  Only the small ones are selected."""
    from tests import tar_files as tf
    far(1)
    small = [tf.payload(n, 0x0FA40040 + n) for n in (1000, 70001, 3000, 1, 513)]
    edge = fb.S32 + fb.S31
    entries, at = [], 0                 # (header offset, name, size, bytes or None)

    def add(name, data=None, size=None):
        nonlocal at
        size = len(data) if data is not None else size
        entries.append((at, name, size, data))
        at += tf.BLOCK + size + (-size % tf.BLOCK)
    add(b"zeros/first", size=fb.S32 + 12345)
    add(b"small/0", small[0])
    add(b"small/1", small[1])
    add(b"zeros/second", size=edge - 3 * tf.BLOCK - (at + tf.BLOCK))
    add(b"small/2-across", small[2])
    add(b"small/3", small[3])
    add(b"small/4", small[4])
    total = at + 2 * tf.BLOCK
    assert entries[4][0] + tf.BLOCK < edge < entries[4][0] + tf.BLOCK + 3000
    assert all(e[0] >= fb.S32 for e in entries[1:]) and entries[5][0] > edge
    data = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    for off, name, size, body in entries:
        rec = tf.header(name, size=size) + (body or b"")
        data[off:off + len(rec)] = torch.frombuffer(bytearray(rec), dtype=torch.uint8).cuda()
    m, cap = len(entries), 16
    res = torch.full((6,), UNSET, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * cap + 1,), UNSET, dtype=torch.int64, device="cuda")
    per = torch.full((cap + 1,), UNSET, dtype=torch.int32, device="cuda")
    dec.index_tar_batch(data, cap, res, per, index=idx, in_nbytes=total)
    torch.cuda.synchronize()
    words = res.cpu().tolist()
    assert words[:2] == [SUCCESS, m] and words[3] == sum(e[2] for e in entries) and words[5] == UNSET
    assert per.cpu().tolist() == [SUCCESS] * m + [UNSET] * (cap + 1 - m)
    rows = idx.cpu().numpy()
    assert (rows[8 * m:] == UNSET).all()
    rows = rows[:8 * m].reshape(m, 8)
    out_off = np.cumsum([0] + [e[2] for e in entries]).tolist()
    for k, (off, name, size, body) in enumerate(entries):
        assert [int(rows[k, w]) for w in (0, 4, 5, 7)] == [off, off + tf.BLOCK, size, out_off[k]], k
    sel = [4, 1, 6, 2, 5, 4]
    want = b"".join(entries[k][3] for k in sel)
    out = torch.full((len(want) + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
    got = torch.full((len(sel) + 1,), UNSET, dtype=torch.int32, device="cuda")
    offs = dec.read_tar_batch(data, rows, sel, out, got, in_nbytes=total, out_avail=len(want))
    torch.cuda.synchronize()
    assert offs.tolist() == np.cumsum([0] + [entries[k][2] for k in sel]).tolist()
    assert got.cpu().tolist() == [SUCCESS] * len(sel) + [UNSET]
    assert out.cpu().numpy().tobytes() == want + bytes([fb.CANARY]) * 64
    del data


# ---- PNG reading ----

def test_png_index_and_decode(torch, far, api, dec):
    """index_png_batch and index_png_batch_ex with far in_offsets: their rows
    are the CPU model's with every offset word moved, high words intact.  Then
    decode_png_batch, decode_png_pixels_batch and - for the Adam7 image among
    them - decode_png_batch_ex read the far files through those rows into a
    near buffer, which the calls pack themselves."""
    from tests import png_adam7_files as p7
    from tests import png_files as pf
    from tools.models import png_adam7 as m7
    from tools.models import png_model as pm
    from tools.models import png_pixels_model as px
    files = [pf.make(5, 3, 8, 2, seed=1), pf.make(33, 9, 4, 3, seed=2, trns=bytes(range(16))),
             pf.make(17, 5, 16, 0, seed=3), p7.make7(19, 11, 8, 2, seed=4),
             pf.make(64, 40, 8, 6, seed=5, idat=3), pf.make(1, 1, 1, 0, seed=6)]
    blobs = [f.data for f in files]
    b = Batch(torch, far, blobs, None, seed=51, out=False)
    n = 3 * b.n
    offs, mask48 = b.inp.column([o for o, _ in b.inp.spans]), (1 << 48) - 1

    def moved(row, shift):
        """a row of the near buffer `shift` bytes further on"""
        r = list(row)
        r[0] += shift
        if any(row[2:]):
            r[4] += shift
            for w in (6, 7):
                if r[w]:
                    r[w] = (r[w] & ~mask48) | ((r[w] & mask48) + shift)
        return r

    def index(call, model, **kw):
        idx = torch.full((8 * n + 8,), -1, dtype=torch.int64, device="cuda")
        per = torch.full((n + 1,), UNSET, dtype=torch.int32, device="cuda")
        call(b.d_in.t, b.in_off, b.in_n, idx, per, **kw)
        torch.cuda.synchronize()
        rows = idx.cpu().numpy().view(np.uint64).reshape(-1, 8)
        res = per.cpu().tolist()
        assert (rows[n] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and res[n] == UNSET
        near = [model(b.buf, o, s) for o, s in b.inp.spans]
        assert res[:n] == [w[0] for w in near] * 3
        want = [moved(w[1], b.inp.shifts[c]) for c in range(3) for w in near]
        got = [[int(x) for x in r] for r in rows[:n]]
        assert got == want
        return got, [w[1] for w in near] * 3

    def decode(call, rows, near, sel, model, room, **kw):
        at = [0]
        for k in sel:
            at.append(at[-1] + room(near[k]))
        out = torch.full((at[-1] + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
        per = torch.full((len(sel) + 1,), UNSET, dtype=torch.int32, device="cuda")
        got = call(b.d_in.t, rows, sel, out, per, in_nbytes=b.inp.end, out_avail=at[-1], **kw)
        torch.cuda.synchronize()
        assert got.tolist() == at
        want = [model(b.buf, near[k]) for k in sel]
        assert per.cpu().tolist() == [SUCCESS] * len(sel) + [UNSET] == [w[0] for w in want] + [UNSET]
        assert out.cpu().numpy().tobytes() == b"".join(w[1] for w in want) + bytes([fb.CANARY]) * 64

    rows, near = index(dec.index_png_batch, pm.index)
    assert [r[0] for r in near[:b.n]] == [o for o, _ in b.inp.spans] and pm.is_zero(near[3])
    plain = [k for k in range(n) if k % b.n != 3]
    sel = plain[::-1] + plain[:2]
    decode(dec.decode_png_batch, rows, near, sel, pm.decode,
           lambda r: (r[2] >> 32) * pm.row_rowbytes(r))
    decode(dec.decode_png_pixels_batch, rows, near, sel,
           lambda buf, r: px.decode(buf, r, api.binding.PNG_RGBA),
           lambda r: px.out_bytes(r, api.binding.PNG_RGBA), fmt=api.binding.PNG_RGBA)
    rows7, near7 = index(dec.index_png_batch_ex,
                         lambda buf, o, s: m7.index(buf, o, s, m7.ADAM7), flags=m7.ADAM7)
    assert near7[3][3] >> 16 & 1 and files[3].pixels
    sel7 = [3 + 2 * b.n, 0, 3, 3 + b.n, 4 + b.n]
    decode(dec.decode_png_batch_ex, rows7, near7, sel7,
           lambda buf, r: m7.decode(buf, r, 0, 0),
           lambda r: m7.out_sizes([r], [0])[1], fmt=0, flags=m7.ADAM7)
    want7 = m7.decode(b.buf, near7[3], 0, 0)
    assert want7 == (SUCCESS, files[3].pixels)


# ---- PNG writing ----

def test_encode_png_batch(torch, far, api):
    """pixels, PLTE and tRNS data at far offsets; the files come out packed,
    and the CPU model reads every one back to its pixels"""
    from tests import png_files as pf
    from tools.models import png_model as pm
    images = [(5, 3, 8, 2, None, None), (33, 9, 4, 3, pf.palette(16), bytes(range(16))),
              (17, 5, 16, 0, None, None), (64, 40, 8, 6, None, None), (1, 1, 1, 0, None, None)]
    blobs, kinds = [], []
    for k, (w, h, d, c, plte, trns) in enumerate(images):
        blobs.append(pf.pixels_random(w, h, d, c, 60 + k))
        kinds.append(("pixels", k))
        for word, data in ((6, plte), (7, trns)):
            if data is not None:
                blobs.append(data)
                kinds.append((word, k))
    b = Batch(torch, far, blobs, None, seed=61, out=False)
    rows = []
    for cp in range(3):
        for k, (w, h, d, c, plte, trns) in enumerate(images):
            at = {kind: b.inp.at(cp, b.inp.spans[i][0]) for i, (kind, j) in enumerate(kinds) if j == k}
            rows.append([at["pixels"], len(blobs[kinds.index(("pixels", k))]), w | h << 32, d | c << 8,
                         0, 0, at[6] | (len(plte) // 3) << 48 if plte else 0,
                         at[7] | len(trns) << 48 if trns else 0])
    n = len(rows)
    c = api.Compressor(6)
    try:
        bound = c.png_encode_bound(rows)
        out = torch.full((bound + 64,), fb.CANARY, dtype=torch.uint8, device="cuda")
        res = torch.full((api.binding.PNGW_RESULT_WORDS + 1,), UNSET, dtype=torch.int64, device="cuda")
        idx = torch.full((8 * n + 1,), UNSET, dtype=torch.int64, device="cuda")
        c.encode_png_batch(rows, b.d_in.t, out, res, idx, in_avail=b.inp.end, out_avail=bound)
        torch.cuda.synchronize()
    finally:
        c.close()
    words, host = res.cpu().tolist(), out.cpu().numpy()
    pixels = sum(len(blobs[kinds.index(("pixels", k))]) for k in range(len(images)))
    assert words == [SUCCESS, words[1], 3 * pixels, n, UNSET] and 0 < words[1] <= bound
    assert not (host[words[1]:] != fb.CANARY).any(), "bytes written behind the files"
    index = idx.cpu().numpy()
    assert index[8 * n] == UNSET
    index = index[:8 * n].view(np.uint64).reshape(n, 8)
    files, at = host[:words[1]].tobytes(), 0
    for k, r in enumerate(index):
        off, size = int(r[0]), int(r[1])
        assert off == at and off + size <= words[1], k
        at += size
        code, row = pm.index(files, off, size)
        assert code == SUCCESS and row == [int(x) for x in r], k
        assert pm.decode(files, row) == (SUCCESS, blobs[kinds.index(("pixels", k % len(images)))]), k
    assert at == words[1]
