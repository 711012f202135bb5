"""ONE large stream from device memory to device memory on many waves:
libdeflate_amd_decompress_large (csrc/host_stream.hip with a device pointer as
its input source, csrc/stream_probe_kernels.hip).  Streams compressed by the
real reference (zlib where oracle/_ref did not travel); every result,
actual_in / actual_out and byte against the oracle, and
libdeflate_amd_stream_stats() says which path answered.

Inputs sit at byte offset 3 of their tensor with three junk bytes behind the
stream; outputs sit at an odd offset between two 64-byte canaries that must be
unchanged afterwards."""
import struct
import zlib

import numpy as np
import pytest

from libdeflate_amd import binding
from tests import datagen, oracle_util, streams

pytestmark = pytest.mark.gpu
CANARY = bytes(range(0x80, 0xC0))
OUT_AT = 1 + len(CANARY)        # odd


@pytest.fixture(scope="module")
def dec():
    from libdeflate_amd import api
    d = api.Decompressor()
    yield d
    d.close()


@pytest.fixture(scope="module")
def comp():
    ref = oracle_util.load_ref()
    if ref is not None:
        return lambda fmt, lvl, d: ref.compress(fmt, lvl, d)
    return lambda fmt, lvl, d: streams._zcompress(fmt, min(lvl, 9), d)


def _data(kind, n, seed):
    if kind == "text":
        return datagen.text_chunk(n, seed)
    return b"".join(datagen.chunk(i, 65536, seed) for i in range((n + 65535) // 65536))[:n]


def _upload(s, extra=b"\xee\xdd\xcc"):
    """-> (tensor, view of the stream at byte offset 3)"""
    import torch
    host = np.frombuffer(b"\xaa\xbb\xcc" + bytes(s) + extra, dtype=np.uint8).copy()
    t = torch.from_numpy(host).cuda()
    return t, t[3:3 + len(s)]


def _out_tensor(avail):
    import torch
    host = np.full(OUT_AT + avail + len(CANARY), 0x5A, dtype=np.uint8)
    host[1:OUT_AT] = np.frombuffer(CANARY, dtype=np.uint8)
    host[OUT_AT + avail:] = np.frombuffer(CANARY, dtype=np.uint8)
    return torch.from_numpy(host).cuda()


def large(dec, fmt, s, avail, want=True, stream=None, in_view=None, in_nbytes=None, out=None):
    """-> (result, actual_in, actual_out, bytes) like api.decompress_ex, from
    and to device memory; the canaries around the output are checked."""
    if in_view is None:
        _keep, in_view = _upload(s)
    if out is None:
        out = _out_tensor(avail)
    r, ain, aout = dec.decompress_large(fmt, in_view, out[OUT_AT:OUT_AT + avail],
                                        in_nbytes=len(s) if in_nbytes is None else in_nbytes,
                                        out_avail=avail, want_actual_out=want, stream=stream)
    host = out.cpu().numpy().tobytes()
    assert host[1:OUT_AT] == CANARY, "bytes in front of d_out were written"
    assert host[OUT_AT + avail:] == CANARY, "bytes at or past d_out + out_nbytes_avail were written"
    nout = aout if want else avail
    return r, ain, aout, host[OUT_AT:OUT_AT + nout]


def against_oracle(dec, oracle, fmt, s, avail, want, tag):
    got = large(dec, fmt, s, avail, want)
    st = binding.stream_stats()
    exp = oracle.decompress_ex(fmt, s, avail, want)
    assert got[0] == exp[0], (tag, fmt, want, got[:3], exp[:3], st)
    if exp[0] == 0:
        assert got[1] == exp[1] and got[3] == exp[3], (tag, fmt, want, st)
        if want:
            assert got[2] == exp[2], (tag, fmt, st)
    return got, st


@pytest.mark.parametrize("mib", [1, 4])
@pytest.mark.parametrize("kind", ["text", "mix"])
@pytest.mark.parametrize("level", [1, 6, 12])
def test_round_trips(dec, comp, oracle, mib, level, kind):
    n = mib << 20
    data = _data(kind, n, 0x61000 + mib + level)
    fmt = ("gzip", "zlib", "deflate")[(mib + level + len(kind)) % 3]
    z = comp(fmt, level, data)
    got, st = against_oracle(dec, oracle, fmt, z, n, True, "round trip")
    assert got == (0, len(z), n, data), (got[:3], st)
    assert st["parallel"] == 1 and st["bytes"] == n, st
    # exact fill (actual_out_nbytes_ret = NULL), with the trailing bytes as input
    keep, view = _upload(z)
    r2 = large(dec, fmt, z, n, False, in_view=view, in_nbytes=len(z) + 3)
    assert (r2[0], r2[1], r2[3]) == (0, len(z), data)
    assert binding.stream_stats()["parallel"] == 1
    # the host call on the same stream: the same four values
    h = dec.decompress_ex(fmt, z, n)
    assert h == got
    print(f"{mib} MiB {kind} L{level} {fmt}: {st}")


@pytest.mark.parametrize("fmt", ["deflate", "gzip", "zlib"])
def test_result_codes_of_damaged_large_streams(dec, comp, oracle, fmt):
    n = 3 << 20
    data = _data("mix", n, 0x52000)
    z = comp(fmt, 6, data)
    rng = np.random.default_rng(7)
    variants = [("ok", z, n), ("short", z, n + 1), ("nospace", z, n - 1),
                ("trunc1", z[:len(z) // 3], n), ("trunc2", z[:-9], n),
                ("trunc3", z[:-1], n)]
    for k in range(6):
        b = bytearray(z)
        pos = int(rng.integers(0, len(b)))
        b[pos] ^= 1 << int(rng.integers(0, 8))
        variants.append((f"flip{k}@{pos}", bytes(b), n))
    b = bytearray(z)
    b[-5] ^= 0x40       # footer (or, raw: the stream's last bytes)
    variants.append(("footer", bytes(b), n))
    for name, s, avail in variants:
        for want in (True, False):
            against_oracle(dec, oracle, fmt, s, avail, want, name)


def test_small_shapes_everything_through_the_stream_path(dec, oracle, comp, monkeypatch):
    """Every stream, however small, through the many-wave path with 4 KiB
    chunks, from device memory: the oracle's answer for each, and at least an
    eighth of them answered by the many-wave path."""
    monkeypatch.setenv("LDA_STREAM_PAR_MIN", "0")
    monkeypatch.setenv("LDA_STREAM_CHUNK", "4096")
    binding.reload_env()
    cases = streams.random_cases(31, 120, compress=comp,
                                 sizes=[0, 1, 5, 100, 1000, 5000, 20000, 70000, 300000])
    cases += [(f, s, a, w, t) for f, s, a, w, t in streams.garbage_cases(32, 60)]
    for s, want in streams.stored_then_match_streams():
        cases.append(("deflate", s, len(want), True, "stored_then_match"))
    for name, s, want in streams.parallel_round_streams():
        cases.append(("deflate", s, len(want), True, name))
    for s in (streams.empty_static_blocks(), streams.empty_dynamic_blocks()):
        cases.append(("deflate", s, 10000, True, "slow"))
    npar = 0
    for fmt, s, avail, want, tag in cases:
        _got, st = against_oracle(dec, oracle, fmt, s, avail, want, tag)
        npar += st["parallel"]
    print(f"{npar} of {len(cases)} cases were answered by the many-wave path")
    assert npar >= len(cases) // 8


def test_stored_blocks(dec, oracle):
    """Runs of stored blocks are walked over the rows of
    lda_stream_find_stored_kernel (stats slot 15: chunks made that way)."""
    rnd = datagen.random_chunk(2 << 20, 5)
    stored = streams._zcompress("deflate", 0, rnd)
    got, st = against_oracle(dec, oracle, "deflate", stored, len(rnd), True, "level 0")
    print("stored-only:", st)
    assert got == (0, len(stored), len(rnd), rnd)
    assert st["parallel"] == 1 and st["host_chunks"] >= 32 and st["chunks_decoded"] >= 32, st
    # truncated inside a block; the third block's NLEN no longer matches
    h3 = 0
    for _ in range(2):
        h3 += 5 + (stored[h3 + 1] | stored[h3 + 2] << 8)
    for bad in (stored[:len(stored) - 70000],
                stored[:h3 + 3] + bytes([stored[h3 + 3] ^ 0x40]) + stored[h3 + 4:]):
        got, st = against_oracle(dec, oracle, "deflate", bad, len(rnd), True, "damaged level 0")
        assert got[0] != 0
    # stored blocks between Huffman blocks (zlib's full flushes leave empty ones)
    txt = datagen.text_chunk(1 << 20, 9)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    mixed = b""
    for i in range(24):
        mixed += co.compress(txt[i * 40000:(i + 1) * 40000]) + co.flush(zlib.Z_FULL_FLUSH)
    mixed += co.flush()
    got, st = against_oracle(dec, oracle, "deflate", mixed, 24 * 40000, True, "full flushes")
    assert got == (0, len(mixed), 24 * 40000, txt[:24 * 40000]), st
    assert st["parallel"] == 1, st
    # a payload in which every fourth offset looks like LEN / NLEN: more rows
    # than the queue holds; right whichever path answers
    pat = b"\x00\x00\xff\xff" * (1 << 18)
    z = streams._zcompress("gzip", 0, pat)
    got, st = against_oracle(dec, oracle, "gzip", z, len(pat), True, "00 00 FF FF")
    print("00 00 FF FF payload:", st)
    assert got == (0, len(z), len(pat), pat), st


def test_stored_run_into_the_footer(dec, oracle, monkeypatch):
    """tests/test_stream_gpu.py::test_stored_run_into_the_footer from device
    memory: a 32 KiB window that ends t bytes into the gzip footer, a final
    stored block whose LEN reaches `over` bytes into it."""
    monkeypatch.setenv("LDA_STREAM_WINDOW", "32768")
    monkeypatch.setenv("LDA_STREAM_PAR_MIN", "0")
    binding.reload_env()
    rng = np.random.default_rng(0xF007)
    for t in range(1, 8):
        for over in (0, 1, t, 8):
            raw_len = 32768 - t
            payload, raw = bytearray(), bytearray()
            while raw_len - len(raw) > 5 + 1000:
                blk = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
                raw += b"\x00" + struct.pack("<HH", 1000, 1000 ^ 0xFFFF) + blk
                payload += blk
            k = raw_len - len(raw) - 5
            blk = rng.integers(0, 256, k, dtype=np.uint8).tobytes()
            raw += b"\x01" + struct.pack("<HH", k + over, (k + over) ^ 0xFFFF) + blk
            payload += blk
            assert len(raw) == raw_len
            z = (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + bytes(raw) +
                 struct.pack("<II", zlib.crc32(bytes(payload)), len(payload)))
            got, st = against_oracle(dec, oracle, "gzip", z, len(payload) + 64, True, (t, over))
            if over == 0:
                assert got == (0, len(z), len(payload), bytes(payload)), (t, st)


def test_blocks_of_one_codeword_length(dec, comp, oracle):
    """Dynamic blocks over incompressible bytes: the host has no header to
    read, lda_stream_hdr_class_kernel classifies the parsed ones.  Without it
    the chain of a Huffman-only stream needs more repairs than it has chunks."""
    rng = np.random.default_rng(0x1E6)
    txt = datagen.text_chunk(3 << 20, 41)
    parts = []
    for i in range(12):
        parts.append(txt[i * 200000:(i + 1) * 200000])
        parts.append(rng.integers(0, 256, 70000, dtype=np.uint8).tobytes())
    mixed = b"".join(parts)
    z = comp("gzip", 6, mixed)
    got, st = against_oracle(dec, oracle, "gzip", z, len(mixed), True, "text and noise")
    print("text and incompressible bytes:", st)
    assert got == (0, len(z), len(mixed), mixed), (got[:3], st)
    assert st["parallel"] == 1, st
    for nv in (256, 250, 64):
        raw = rng.integers(0, nv, 3 << 20, dtype=np.uint8).tobytes()
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        h = co.compress(raw) + co.flush()
        got, st = against_oracle(dec, oracle, "deflate", h, len(raw), True, f"huffman {nv}")
        print(f"Huffman-only, {nv} values:", st)
        assert got == (0, len(h), len(raw), raw), (nv, got[:3], st)
        assert st["parallel"] == 1, st
        assert st["repairs"] <= st["chunks_decoded"], st
        bad = h[:len(h) // 2] + bytes([h[len(h) // 2] ^ 0x10]) + h[len(h) // 2 + 1:]
        against_oracle(dec, oracle, "deflate", bad, len(raw), True, f"damaged huffman {nv}")


@pytest.mark.parametrize("win", ["32768", "65536", "262144"])
def test_input_windows(dec, comp, oracle, monkeypatch, win):
    data = _data("mix", 3 << 20, 0x53000)
    monkeypatch.setenv("LDA_STREAM_WINDOW", win)
    monkeypatch.setenv("LDA_STREAM_PAR_MIN", "0")
    binding.reload_env()
    for fmt, lvl in (("gzip", 6), ("deflate", 1), ("zlib", 12), ("deflate", 0)):
        z = comp(fmt, lvl, data)
        got, st = against_oracle(dec, oracle, fmt, z, len(data), True, (win, fmt, lvl))
        assert got == (0, len(z), len(data), data), (win, fmt, lvl, got[:3], st)
        assert st["parallel"] == 1, (win, fmt, lvl, st)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    txt = data[:500000]
    z = co.compress(txt) + co.flush()
    got, st = against_oracle(dec, oracle, "deflate", z, len(txt), True, "Z_FIXED")
    assert got == (0, len(z), len(txt), txt), st
    z = comp("gzip", 6, data)
    for cut in (len(z) // 2, len(z) - 9):
        against_oracle(dec, oracle, "gzip", z[:cut], len(data), True, ("cut", cut))


def test_members_and_small_streams(dec, comp, oracle, monkeypatch):
    a = datagen.text_chunk(1 << 20, 0x64001)
    b = _data("mix", (1 << 20) + 12345, 0x64002)
    za, zb = comp("gzip", 6, a), comp("gzip", 6, b)
    keep, view = _upload(za + zb)
    r = large(dec, "gzip", za + zb, len(a) + 100, True, in_view=view)
    assert r == (0, len(za), len(a), a), (r[:3], binding.stream_stats())
    assert binding.stream_stats()["parallel"] == 1
    r = large(dec, "gzip", zb, len(b), True, in_view=view[r[1]:], in_nbytes=len(zb))
    assert r == (0, len(zb), len(b), b), (r[:3], binding.stream_stats())
    assert binding.stream_stats()["parallel"] == 1
    # a small stream stays on one wave; so does everything under the switch
    small = datagen.text_chunk(1000, 3)
    z = comp("zlib", 6, small)
    got, st = against_oracle(dec, oracle, "zlib", z, 1000, True, "small")
    assert got == (0, len(z), 1000, small) and st["parallel"] == 0, st
    monkeypatch.setenv("LDA_NO_STREAM_PAR", "1")
    binding.reload_env()
    got, st = against_oracle(dec, oracle, "gzip", za, len(a), True, "switched off")
    assert got == (0, len(za), len(a), a) and st["parallel"] == 0, st


def test_stream_order(dec, comp):
    """d_in is produced by a copy queued on a non-default stream; the call gets
    that stream and nothing synchronises in between."""
    import torch
    data = datagen.text_chunk(2 << 20, 0x65001)
    z = comp("gzip", 6, data)
    keep, staged = _upload(z)
    ballast = torch.zeros(256 << 20, dtype=torch.uint8, device="cuda")
    sink = torch.empty_like(ballast)
    t_in = torch.full((len(z) + 6,), 0x33, dtype=torch.uint8, device="cuda")
    out = _out_tensor(len(data))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(32):     # (something for the copy to queue up behind)
            sink.copy_(ballast, non_blocking=True)
        t_in[3:3 + len(z)].copy_(staged, non_blocking=True)
    r = large(dec, "gzip", z, len(data), True, stream=s, in_view=t_in[3:3 + len(z)], out=out)
    st = binding.stream_stats()
    assert r == (0, len(z), len(data), data), (r[:3], st)
    assert st["parallel"] == 1, st
