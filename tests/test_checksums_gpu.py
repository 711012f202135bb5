"""Batched CRC-32 / Adler-32 on the GPU vs the oracle (and zlib as the second
independent control, as programs/test_checksums.c:111-196 does)."""
import zlib

import numpy as np
import pytest

from tests import datagen

pytestmark = pytest.mark.gpu


def _device_batch(chunks, align_pad=0):
    import torch
    offs, sizes, blob = [], [], bytearray()
    for c in chunks:
        blob += bytes(align_pad)
        offs.append(len(blob))
        sizes.append(len(c))
        blob += c
    blob += bytes(64)
    data = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    return (data, torch.tensor(offs, dtype=torch.int64).cuda(),
            torch.tensor(sizes, dtype=torch.int64).cuda())


@pytest.mark.parametrize("kind", ["crc32", "adler32"])
def test_batch_matches_oracle(kind, oracle):
    import torch
    from libdeflate_amd import api
    rng = np.random.default_rng(7)
    sizes = [0, 1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4096, 5552,
             5553, 65535, 65536, 65537, 200000]
    chunks = [datagen.chunk(i, n, 0x0E110000) for i, n in enumerate(sizes)]
    chunks.append(b"\xff" * 5553)
    for pad in (0, 1, 7, 13):
        data, offs, nb = _device_batch(chunks, pad)
        inits = rng.integers(0, 2**32, size=len(chunks), dtype=np.uint32)
        if kind == "adler32":
            lo = rng.integers(0, 65521, size=len(chunks))
            hi = rng.integers(0, 65521, size=len(chunks))
            inits = ((hi << 16) | lo).astype(np.uint32)
            inits[-1] = (65520 << 16) | 65520   # test_checksums.c:184-196
        init_t = torch.from_numpy(inits.view(np.int32)).cuda()
        out = torch.zeros(len(chunks), dtype=torch.int32, device="cuda")
        for init in (None, init_t):
            api.checksum_batch(kind, data, offs, nb, out, init=init)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            for i, c in enumerate(chunks):
                iv = int(inits[i]) if init is not None else (0 if kind == "crc32" else 1)
                want = getattr(oracle, kind)(c, iv)
                assert got[i] == want, (kind, pad, i, len(c))
                z = zlib.crc32(c, iv) if kind == "crc32" else zlib.adler32(c, iv)
                assert want == z


def test_single_buffer_api(oracle):
    from libdeflate_amd import api, binding
    lib = binding.load()
    # NULL-buffer rules, lib/crc32.c:259-260, lib/adler32.c:159-160
    assert lib.libdeflate_crc32(1234, None, 1234) == 0
    assert lib.libdeflate_adler32(1234, None, 0) == 1
    data = datagen.text_chunk(100000, 3)
    assert api.crc32(data) == oracle.crc32(data)
    assert api.adler32(data) == oracle.adler32(data)
    # chaining: f(f(v,A),B) == f(v,A||B)  (test_checksums.c:73-84)
    a, b = data[:33333], data[33333:]
    assert api.crc32(b, api.crc32(a)) == api.crc32(data)
    assert api.adler32(b, api.adler32(a)) == api.adler32(data)
    assert api.crc32(b"") == 0 and api.adler32(b"") == 1


SEG = 1 << 24    # ADLER_SEG: the Adler-32 kernel's segment of one chunk


def test_batch_above_one_segment():
    """chunks of 2^24 - 1, 2^24, 2^24 + 1 and 2^25 + 17 bytes (the Adler-32
    kernel's multi-segment update s2 += n*s1 + W): all 0xFF and random bytes,
    the default and the largest initial value, offsets 0 and 13"""
    import torch
    from libdeflate_amd import api
    rng = np.random.default_rng(0x0E110A32)
    rnd = rng.integers(0, 256, size=2 * SEG + 17, dtype=np.uint8).tobytes()
    sizes = [SEG - 1, SEG, SEG + 1, 2 * SEG + 17]
    for pad in (0, 13):
        for fill in ("ff", "random"):
            chunks = [b"\xff" * n if fill == "ff" else rnd[:n] for n in sizes]
            data, offs, nb = _device_batch(chunks, pad)
            out = torch.zeros(len(chunks), dtype=torch.int32, device="cuda")
            for kind, inits in (("adler32", (1, (65520 << 16) | 65520)),
                                ("crc32", (0, 0xFFFFFFFF))):
                for iv in inits:
                    init = torch.from_numpy(
                        np.full(len(chunks), iv, dtype=np.uint32).view(np.int32)).cuda()
                    api.checksum_batch(kind, data, offs, nb, out, init=init)
                    torch.cuda.synchronize()
                    got = out.cpu().numpy().view(np.uint32)
                    for i, c in enumerate(chunks):
                        z = zlib.adler32(c, iv) if kind == "adler32" else zlib.crc32(c, iv)
                        assert got[i] == z, (kind, fill, pad, len(c), hex(iv))
            del data


def test_single_buffer_above_one_segment():
    """libdeflate_adler32 / libdeflate_crc32 on 40 MiB, and chained over a
    split that leaves both sides longer than one segment"""
    from libdeflate_amd import api
    rng = np.random.default_rng(0x0E110A33)
    data = rng.integers(0, 256, size=40 << 20, dtype=np.uint8).tobytes()
    assert api.adler32(data) == zlib.adler32(data)
    assert api.crc32(data) == zlib.crc32(data)
    cut = SEG + 4097
    a, b = data[:cut], data[cut:]
    assert api.adler32(b, api.adler32(a)) == zlib.adler32(data)
    assert api.crc32(b, api.crc32(a)) == zlib.crc32(data)
    ff = b"\xff" * (2 * SEG + 17)
    assert api.adler32(ff, (65520 << 16) | 65520) == zlib.adler32(ff, (65520 << 16) | 65520)


def test_zlib_footer_above_one_segment():
    """a zlib stream of 2^24 + 4097 bytes of output as a batch of one: its
    footer is checked with the whole output's Adler-32 in one chunk; a
    wrong footer is refused"""
    from libdeflate_amd import api
    n = SEG + 4097
    raw = datagen.text_chunk(n, 0x0E110A34)
    z = zlib.compress(raw, 1)
    d = api.Decompressor()
    try:
        r = d.decompress_batch_host("zlib", [z], [n])[0]
        assert r[0] == 0 and r[1] == len(z) and r[2] == n and r[3] == raw
        for at in (-1, -3):
            b = bytearray(z)
            b[at] ^= 0x01
            assert d.decompress_batch_host("zlib", [bytes(b)], [n])[0][0] == 1
    finally:
        d.close()
