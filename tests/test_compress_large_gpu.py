"""libdeflate_amd_compress_large_batch: ONE raw DEFLATE / zlib / gzip stream
from one device buffer, enqueue only.  Every case checks (a) the device bytes
and size against what the single-buffer host call of the same object returns -
the call's defining property -, and, on zlib so that a mistake shared with the
host form still shows, (b) the round trip and (c) the footer."""
import zlib

import pytest

from tests import datagen

pytestmark = pytest.mark.gpu
WBITS = {"deflate": -15, "zlib": 15, "gzip": 31}
FORMATS = ("deflate", "zlib", "gzip")
CANARY = 64
_PARTS = []


def _mix(n, shift=0):
    """n bytes of the datagen mix: 64 KiB chunks of rotating kinds (16 distinct
    ones, repeated 1 MiB apart - beyond any window)"""
    if not _PARTS:
        kinds = [0, 5, 6, 7, 1]
        _PARTS.extend(datagen.chunk(kinds[k % 5], 65536, 0x0E110C00 + k) for k in range(16))
    return b"".join(_PARTS[(k + shift) % 16] for k in range((n + 65535) // 65536))[:n]


def _device(c, fmt, d, out_avail=None, in_shift=0, out_shift=0):
    """-> (size the device reported, the out_avail bytes of the output, the
    canary bytes behind them), synchronised"""
    import numpy as np
    import torch
    if out_avail is None:
        out_avail = c.bound(fmt, len(d))
    data = torch.zeros(in_shift + len(d) + 16, dtype=torch.uint8, device="cuda")
    data[in_shift:in_shift + len(d)] = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy())
    out = torch.full((out_shift + out_avail + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    c.compress_large_batch(fmt, data[in_shift:], out[out_shift:], size, in_nbytes=len(d),
                           out_avail=out_avail)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return int(size[0]), o[out_shift:out_shift + out_avail].tobytes(), \
        o[out_shift + out_avail:].tobytes()


def _check(c, fmt, d, tag, **kw):
    want = c.compress(fmt, d)
    assert want is not None, tag
    size, got, canary = _device(c, fmt, d, **kw)
    # (a) the host call's bytes
    assert size == len(want), (tag, size, len(want))
    assert got[:size] == want, (tag, "bytes differ from the host call's")
    assert canary == b"\xA5" * CANARY, tag
    z = got[:size]
    # (b) zlib reads it
    assert zlib.decompress(z, WBITS[fmt]) == d, (tag, "zlib round trip")
    # (c) the footer is the whole buffer's
    if fmt == "gzip":
        assert z[:4] == b"\x1f\x8b\x08\x00" and z[9] == 0xFF, tag
        assert int.from_bytes(z[-8:-4], "little") == zlib.crc32(d), (tag, "CRC-32")
        assert int.from_bytes(z[-4:], "little") == len(d) % (1 << 32), (tag, "ISIZE")
    if fmt == "zlib":
        assert int.from_bytes(z[-4:], "big") == zlib.adler32(d), (tag, "Adler-32")
    return z


# 131071: the last single-chunk size; 131072: 8 segments of 16 KiB; 131073: a
# last piece of one byte; 4194305: S becomes 32 KiB; 8388609: S becomes 64 KiB
SEAMS = [0, 1, 131071, 131072, 131073, 200000, 4194305, 8388609]


@pytest.mark.parametrize("level", [1, 6, 12])
@pytest.mark.parametrize("n", SEAMS)
def test_sizes_at_the_seams(n, level):
    from libdeflate_amd import api
    c = api.Compressor(level)
    d = _mix(n)
    for fmt in FORMATS:
        _check(c, fmt, d, (n, level, fmt))
    c.close()


@pytest.mark.parametrize("n", [131073, 1 << 20])
def test_level_0_is_one_chunk(n):
    from libdeflate_amd import api
    c = api.Compressor(0)
    d = _mix(n, 3)
    for fmt in FORMATS:
        z = _check(c, fmt, d, (n, 0, fmt))
        assert len(z) > n       # stored
    c.close()


@pytest.mark.parametrize("fmt", ["gzip", "zlib"])
def test_more_segments_than_one_scan_block(fmt, monkeypatch):
    """2050 segments of 8 KiB: the offsets of the last ones are a local prefix
    plus the first scan block's total, and every thread of the checksum
    combine has a run of more than one piece (CRC-32 and Adler-32)"""
    from libdeflate_amd import api, binding
    monkeypatch.setenv("LDA_SEG_BYTES", "8192")
    binding.reload_env()
    n = 2049 * 8192 + 5
    c = api.Compressor(1)
    _check(c, fmt, _mix(n, 1), ("2050 segments", fmt))
    c.close()


@pytest.mark.parametrize("n", [200000, 100000])
def test_does_not_fit(n):
    """one byte too little: size 0 and nothing behind out_avail touched, for
    segments and for one chunk"""
    from libdeflate_amd import api
    c = api.Compressor(6)
    d = _mix(n, 2)
    for fmt in FORMATS:
        want = c.compress(fmt, d)
        size, _, canary = _device(c, fmt, d, out_avail=len(want) - 1)
        assert size == 0, (n, fmt)
        assert canary == b"\xA5" * CANARY, (n, fmt)
        assert c.compress(fmt, d, out_avail=len(want) - 1) is None
        # and exactly enough is enough
        size, got, canary = _device(c, fmt, d, out_avail=len(want))
        assert size == len(want) and got == want and canary == b"\xA5" * CANARY, (n, fmt)
    c.close()


def test_unaligned_pointers():
    """input at 3 and output at 1 modulo 16; the header moves the payload by
    0, 2 or 10 bytes more"""
    from libdeflate_amd import api
    c = api.Compressor(6)
    d = _mix(200000, 4)
    for fmt in FORMATS:
        _check(c, fmt, d, ("unaligned", fmt), in_shift=3, out_shift=1)
    c.close()


def test_two_calls_back_to_back():
    """queued on one object with nothing between them, the second one larger
    (the scratch grows); both right after one synchronise"""
    import numpy as np
    import torch
    from libdeflate_amd import api
    c, h = api.Compressor(6), api.Compressor(6)
    ds = [_mix(200000, 5), _mix(4194305, 6)]
    outs, sizes = [], []
    datas = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for d in ds]
    torch.cuda.synchronize()
    for d, t in zip(ds, datas):
        outs.append(torch.zeros(c.bound("gzip", len(d)), dtype=torch.uint8, device="cuda"))
        sizes.append(torch.zeros(1, dtype=torch.int64, device="cuda"))
        c.compress_large_batch("gzip", t, outs[-1], sizes[-1])
    torch.cuda.synchronize()
    for d, o, s in zip(ds, outs, sizes):
        want = h.compress("gzip", d)
        z = o.cpu().numpy()[:int(s[0])].tobytes()
        assert z == want, len(d)
        assert zlib.decompress(z, 31) == d
        assert int.from_bytes(z[-8:-4], "little") == zlib.crc32(d)
    c.close()
    h.close()


def test_zeros_across_many_segments():
    """lengths and distances at their limits across the primed tiles"""
    from libdeflate_amd import api
    c = api.Compressor(6)
    _check(c, "gzip", bytes(5 * 65536 + 17), ("zeros",))
    c.close()
