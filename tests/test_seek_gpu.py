"""The seek index over ONE plain DEFLATE / zlib / gzip stream in device memory
and the ranged reads through it: libdeflate_amd_decompress_large_index and
libdeflate_amd_seek_read_batch (csrc/host_seek.hip, seek_plan.h,
seek_kernels.hip, lda_seek_decode_kernel of inflate_stream.hip).  Streams
compressed by the real reference (zlib where oracle/_ref did not travel);
expected bytes are slices of the plain data.

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
WIN = binding.SEEK_WINDOW
MAGIC, END = 0x314B45455341444C, 0x21444E454B454553
BAD_DATA = 1


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


def _canaries(host, avail):
    assert host[1:OUT_AT] == CANARY, "bytes in front of d_out were written"
    assert host[OUT_AT + avail:] == CANARY, "bytes at or past d_out + out_avail were written"


class Indexed:
    """a stream on the device with its index, windows and plain bytes"""

    def __init__(self, dec, fmt, z, data, spacing=65536, max_points=None, avail=None):
        self.fmt, self.z, self.data, self.spacing = fmt, z, data, spacing
        n = len(data)
        avail = n if avail is None else avail
        if max_points is None:
            max_points = n // spacing + 2
        self.keep, self.view = _upload(z)
        out = _out_tensor(avail)
        self.result, self.ain, self.aout, self.rows, self.windows = dec.decompress_large_index(
            fmt, self.view, out[OUT_AT:OUT_AT + avail], spacing, max_points,
            in_nbytes=len(z), out_avail=avail)
        self.stats = binding.stream_stats()
        host = out.cpu().numpy().tobytes()
        _canaries(host, avail)
        self.out = host[OUT_AT:OUT_AT + self.aout]
        if self.result == 0:
            self.npts = len(self.rows) - 2
            self.offs = [int(v) for v in self.rows[1:-1, 0]]

    def check_rows(self, raw_off=None):
        """the invariants of the rows, and every window against the data"""
        rows, n = self.rows, len(self.data)
        assert self.result == 0 and (self.ain, self.aout, self.out) == (len(self.z), n, self.data)
        assert rows.dtype == np.uint64 and rows.shape == (self.npts + 2, 4)
        assert int(rows[0, 0]) == MAGIC and int(rows[0, 1]) == binding.FORMATS[self.fmt]
        assert int(rows[0, 3]) == self.npts >= 1
        assert [int(v) for v in rows[1]] == [0, 0, 0, 0], "point 0: the first bit at offset 0"
        pts = rows[1:-1].astype(object)
        for k in range(1, self.npts):
            assert pts[k][0] > pts[k - 1][0] and pts[k][1] > pts[k - 1][1], (k, pts[k - 1], pts[k])
            assert pts[k][0] - pts[k - 1][0] >= self.spacing, (k, pts[k - 1], pts[k])
            assert pts[k][3] in (0, 2) and pts[k][0] < n
        total, raw_n, ftr, end = (int(v) for v in rows[-1])
        assert total == n and end == END
        assert int(rows[0, 2]) + raw_n + ftr == len(self.z), "the closing row equals the totals"
        if raw_off is not None:
            assert int(rows[0, 2]) == raw_off
        assert self.windows.numel() == self.npts * WIN
        wins = self.windows.cpu().numpy().tobytes()
        for k, off in enumerate(self.offs):
            have = min(off, WIN)
            exp = bytes(WIN - have) + self.data[off - have:off]
            assert wins[k * WIN:(k + 1) * WIN] == exp, f"window {k} at {off}"


def read(dec, ix, ranges, rows=None, view=None, avail=None, stream=None, out=None):
    """-> (results, bytes of d_out[:sum]); the canaries are checked"""
    import torch
    ranges = np.array(ranges, dtype=np.uint64).reshape(-1, 2)
    need = int(ranges[:, 1].sum()) if len(ranges) else 0
    avail = need if avail is None else avail
    if out is None:
        out = _out_tensor(avail)
    res = torch.full((max(len(ranges), 1),), 77, dtype=torch.int32, device="cuda")
    dec.seek_read_batch(ix.view if view is None else view, ix.rows if rows is None else rows,
                        ix.windows, ranges, out[OUT_AT:OUT_AT + avail], res, stream=stream,
                        in_nbytes=len(ix.z), out_avail=avail)
    if stream is not None:
        stream.synchronize()
    host = out.cpu().numpy().tobytes()
    _canaries(host, avail)
    return res.cpu().numpy().tolist()[:len(ranges)], host[OUT_AT:OUT_AT + need]


def expected(data, ranges):
    return b"".join(data[a:a + n] for a, n in ranges)


def range_set(ix):
    """the ranges every index is read with, whatever points it holds"""
    n, offs = len(ix.data), ix.offs
    ends = offs + [n]
    rs = [(0, 0), (n, 0)]
    if n:
        rs += [(0, 1), (0, n), (n - 1, 1)]
    k = len(offs) // 2
    if ends[k + 1] - ends[k] > 2:                       # inside one interval
        rs.append((ends[k] + 1, min(ends[k + 1] - ends[k] - 2, 5000)))
    if len(offs) >= 2:
        rs.append((offs[k] - 1 if k else offs[1] - 1, 2))     # two bytes straddling a point
        j = max(k - 1, 0)
        rs.append((ends[j], ends[j + 1] - ends[j]))     # exactly point j to point j + 1
    if len(offs) >= 3:                                  # a span of three intervals
        j = min(k, len(offs) - 3)
        rs.append((ends[j] + 7, ends[j + 3] - 11 - (ends[j] + 7)))
    if n > 100:
        rs += [(n // 3, 99), (n // 3, 99)]              # the same range twice
    return rs


def read_and_check(dec, ix, tag):
    rs = range_set(ix)
    order = list(range(len(rs)))
    np.random.default_rng(len(rs) + len(ix.data)).shuffle(order)
    for ranges in (rs, [rs[i] for i in order]):
        res, got = read(dec, ix, ranges)
        assert res == [0] * len(ranges), (tag, res, ranges)
        exp = expected(ix.data, ranges)
        assert len(got) == len(exp) and got == exp, (tag, ranges)
    return rs


CASES = [(mib, kind, level) for mib in (1, 3) for kind in ("text", "mix") for level in (1, 6, 12)]
_built = {}


def built(dec, comp, mib, kind, level):
    """one index per case, shared by the tests that read through it"""
    key = (mib, kind, level)
    if key not in _built:
        n = mib << 20
        data = _data(kind, n, 0x5EE000 + mib + level)
        fmt = ("gzip", "zlib", "deflate")[(mib + level + len(kind)) % 3]
        z = comp(fmt, level, data)
        _built[key] = Indexed(dec, fmt, z, data)
    return _built[key]


@pytest.mark.parametrize("mib,kind,level", CASES)
def test_index_build(dec, comp, oracle, mib, kind, level):
    ix = built(dec, comp, mib, kind, level)
    n = len(ix.data)
    assert ix.stats["parallel"] == 1 and ix.stats["bytes"] == n, ix.stats
    ix.check_rows()
    assert ix.npts >= 2, ix.rows
    # the same answers as decompress_large and as the oracle
    out = _out_tensor(n)
    r = dec.decompress_large(ix.fmt, ix.view, out[OUT_AT:OUT_AT + n], in_nbytes=len(ix.z),
                             out_avail=n)
    host = out.cpu().numpy().tobytes()
    assert (ix.result, ix.ain, ix.aout) == r and host[OUT_AT:OUT_AT + n] == ix.out
    exp = oracle.decompress_ex(ix.fmt, ix.z, n, True)
    assert (ix.result, ix.ain, ix.aout, ix.out) == tuple(exp[:4])
    print(f"{mib} MiB {kind} L{level} {ix.fmt}: {ix.npts} points, "
          f"{ix.npts / mib:.1f} per MiB at spacing {ix.spacing}")


@pytest.mark.parametrize("mib,kind,level", CASES)
def test_reads(dec, comp, mib, kind, level):
    import torch
    ix = built(dec, comp, mib, kind, level)
    assert ix.result == 0
    rs = read_and_check(dec, ix, (mib, kind, level))
    # one byte of room less: refused, nothing written
    need = sum(n for _a, n in rs)
    out = _out_tensor(need)
    before = out.clone()
    with pytest.raises(RuntimeError, match="out_avail"):
        read(dec, ix, rs, avail=need - 1, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, before)


def _mixed_stream():
    """dynamic, static and stored blocks in one raw stream: parts of four
    compressors, each ended by a full flush (a byte boundary, no history kept)"""
    parts = [(6, zlib.Z_DEFAULT_STRATEGY, datagen.text_chunk(400000, 0x5EE101)),
             (6, zlib.Z_FIXED, datagen.text_chunk(300000, 0x5EE102)),
             (0, zlib.Z_DEFAULT_STRATEGY, datagen.random_chunk(200000, 0x5EE103)),
             (6, zlib.Z_FIXED, datagen.text_chunk(70000, 0x5EE104)),
             (9, zlib.Z_DEFAULT_STRATEGY, _data("mix", 400000, 0x5EE105))]
    z = b""
    for i, (lvl, strat, d) in enumerate(parts):
        co = zlib.compressobj(lvl, zlib.DEFLATED, -15, 9, strat)
        z += co.compress(d) + co.flush(zlib.Z_FINISH if i == len(parts) - 1 else zlib.Z_FULL_FLUSH)
    return z, b"".join(d for _l, _s, d in parts)


def test_block_kinds(dec, oracle):
    """Stored runs, static blocks, all kinds in one stream, a gzip header with
    a file name: read right whatever points the index holds."""
    rnd = datagen.random_chunk(2 << 20, 0x5EE200)
    txt = datagen.text_chunk(1 << 20, 0x5EE201)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    fixed = co.compress(txt) + co.flush()
    mixed, mixed_data = _mixed_stream()
    head = b"\x1f\x8b\x08\x08\x12\x34\x56\x78\x02\x03" + b"a-file-name.txt\x00"
    named = (head + streams._zcompress("deflate", 6, txt) +
             struct.pack("<II", zlib.crc32(txt), len(txt)))
    for tag, fmt, z, data, raw_off in (
            ("level 0", "deflate", streams._zcompress("deflate", 0, rnd), rnd, 0),
            ("Z_FIXED", "deflate", fixed, txt, 0),
            ("mixed", "deflate", mixed, mixed_data, 0),
            ("FNAME", "gzip", named, txt, len(head))):
        ix = Indexed(dec, fmt, z, data)
        exp = oracle.decompress_ex(fmt, z, len(data), True)
        assert (ix.result, ix.ain, ix.aout, ix.out) == tuple(exp[:4]), (tag, ix.stats)
        ix.check_rows(raw_off)
        print(f"{tag}: {ix.npts} points, {ix.stats}")
        if tag in ("level 0", "FNAME"):     # (a Z_FIXED stream may have one point)
            assert ix.stats["parallel"] == 1 and ix.npts >= 2, (tag, ix.stats)
        read_and_check(dec, ix, tag)
    # the small hand-built streams: static, stored, dynamic, static
    for z, data in streams.static_dynamic_static_streams():
        ix = Indexed(dec, "deflate", z, data, spacing=256, max_points=8)
        ix.check_rows(0)
        read_and_check(dec, ix, "static / dynamic / static")


def test_small_ends(dec, comp):
    small = datagen.text_chunk(1000, 3)
    ix = Indexed(dec, "zlib", comp("zlib", 6, small), small)
    assert ix.stats["parallel"] == 0 and ix.npts == 1, (ix.stats, ix.rows)
    ix.check_rows(2)
    read_and_check(dec, ix, "under LDA_STREAM_PAR_MIN")
    ix = Indexed(dec, "gzip", comp("gzip", 6, b"x"), b"x")
    assert ix.npts == 1
    ix.check_rows(10)
    read_and_check(dec, ix, "one byte")
    ix = Indexed(dec, "deflate", comp("deflate", 6, b""), b"", avail=16)
    assert ix.npts == 1
    ix.check_rows(0)
    rs = read_and_check(dec, ix, "empty")
    assert all(n == 0 for _a, n in rs)
    data = datagen.text_chunk(1 << 20, 0x5EE300)
    z = comp("gzip", 6, data)
    ix = Indexed(dec, "gzip", z, data, max_points=1)
    assert ix.stats["parallel"] == 1 and ix.npts == 1
    ix.check_rows()
    read_and_check(dec, ix, "capacity 1")
    # 16 points at this spacing, room for 3: the spacing was doubled (twice at
    # least: 262144 leaves 4), and the rows keep the doubled spacing
    ix = Indexed(dec, "gzip", z, data, max_points=3)
    assert 2 <= ix.npts <= 3, ix.rows
    ix.spacing = 4 * 65536
    ix.check_rows()
    read_and_check(dec, ix, "capacity 3")


def test_an_index_that_lies(dec, comp):
    """Point k + 1's out_off raised by one on the host: intervals k and k + 1
    no longer parse to the lengths the index says.  Ranges that touch them are
    BAD_DATA, every other range is right."""
    ix = built(dec, comp, 1, "text", 6)
    assert ix.npts >= 6
    k = 2
    rows = ix.rows.copy()
    rows[k + 2, 0] += 1
    ends = ix.offs + [len(ix.data)]
    ranges = [(0, 100), (ends[k] - 50, 40), (ends[k] - 5, 10), (ends[k] + 9, 100),
              (ends[k + 1] + 5, 7), (ends[k + 2] - 9, 9), (ends[k + 2] - 1, 2),
              (ends[k + 2] + 1, 3000), (ends[k + 3], ends[k + 4] - ends[k + 3]),
              (0, ends[k]), (ends[k + 2] + 1, len(ix.data) - ends[k + 2] - 1)]
    touches = [n > 0 and a + n > ends[k] and a < ends[k + 2] for a, n in ranges]
    res, got = read(dec, ix, ranges, rows=rows)
    assert res == [BAD_DATA if t else 0 for t in touches], (res, touches)
    at = 0
    for (a, n), t in zip(ranges, touches):
        if not t:
            assert got[at:at + n] == ix.data[a:a + n], (a, n)
        at += n


def test_input_that_does_not_belong(dec, comp):
    """64 bytes of d_in inside interval k overwritten: every range that does
    not touch interval k is right, every result is 0 or BAD_DATA, nothing is
    written outside d_out.  No claim on the touched ranges."""
    ix = built(dec, comp, 1, "text", 6)
    assert ix.npts >= 6
    k = 3
    raw_off = int(ix.rows[0, 2])
    mid = (int(ix.rows[k + 1, 1]) + int(ix.rows[k + 2, 1])) // 16
    assert int(ix.rows[k + 1, 1]) // 8 + 8 < mid and mid + 72 < int(ix.rows[k + 2, 1]) // 8
    keep = ix.keep.clone()
    view = keep[3:3 + len(ix.z)]
    view[raw_off + mid:raw_off + mid + 64] = 0xFF
    ends = ix.offs + [len(ix.data)]
    ranges = [(0, 100), (ends[k] - 50, 50), (ends[k] - 5, 10), (ends[k] + 9, 100),
              (ends[k + 1] - 3, 3), (ends[k + 1], 5000), (ends[k - 1], ends[k] - ends[k - 1]),
              (ends[k + 1], len(ix.data) - ends[k + 1]), (0, ends[k])]
    touches = [a + n > ends[k] and a < ends[k + 1] for a, n in ranges]
    res, got = read(dec, ix, ranges, view=view)
    assert all(r in (0, BAD_DATA) for r in res), res
    at = 0
    for (a, n), t, r in zip(ranges, touches, res):
        if not t:
            assert r == 0 and got[at:at + n] == ix.data[a:a + n], (a, n, r)
        at += n
    print("results of the touched ranges:", [r for r, t in zip(res, touches) if t])


def test_a_side_stream(dec, comp):
    """The read is enqueued on a non-default stream behind the copy that
    writes its input there; one synchronisation, then the bytes are right."""
    import torch
    ix = built(dec, comp, 1, "text", 6)
    ends = ix.offs + [len(ix.data)]
    ranges = [(ends[1] - 3, 70000), (5, 0), (ends[-2] + 1, ends[-1] - ends[-2] - 1)]
    t_in = torch.full((len(ix.z) + 6,), 0x33, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t_in[3:3 + len(ix.z)].copy_(ix.view, non_blocking=True)
    res, got = read(dec, ix, ranges, view=t_in[3:3 + len(ix.z)], stream=s)
    assert res == [0, 0, 0] and got == expected(ix.data, ranges)
