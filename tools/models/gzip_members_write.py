"""CPU model of the gzip-members writer
(libdeflate_amd_gzip_members_compress_bound / _compress_batch): the whole rule
of include/libdeflate_amd.h in plain Python.  (records, per-record raw DEFLATE
streams, names, mtime, level) -> the file's bytes, the result words and the
index pairs.  The kernels (csrc/gzip_members_write_kernels.hip) are checked
against it byte for byte, and it is checked against Python's gzip and a zlib
member walk in tests/test_gzip_members_write_abi.py."""
import struct
import zlib
from collections import namedtuple

SUCCESS, INSUFFICIENT_SPACE = 0, 3
RESULT_WORDS = 4
HEADER_BYTES, FOOTER_BYTES = 10, 8
NAME_MAX = 65534
FNAME = 8
EMPTY_STREAM = b"\x01\x00\x00\xff\xff"     # what the compressor makes of 0 bytes

File = namedtuple("File", "data words index")


def deflate_bound(n):
    """libdeflate_deflate_compress_bound"""
    return n + 5 * max(1, -(-n // 5000))


def bound(sizes, name_lens=None):
    """Sum(libdeflate_gzip_compress_bound(size) + (name ? name + 1 : 0))"""
    if name_lens is None:
        name_lens = [0] * len(sizes)
    assert len(name_lens) == len(sizes)
    return sum(HEADER_BYTES + FOOTER_BYTES + deflate_bound(s) + (nl + 1 if nl else 0)
               for s, nl in zip(sizes, name_lens))


def xfl(level):
    """lib/gzip_compress.c:56-62"""
    return 4 if level < 2 else 2 if level >= 8 else 0


def member(raw, stream, name=b"", mtime=0, level=6):
    """one member: the 10 fixed bytes, the name field, the stream, CRC-32 and
    ISIZE"""
    assert len(name) <= NAME_MAX and 0 not in name and len(raw) < 1 << 32
    head = struct.pack("<BBBBIBB", 0x1F, 0x8B, 8, FNAME if name else 0, mtime, xfl(level), 0xFF)
    return head + (name + b"\0" if name else b"") + stream + \
        struct.pack("<II", zlib.crc32(raw), len(raw))


def build(records, streams, names=None, mtime=0, level=6, out_avail=None):
    """records: the records' bytes; streams: per record the raw DEFLATE stream
    the compressor gives for it (None for a record of 0 bytes: the empty final
    stored block); names: None, or per record bytes (b"" / None: no name).
    -> File: data and index are None where the file does not fit out_avail
    (nothing is written then)."""
    n = len(records)
    assert len(streams) == n and (names is None or len(names) == n)
    parts, index, at, uoff = [], [], 0, 0
    for k, (raw, s) in enumerate(zip(records, streams)):
        if s is None:
            assert not raw
            s = EMPTY_STREAM
        m = member(raw, s, (names[k] or b"") if names is not None else b"", mtime, level)
        parts.append(m)
        index.append([at, uoff])
        at += len(m)
        uoff += len(raw)
    index.append([at, uoff])
    fits = out_avail is None or at <= out_avail
    words = [SUCCESS if fits else INSUFFICIENT_SPACE, at, uoff, n]
    return File(b"".join(parts) if fits else None, words, index if fits else None)


def walk(data):
    """the member walk of zlib: -> (index pairs with the closing pair, the
    members' bytes)"""
    index, plain, at, uoff = [], [], 0, 0
    while at < len(data):
        d = zlib.decompressobj(31)
        out = d.decompress(data[at:])
        assert d.eof
        index.append([at, uoff])
        plain.append(out)
        at = len(data) - len(d.unused_data)
        uoff += len(out)
    index.append([at, uoff])
    return index, plain
