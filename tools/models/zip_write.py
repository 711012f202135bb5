"""CPU model of the ZIP writer (libdeflate_amd_zip_compress_bound /
_compress_batch): the whole rule of include/libdeflate_amd.h in plain Python.
(names, entries, per-entry raw DEFLATE streams, datetime, flags) -> the
archive's bytes, the result words and the index rows.  The kernels
(csrc/zip_write_kernels.hip) are checked against it byte for byte, and it is
checked against Python's zipfile and the reader's model (tools/models/
zip_walk.py) in tests/test_zip_write_abi.py."""
import struct
import zlib
from collections import namedtuple

SUCCESS, INSUFFICIENT_SPACE = 0, 3
STORE, FORCE_ZIP64 = 1, 2
RESULT_WORDS, WORDS = 4, 8
LOCAL_BYTES, CEN_BYTES, CEN64_EXTRA, END_BYTES, END64_BYTES = 30, 46, 12, 22, 76
MARK32, MARK16 = 0xFFFFFFFF, 0xFFFF
DEFAULT_DATETIME = 0x00210000   # 1980-01-01 00:00

Archive = namedtuple("Archive", "data words rows zip64")


def bound(name_lens, sizes, flags=0):
    """-> (the exact bound, ZIP64 mode, bytes of the directory, bytes behind it)"""
    n = len(sizes)
    assert len(name_lens) == n
    locals_ = sum(LOCAL_BYTES + a + b for a, b in zip(name_lens, sizes))
    cd = sum(CEN_BYTES + a for a in name_lens)
    z = bool(flags & FORCE_ZIP64) or n >= 65535 or locals_ + cd + END_BYTES >= MARK32
    if z:
        cd += CEN64_EXTRA * n
    end = END_BYTES + (END64_BYTES if z else 0)
    return locals_ + cd + end, z, cd, end


def build(names, entries, streams, dos_datetime=0, flags=0, out_avail=None):
    """names: bytes each; entries: the entries' bytes; streams: per entry the
    raw DEFLATE stream the compressor gives for it, or None (not looked at
    under STORE).  -> Archive: data is None where the archive does not fit
    out_avail (then rows is None too: nothing is written)."""
    n = len(names)
    assert len(entries) == n and len(streams) == n
    _, z, cd_size, end_bytes = bound([len(x) for x in names], [len(x) for x in entries], flags)
    dt = dos_datetime or DEFAULT_DATETIME
    ver = 45 if z else 20
    parts, cen, rows, at, uoff, deflated = [], [], [], 0, 0, 0
    for name, raw, s in zip(names, entries, streams):
        assert 0 < len(name) <= 65535 and len(raw) < 1 << 32
        use = not (flags & STORE) and s is not None and len(raw) and len(s) < len(raw)
        body, method = (s, 8) if use else (raw, 0)
        deflated += method == 8
        gp = 0x800 if any(b >= 0x80 for b in name) else 0
        crc = zlib.crc32(raw)
        fields = (ver, gp, method, dt & 0xFFFF, dt >> 16, crc, len(body), len(raw), len(name))
        parts.append(struct.pack("<4sHHHHHIIIHH", b"PK\3\4", *fields, 0) + name + body)
        extra = struct.pack("<HHQ", 1, 8, at) if z else b""
        cen.append(struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\1\2", ver, *fields, len(extra), 0, 0,
                               0, 0, MARK32 if z else at) + name + extra)
        rows.append([None, len(name), method | gp << 16, crc, at + LOCAL_BYTES + len(name),
                     len(body), len(raw), uoff])
        at += LOCAL_BYTES + len(name) + len(body)
        uoff += len(raw)
    cd_off, rel = at, 0
    for row, rec in zip(rows, cen):
        row[0] = cd_off + rel
        rel += len(rec)
    assert rel == cd_size
    if z:
        end = struct.pack("<4sQHHIIQQQQ", b"PK\6\6", 44, 45, 45, 0, 0, n, n, cd_size, cd_off)
        end += struct.pack("<4sIQI", b"PK\6\7", 0, cd_off + cd_size, 1)
        end += struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, MARK16, MARK16, MARK32, MARK32, 0)
    else:
        end = struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, n, n, cd_size, cd_off, 0)
    assert len(end) == end_bytes
    total = cd_off + cd_size + end_bytes
    if out_avail is not None and total > out_avail:
        return Archive(None, [INSUFFICIENT_SPACE, total, cd_off, deflated], None, z)
    data = b"".join(parts) + b"".join(cen) + end
    assert len(data) == total
    return Archive(data, [SUCCESS, total, cd_off, deflated], rows, z)
