"""A pure-Python reader of BGZF files (SAM/BAM spec 4.1), written from the
spec: it checks every member's fixed header, its BSIZE against the bytes that
follow, its CRC-32 and ISIZE, and the EOF member, and returns what it found.
The GPU tests use it as the structural oracle of libdeflate_amd's BGZF
output; tests/test_bgzf_abi.py checks it against files built with zlib."""
import struct
import zlib

PREFIX = bytes.fromhex("1f8b08040000000000ff060042430200")
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEADER = 18
MEMBER_MAX = 65536
BLOCK = 65280


class BgzfError(ValueError):
    pass


class Member:
    __slots__ = ("offset", "size", "body", "crc", "isize", "data")

    def __init__(self, offset, size, body, crc, isize, data):
        self.offset, self.size, self.body = offset, size, body
        self.crc, self.isize, self.data = crc, isize, data


def walk(buf, require_eof=True):
    """-> (members, has_eof): every member before the EOF member (which is
    not listed), each decoded and checked.  Raises BgzfError on any
    deviation from the spec's layout."""
    buf = bytes(buf)
    members, pos, has_eof = [], 0, False
    while pos < len(buf):
        if buf[pos:pos + 16] != PREFIX:
            raise BgzfError(f"member at {pos}: header {buf[pos:pos + 16].hex()}")
        if len(buf) - pos < HEADER + 8:
            raise BgzfError(f"member at {pos}: truncated")
        size = struct.unpack_from("<H", buf, pos + 16)[0] + 1
        if size < HEADER + 8 or pos + size > len(buf):
            raise BgzfError(f"member at {pos}: BSIZE {size - 1} runs past the file")
        if buf[pos:pos + size] == EOF_MEMBER:
            if pos + size != len(buf):
                raise BgzfError(f"EOF member at {pos} is not the last")
            has_eof = True
            break
        body = buf[pos + HEADER:pos + size - 8]
        crc, isize = struct.unpack_from("<II", buf, pos + size - 8)
        d = zlib.decompressobj(-15)
        try:
            data = d.decompress(body) + d.flush()
        except zlib.error as e:
            raise BgzfError(f"member at {pos}: {e}") from None
        if not d.eof or d.unused_data:
            raise BgzfError(f"member at {pos}: the deflate stream does not end at BSIZE")
        if zlib.crc32(data) != crc or len(data) != isize:
            raise BgzfError(f"member at {pos}: CRC / ISIZE mismatch")
        if isize > BLOCK:
            raise BgzfError(f"member at {pos}: {isize} bytes of input")
        members.append(Member(pos, size, body, crc, isize, data))
        pos += size
    if require_eof and not has_eof:
        raise BgzfError("no EOF member")
    return members, has_eof


def member(data, level=6):
    """One BGZF member of `data` by zlib (the hand-built reference)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    return (PREFIX + struct.pack("<H", HEADER + len(body) + 8 - 1) + body +
            struct.pack("<II", zlib.crc32(data), len(data)))


def build(data, level=6, eof=True):
    """A whole BGZF file of `data` by zlib: members of BLOCK bytes."""
    out = b"".join(member(data[k:k + BLOCK], level) for k in range(0, len(data), BLOCK))
    return out + (EOF_MEMBER if eof else b"")
