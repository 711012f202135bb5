"""Files of concatenated gzip members for the tests of the member finder
(libdeflate_amd_gzip_members_decompress_batch), written with Python's zlib
and hand-written headers only.  Every file keeps the list of its members
(offset, size, uncompressed size) as it was put together, so the tests compare
the library's index with what was recorded and the decoded bytes with
gzip.decompress().

The adversarial files carry gzip signatures - whole members, even - inside
level-0 (stored) payloads; each helper asserts that the false candidates are
really there.  The defect files are one good file with one thing wrong."""
import gzip
import random
import struct
import zlib

import numpy as np

from tests import datagen

SIG = b"\x1f\x8b\x08"
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


def member(data, level=6, mtime=0, xfl=0, os=255, extra=None, name=None, comment=None,
           hcrc=False, text=False):
    """one gzip member (RFC 1952) around a raw DEFLATE stream of zlib's"""
    flg = (FTEXT if text else 0) | (FHCRC if hcrc else 0) | (FEXTRA if extra is not None else 0)
    flg |= (FNAME if name is not None else 0) | (FCOMMENT if comment is not None else 0)
    head = SIG + struct.pack("<BIBB", flg, mtime, xfl, os)
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    for s in (name, comment):
        if s is not None:
            assert 0 not in s
            head += s + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    return head + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


class File:
    def __init__(self, pieces, name=""):
        """pieces: (member bytes, plain bytes) in file order"""
        self.name, self._rows = name, None
        self.members, blob, plain = [], bytearray(), bytearray()
        for mem, data in pieces:
            assert mem[:3] == SIG and gzip.decompress(mem) == data
            self.members.append((len(blob), len(mem), len(data)))
            blob += mem
            plain += data
        self.data, self.plain = bytes(blob), bytes(plain)
        assert gzip.decompress(self.data) == self.plain

    @property
    def m(self):
        return len(self.members)

    def rows(self):
        """the index: (compressed, uncompressed) offset of every member, then
        the closing pair"""
        if self._rows is None:
            out, u = [], 0
            for off, _, size in self.members:
                out.append((off, u))
                u += size
            self._rows = np.array(out + [(len(self.data), u)], dtype=np.uint64).reshape(-1, 2)
        return self._rows.copy()

    def __repr__(self):
        return f"<{self.name}: {self.m} members, {len(self.data)} bytes>"


def piece(data, level=6, **kw):
    return member(data, level, **kw), data


def text(n, seed):
    return datagen.text_chunk(n, seed)


def n_candidates(data):
    """offsets that pass the candidate rule of include/libdeflate_amd.h"""
    n, k, p = len(data), 0, data.find(SIG)
    while p >= 0 and p + 18 <= n:
        k += not data[p + 3] & 0xE0
        p = data.find(SIG, p + 1)
    return k


# ---- shapes ----

def one():
    return File([piece(text(5000, 1))], "one")


def two():
    return File([piece(text(3000, 2)), piece(text(70000, 3), 9)], "two")


def tiny(count=2100, seed=4):
    """members of 20 to 40 bytes: more than two blocks of 1024 candidates"""
    rng = random.Random(seed)
    pieces = []
    for _ in range(count):
        data = bytes(rng.choice(b"abcdefgh") for _ in range(rng.randrange(0, 15)))
        pieces.append(piece(data))
        assert 20 <= len(pieces[-1][0]) <= 40
    return File(pieces, f"tiny{count}")


def empties():
    """an empty 20-byte member at the front, in the middle and at the end"""
    e = piece(b"")
    assert len(e[0]) == 20
    return File([e, piece(text(4000, 5)), e, piece(text(900, 6), 1), e], "empties")


def flagged():
    """FEXTRA + FNAME + FCOMMENT + FHCRC, free MTIME / XFL / OS"""
    kw = dict(extra=b"ab\x03\x00xyz", name=b"a name.txt", comment=b"and a comment", hcrc=True)
    return File([piece(text(6000, 7), mtime=0x5F3759DF, xfl=2, os=3, text=True, **kw),
                 piece(text(100, 8), 1, extra=b"", name=b"n", hcrc=True),
                 piece(b"", comment=b"an empty one", hcrc=True),
                 piece(text(20000, 9), 9, **kw)], "flagged")


def stored():
    return File([piece(text(n, 10 + k), 0) for k, n in enumerate((1, 300, 70000, 65535, 4000))],
                "stored")


def mixed(count=300, seed=11):
    """members between 1 byte and 200 KiB of text at levels 1, 6 and 9"""
    rng = random.Random(seed)
    sizes = [1, 200 << 10] + [int(100000 ** rng.random()) for _ in range(count - 2)]
    rng.shuffle(sizes)
    return File([piece(text(n, 100 + k), (1, 6, 9)[k % 3]) for k, n in enumerate(sizes)],
                f"mixed{count}")


def boundary(at):
    """the second member's signature starts at offset `at`: the first member's
    FNAME is padded to put it there"""
    data = text(2000, 12)
    pad = at - len(member(data, name=b""))
    assert pad >= 0
    first = piece(data, name=b"n" * pad)
    assert len(first[0]) == at
    f = File([first, piece(text(3000, 13), 1), piece(text(500, 14))], f"boundary{at}")
    assert f.members[1][0] == at
    return f


BOUNDARIES = (4093, 4094, 4095, 4096, 16381, 16382, 16383, 16384)


def shapes():
    return [one(), two(), tiny(), empties(), flagged(), stored(), mixed()]


# ---- false candidates ----

def _around(payload, name, false):
    """a level-0 member of `payload` between ordinary members"""
    mid = piece(payload, 0)
    assert payload in mid[0], "one stored block expected"
    f = File([piece(text(9000, 20)), piece(text(1234, 21), 1), mid, piece(text(5000, 22)),
              piece(text(77, 23), 9)], name)
    assert n_candidates(f.data) >= f.m + false, "the false candidates are gone"
    return f


def false_candidates(kind, seed=0xFA15E):
    rng = random.Random(seed)
    noise = lambda n: bytes(rng.randrange(32, 127) for _ in range(n))    # noqa: E731
    if kind == "member":    # a complete valid member in a payload: counts, is not on the chain
        return _around(noise(500) + member(text(4000, 24)) + noise(700), "false-member", 1)
    if kind == "pair":      # one false candidate's successor is another false candidate
        return _around(noise(300) + member(text(2000, 25), 1) + member(text(900, 26)) +
                       noise(400), "false-pair", 2)
    if kind == "junk":      # a header and no stream behind it
        return _around(noise(400) + SIG + b"\0" + noise(600), "false-junk", 1)
    if kind == "stride3":   # overlapping candidates in one thread's 16 bytes
        return _around(noise(100) + SIG * 200 + noise(100), "false-stride3", 199)
    if kind == "names":     # headers with FNAME set in front of bytes without a zero
        return _around(noise(100) + (SIG + b"\x08") * 300 + noise(3000), "false-names", 300)
    raise ValueError(kind)


FALSE_KINDS = ("member", "pair", "junk", "stride3", "names")
NAME_MAX = 65536    # LIBDEFLATE_AMD_GZM_NAME_MAX: bytes of FNAME + FCOMMENT, terminators included


def long_names(total):
    """a member whose FNAME and FCOMMENT take `total` bytes together, between
    ordinary members: a member to the reader up to NAME_MAX, none above"""
    name = b"n" * (total // 2 - 1)
    comment = b"c" * (total - len(name) - 2)
    assert len(name) + len(comment) + 2 == total
    return File([piece(text(700, 40)), piece(text(2000, 41), name=name, comment=comment),
                 piece(text(300, 42), 1)], f"names{total}")


def overflow():
    """one level-0 member whose payload holds 1500 four-byte signatures: 1501
    candidates"""
    payload = (SIG + b"\0") * 1500 + b"." * 32
    mem = member(payload, 0)
    assert payload in mem
    f = File([(mem, payload)], "overflow")
    assert n_candidates(f.data) == 1501
    return f


def good_files():
    """every file the reader must read; overflow() needs max_members >= 477"""
    return (shapes() + [boundary(at) for at in BOUNDARIES] +
            [false_candidates(k) for k in FALSE_KINDS] + [overflow(), long_names(NAME_MAX)])


# ---- defects, one per file ----

def defect_base():
    return File([piece(text(3000, 30)), piece(text(800, 31), 1), piece(text(12000, 32), 9),
                 piece(text(50, 33)), piece(text(2500, 34), 1, name=b"last")], "defect-base")


def defects():
    """(name, bytes) of defect_base() with one thing wrong"""
    f = defect_base()
    b = f.data
    off = [o for o, _, _ in f.members]
    end = [o + s for o, s, _ in f.members]

    def flip(at, bit=1):
        x = bytearray(b)
        x[at] ^= bit
        return bytes(x)
    return [("crc", flip(end[2] - 8)), ("isize", flip(end[2] - 3)),
            ("truncated", b[:-9]), ("zero1", b + b"\0"), ("zero8", b + b"\0" * 8),
            ("reserved", flip(off[3] + 3, 0x20)), ("nosig", flip(off[0], 0xFF)),
            ("empty", b"")]
