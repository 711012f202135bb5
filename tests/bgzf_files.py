"""BGZF files for the reader's tests, built from bgzf_walk.member() pieces.
Every file keeps the list of its members (offset, size, ISIZE) as it was put
together, so the tests compare the library's index with what was recorded and
the decoded bytes with gzip.decompress(); bgzf_walk.walk() describes what our
own writer may produce and is stricter than a reader may be (no EOF member in
the middle, no member of 65 536 input bytes), so it is used only where it
applies.

The adversarial files carry the member signature inside level-0 (stored)
payloads; each helper asserts that the false hits are really there."""
import gzip
import random
import struct

import numpy as np

from tests import bgzf_walk

PREFIX = bgzf_walk.PREFIX
EOF = bgzf_walk.EOF_MEMBER
B = bgzf_walk.BLOCK


class File:
    def __init__(self, pieces, eof=True, name=""):
        """pieces: (member bytes, plain bytes) in file order"""
        self.name, self._rows = name, None
        self.members, blob, plain = [], bytearray(), bytearray()
        for mem, data in list(pieces) + ([(EOF, b"")] if eof else []):
            assert mem[:4] == PREFIX[:4] and len(mem) == (mem[16] | mem[17] << 8) + 1
            self.members.append((len(blob), len(mem), len(data)))
            blob += mem
            plain += data
        self.data, self.plain = bytes(blob), bytes(plain)
        self.has_eof = bool(self.members) and self.data[self.members[-1][0]:] == EOF
        if self.data:
            assert gzip.decompress(self.data) == self.plain

    @property
    def m(self):
        return len(self.members)

    def rows(self):
        """the index: (compressed, uncompressed) offset of every member, then
        the closing pair"""
        if self._rows is None:
            out, u = [], 0
            for off, _, isize in self.members:
                out.append((off, u))
                u += isize
            self._rows = np.array(out + [(len(self.data), u)], dtype=np.uint64).reshape(-1, 2)
        return self._rows.copy()

    def voffset(self, u):
        """the BAM virtual offset of uncompressed offset u (in the first
        non-empty member that holds it; the end of the data is the closing
        pair's)"""
        rows = self.rows()
        if u == len(self.plain):
            return len(self.data) << 16
        # the last member that starts at or before u is the non-empty one
        k = int(np.searchsorted(rows[:-1, 1], u, side="right")) - 1
        assert self.members[k][2] and int(rows[k][1]) <= u < int(rows[k + 1][1])
        return int(rows[k][0]) << 16 | (u - int(rows[k][1]))


def text(n, seed):
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"acgtn") for _ in range(rng.randrange(3, 12))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
        if rng.random() < 0.05:
            out += bytes(rng.randrange(256) for _ in range(20))
    return bytes(out[:n])


def piece(data, level=6):
    return bgzf_walk.member(data, level), data


def plain_file(n, seed, level=6, eof=True, block=B):
    data = text(n, seed)
    return File([piece(data[k:k + block], level) for k in range(0, n, block)], eof,
                f"plain{n}/l{level}")


def cut_file(n, seed, level=6, lo=1, hi=B):
    """members cut at random sizes lo..hi, as a record-aligned writer does"""
    rng, data, pieces, k = random.Random(seed), text(n, seed), [], 0
    while k < n:
        size = rng.randrange(lo, hi + 1)
        pieces.append(piece(data[k:k + size], level))
        k += size
    return File(pieces, True, f"cut{n}/l{level}")


def cat_file(seed):
    """`cat a.gz b.gz`: an EOF member in the middle"""
    a, b = plain_file(150000, seed), plain_file(70000, seed + 1, level=1)
    pieces = [(a.data[o:o + s], a.plain[u:u + i]) for (o, s, i), u in
              zip(a.members, a.rows()[:, 1].astype(int))]
    pieces += [(b.data[o:o + s], b.plain[u:u + i]) for (o, s, i), u in
               zip(b.members[:-1], b.rows()[:, 1].astype(int))]
    f = File(pieces, True, "cat")
    assert f.data == a.data + b.data
    return f


def big_isize_file():
    """a member of exactly 65 536 input bytes (the spec's limit, above our
    writer's 65 280), and MTIME / XFL / OS bytes that are not htslib's"""
    data = bytes(range(256)) * 256
    mem = bytearray(bgzf_walk.member(data))
    assert len(data) == 65536 and len(mem) < 1000
    other = bytearray(bgzf_walk.member(b"mtime and os set"))
    other[4:8] = struct.pack("<I", 0x5F3759DF)
    other[8], other[9] = 2, 3
    f = File([(bytes(mem), data), (bytes(other), b"mtime and os set"), piece(text(5000, 3))],
             True, "isize65536")
    return f


def fake_header(size):
    assert 28 <= size <= 65536
    return PREFIX + struct.pack("<H", size - 1)


def _stored_with_fakes(payload, fakes, tail_len):
    """a level-0 member of `payload` in which the 18 bytes at payload offset k
    are a header whose size ends `after` bytes past the end of this member,
    for every (k, after) of `fakes`.  tail_len: bytes of the file behind this
    member (a fake's size must stay inside the file to be a candidate)."""
    payload = bytearray(payload)
    marks = []
    for k, _ in fakes:
        payload[k:k + 18] = fake_header(28)
    mem = bgzf_walk.member(bytes(payload), level=0)
    for k, after in fakes:
        at = mem.find(bytes(payload[k:k + 16]), 18 + k)
        assert at == 18 + 5 + k, "one stored block expected"
        size = len(mem) - at + after
        assert after <= tail_len
        payload[k:k + 18] = fake_header(size)
        marks.append(at)
    mem = bgzf_walk.member(bytes(payload), level=0)
    return mem, bytes(payload), marks


def adversarial(kind, seed=0xADF0):
    """-> (File, candidates that are no members: at least this many)"""
    rng = random.Random(seed)
    noise = lambda n: bytes(rng.randrange(1, 250) for _ in range(n))    # noqa: E731
    head = [piece(text(30000, seed + 1)), piece(text(12345, seed + 2), 1)]
    tail = [piece(text(20000, seed + 3)), piece(text(777, seed + 4), 9)]
    tail_len = sum(len(t[0]) for t in tail) + len(EOF)
    if kind == "a":     # a complete real member inside a stored payload
        inner = bgzf_walk.member(text(4000, seed + 5))
        payload = noise(500) + inner + noise(700)
        mid, false = [piece(payload, 0)], 1
    elif kind == "b":   # a fake header that ends exactly on the next true member
        mem, payload, _ = _stored_with_fakes(noise(3000), [(1000, 0)], tail_len)
        mid, false = [(mem, payload)], 1
    elif kind == "c":   # two fake headers, the first pointing at the second
        payload = bytearray(noise(3000))
        payload[2000:2018] = fake_header(28 + 17)       # ends nowhere
        payload[500:518] = fake_header(1500)            # ends at the second one
        mid, false = [piece(bytes(payload), 0)], 2
    elif kind == "d":   # a fake header that ends exactly at the end of the file
        mem, payload, _ = _stored_with_fakes(noise(3000), [(1200, len(EOF))], len(EOF))
        mid, tail, false = [], [(mem, payload)], 1
    elif kind == "e":   # nothing but fake headers: overflows the candidate space
        payload = b"".join(fake_header(rng.randrange(28, 200)) for _ in range(B // 18))
        mid, false = [piece(payload, 0)], B // 18
    else:
        raise ValueError(kind)
    f = File(head + mid + tail, True, f"adversarial-{kind}")
    assert f.data.count(PREFIX) >= f.m + false, "the false hits are gone"
    return f, false


def all_files():
    """the files the finder is checked on, model and kernels alike"""
    out = [File([], False, "empty"), File([], True, "eof-only"),
           plain_file(1, 1), plain_file(65280, 2), plain_file(5 * B + 7, 3),
           plain_file(100000, 4, level=0), plain_file(100000, 5, level=1, eof=False),
           plain_file(200000, 6, level=9), cut_file(400000, 7), cat_file(8),
           big_isize_file()]
    return out + [adversarial(k)[0] for k in "abcde"]
