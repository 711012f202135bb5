"""ZIP archives for the tests of the ZIP reader, built with Python's zipfile
(every good file passes testzip()); the defect files are patched by hand, one
defect per file.  Everything is built once per process and kept."""
import io
import struct
import zipfile
import zlib
from collections import namedtuple

import numpy as np

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
MORE_ENTRIES, MORE_CANDIDATES, UNSUPPORTED = 16, 17, 18

# data: the archive; twin: the same entries in a file zipfile can read (the
# archive itself but for `false`, whose comment holds a look-alike end record
# that zipfile would take for the real one)
Good = namedtuple("Good", "name data twin zip64")
# entry: the one entry that fails (None: the archive as a whole), result: its
# result and the verdict
Defect = namedtuple("Defect", "name data base entry result")

SIZES = (0, 1, 15, 16, 17, 100, 4095, 4096, 4097, 65535, 65536, 300000)
_cache = {}


def _once(fn):
    def wrapped(*a):
        key = (fn.__name__,) + a
        if key not in _cache:
            _cache[key] = fn(*a)
        return _cache[key]
    wrapped.__name__ = fn.__name__
    return wrapped


def payload(n, seed):
    """n bytes that DEFLATE shortens but does not trivialise"""
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 40, size=n // 3 + 2, dtype=np.uint8) + 65
    return np.repeat(words, 3)[:n].tobytes()


def _info(name, method, level=None, comment=b"", extra=b""):
    zi = zipfile.ZipInfo(name, date_time=(2024, 1, 2, 3, 4, 6))
    zi.compress_type = method
    zi._compresslevel = level
    zi.comment = comment
    zi.extra = extra
    return zi


def _write_mixed(zf):
    kinds = [(zipfile.ZIP_DEFLATED, 1), (zipfile.ZIP_DEFLATED, 6), (zipfile.ZIP_DEFLATED, 9),
             (zipfile.ZIP_STORED, None)]
    zf.writestr(_info("dir/", zipfile.ZIP_STORED), b"")
    for i, n in enumerate(SIZES):
        method, level = kinds[i % 4]
        zf.writestr(_info(f"dir/e{n}.bin", method, level), payload(n, i))
    zf.writestr(_info("naïve-ü中.txt", zipfile.ZIP_DEFLATED, 6), payload(777, 90))
    zf.writestr(_info("commented", zipfile.ZIP_DEFLATED, 6, comment=b"an entry comment"),
                payload(3000, 91))
    zf.writestr(_info("extra", zipfile.ZIP_STORED, extra=struct.pack("<HH", 0x7075, 5) + b"\1abcd"),
                payload(50, 92))


@_once
def mixed(comment_len):
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as zf:
        _write_mixed(zf)
        zf.comment = b"c" * comment_len
    return Good(f"mixed{comment_len}", b.getvalue(), b.getvalue(), False)


class _Sink:
    """a file that cannot seek: zipfile writes data descriptors"""

    def __init__(self):
        self.b = io.BytesIO()

    def write(self, x):
        return self.b.write(x)

    def flush(self):
        pass


@_once
def descriptor():
    s = _Sink()
    with zipfile.ZipFile(s, "w") as zf:
        for i, n in enumerate((0, 5, 1000, 70000)):
            zf.writestr(_info(f"d{i}", zipfile.ZIP_DEFLATED if i % 2 else zipfile.ZIP_STORED, 6),
                        payload(n, 20 + i))
    data = s.b.getvalue()
    with zipfile.ZipFile(io.BytesIO(data)) as zf:
        assert all(zi.flag_bits & 8 for zi in zf.infolist())
    return Good("descriptor", data, data, False)


@_once
def zip64():
    """real ZIP64 end records and central ZIP64 extras in a small file: the
    limits at which zipfile switches are lowered while it writes"""
    saved = zipfile.ZIP64_LIMIT, zipfile.ZIP_FILECOUNT_LIMIT
    zipfile.ZIP64_LIMIT, zipfile.ZIP_FILECOUNT_LIMIT = 1000, 5
    try:
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w") as zf:
            for i, n in enumerate((10, 1500, 0, 2000, 30, 1200, 7)):
                zf.writestr(_info(f"z{i}", zipfile.ZIP_DEFLATED if i % 3 else zipfile.ZIP_STORED, 6),
                            payload(n, 40 + i))
    finally:
        zipfile.ZIP64_LIMIT, zipfile.ZIP_FILECOUNT_LIMIT = saved
    data = b.getvalue()
    assert b"PK\6\6" in data and b"PK\6\7" in data
    return Good("zip64", data, data, True)


MANY = 65600


@_once
def many():
    """65 600 stored two-byte entries: a real 0xFFFF count, a ZIP64 end record,
    and a chain across many jump blocks"""
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as zf:
        for i in range(MANY):
            zf.writestr(_info(f"{i:05d}", zipfile.ZIP_STORED), struct.pack("<H", i & 0xFFFF))
    data = b.getvalue()
    return Good("many", data, data, True)


@_once
def trailing(k):
    g = mixed(0)
    data = g.data + b"\0" * k
    return Good(f"trailing{k}", data, data, False)


def _lookalike(n):
    """n bytes of archive comment with an end record in them whose own comment
    would run past the end of the file"""
    fake = b"PK\5\6" + struct.pack("<HHHHIIH", 0, 0, 1, 1, 46, 0, 0xFFFF)
    return (b"xx" + fake + b"y" * n)[:n]


@_once
def false():
    """PK\\1\\2 in names, extras and comments with plausible lengths behind it,
    a stored entry whose data is a whole smaller archive, and a look-alike end
    record inside the archive comment"""
    inner = io.BytesIO()
    with zipfile.ZipFile(inner, "w") as zf:
        zf.writestr(_info("inner-a", zipfile.ZIP_DEFLATED, 6), payload(500, 60))
        zf.writestr(_info("inner-b", zipfile.ZIP_STORED), payload(40, 61))
    # 46 bytes of zeros behind the signature: a record of 46 bytes, whose end
    # lies inside the same field; 0x0101 lengths from a name: one of 817 bytes
    rec = b"PK\1\2" + b"\0" * 60

    def build(comment):
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w") as zf:
            zf.writestr(_info("PK\1\2" + "\1" * 50, zipfile.ZIP_DEFLATED, 6), payload(900, 62))
            zf.writestr(_info("x", zipfile.ZIP_STORED,
                              extra=struct.pack("<HH", 0x7777, len(rec)) + rec), payload(33, 63))
            zf.writestr(_info("y", zipfile.ZIP_DEFLATED, 9, comment=rec), payload(5000, 64))
            zf.writestr(_info("inner.zip", zipfile.ZIP_STORED), inner.getvalue())
            zf.writestr(_info("PK\1\2tail", zipfile.ZIP_STORED), b"PK\1\2" * 30)
            zf.comment = comment
        return b.getvalue()
    twin = build(b"x" * 64)
    data = build(_lookalike(64))
    assert len(twin) == len(data) and twin[:-64] == data[:-64]
    return Good("false", data, twin, False)


@_once
def empty():
    """no entry: an end record alone"""
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w"):
        pass
    assert len(b.getvalue()) == 22
    return Good("empty", b.getvalue(), b.getvalue(), False)


LOOKALIKES = 2000


@_once
def lookalikes():
    """one entry whose comment holds LOOKALIKES signatures: more candidates
    than a small max_entries leaves room for (a limit file, not in
    good_files(): with max_entries exact it is MORE_CANDIDATES)"""
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as zf:
        zf.writestr(_info("one", zipfile.ZIP_DEFLATED, 6, comment=b"PK\1\2" * LOOKALIKES),
                    payload(100, 80))
    return Good("lookalikes", b.getvalue(), b.getvalue(), False)


BOUNDARIES = (4093, 4094, 4095, 4096, 16381, 16382, 16383, 16384)


@_once
def boundary(at):
    """the central directory starts exactly at file offset `at`, around the 4 KiB
    steps and the 16 KiB workgroups of the candidate scan: a stored first entry
    padded to put it there, and right below it a stored last entry of
    look-alike signatures, which lie outside the directory"""
    def build(pad):
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w") as zf:
            zf.writestr(_info("pad", zipfile.ZIP_STORED), payload(pad, 30))
            zf.writestr(_info("a", zipfile.ZIP_DEFLATED, 6), payload(700, 31))
            zf.writestr(_info("b", zipfile.ZIP_DEFLATED, 9), payload(33, 32))
            zf.writestr(_info("sigs", zipfile.ZIP_STORED), b"PK\1\2" * 9)
        return b.getvalue()
    data = build(at - _layout(build(0))[1])
    assert _layout(data)[1] == at and data[at - 4:at + 4] == b"PK\1\2PK\1\2"
    return Good(f"boundary{at}", data, data, False)


GOOD_NAMES = ("mixed0", "mixed1", "mixed65535", "descriptor", "zip64", "many", "trailing1",
              "trailing2", "trailing3", "false", "empty") + tuple(f"boundary{at}" for at in BOUNDARIES)


def good(name):
    """the good file of that name, built on first use"""
    for stem, fn in (("mixed", mixed), ("trailing", trailing), ("boundary", boundary)):
        if name.startswith(stem):
            return fn(int(name[len(stem):]))
    return {"descriptor": descriptor, "zip64": zip64, "many": many, "false": false,
            "empty": empty}[name]()


_expected = {}


def expected(g):
    """(infolist, [bytes of every entry]) as zipfile reads the file, once"""
    if g.name not in _expected:
        with zipfile.ZipFile(io.BytesIO(g.twin)) as zf:
            infos = zf.infolist()   # (read() checks every CRC-32, as testzip() would)
            _expected[g.name] = (infos, [zf.read(zi) for zi in infos])
    return _expected[g.name]


# ---- defects ----

def _layout(data):
    """(end record offset, cd_off, [central record offsets], [local header
    offsets]) of a good archive, walked plainly"""
    p = data.rfind(b"PK\5\6")
    entries, cd_off = struct.unpack_from("<H", data, p + 10)[0], struct.unpack_from("<I", data, p + 16)[0]
    if data[p - 20:p - 16] == b"PK\6\7":
        q = struct.unpack_from("<Q", data, p - 12)[0]
        entries, cd_off = struct.unpack_from("<Q", data, q + 32)[0], struct.unpack_from("<Q", data, q + 48)[0]
    cens, locs, at = [], [], cd_off
    for _ in range(entries):
        assert data[at:at + 4] == b"PK\1\2"
        n, x, c = struct.unpack_from("<HHH", data, at + 28)
        cens.append(at)
        locs.append(struct.unpack_from("<I", data, at + 42)[0])
        at += 46 + n + x + c
    return p, cd_off, cens, locs


@_once
def defect_base():
    """entries 0, 2, 4: deflate; 1, 3, 5: stored"""
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as zf:
        for i, n in enumerate((3000, 100, 70000, 17, 4097, 0)):
            zf.writestr(_info(f"b{i}", zipfile.ZIP_STORED if i % 2 else zipfile.ZIP_DEFLATED, 6),
                        payload(n, 70 + i))
    data = b.getvalue()
    return Good("defect_base", data, data, False)


def _patch(data, at, fmt, fn):
    b = bytearray(data)
    v = struct.unpack_from(fmt, b, at)[0]
    struct.pack_into(fmt, b, at, fn(v))
    return bytes(b)


@_once
def defects():
    g = defect_base()
    d = g.data
    p, cd_off, cens, locs = _layout(d)
    out = []

    def add(name, data, entry, result, base=g):
        assert data != base.data and len(data) == len(base.data)
        out.append(Defect(name, data, base, entry, result))
    # the archive as a whole
    add("end_sig", _patch(d, p, "<B", lambda v: v ^ 1), None, BAD_DATA)
    add("cd_off+1", _patch(d, p + 16, "<I", lambda v: v + 1), None, BAD_DATA)
    for name, step in (("count+1", 1), ("count-1", -1)):
        x = _patch(d, p + 8, "<H", lambda v: v + step)
        add(name, _patch(x, p + 10, "<H", lambda v: v + step), None, BAD_DATA)
    add("cen_sig", _patch(d, cens[2] + 2, "<B", lambda v: v ^ 1), None, BAD_DATA)
    add("name_len+1", _patch(d, cens[2] + 28, "<H", lambda v: v + 1), None, BAD_DATA)
    # one entry
    z = zip64()
    zp, zcd, zcens, zlocs = _layout(z.data)
    k = next(i for i, c in enumerate(zcens) if struct.unpack_from("<I", z.data, c + 24)[0] == 0xFFFFFFFF)
    n = struct.unpack_from("<H", z.data, zcens[k] + 28)[0]
    assert struct.unpack_from("<H", z.data, zcens[k] + 46 + n)[0] == 1
    add("zip64_extra_short", _patch(z.data, zcens[k] + 46 + n + 2, "<H", lambda v: v - 8), k,
        BAD_DATA, base=z)
    add("local_sig", _patch(d, locs[2], "<B", lambda v: v ^ 1), 2, BAD_DATA)
    n4, x4 = struct.unpack_from("<HH", d, locs[4] + 26)
    past = cd_off - (locs[4] + 30 + n4 + x4) + 1
    add("data_past_cd", _patch(d, cens[4] + 20, "<I", lambda v: past), 4, BAD_DATA)
    add("stored_sizes", _patch(d, cens[1] + 24, "<I", lambda v: v + 1), 1, BAD_DATA)
    add("crc", _patch(d, cens[2] + 16, "<I", lambda v: v ^ 0x10), 2, BAD_DATA)
    n2, x2 = struct.unpack_from("<HH", d, locs[2] + 26)
    # BTYPE 3 in the first block header: no DEFLATE stream
    add("deflate_byte", _patch(d, locs[2] + 30 + n2 + x2, "<B", lambda v: v | 6), 2, BAD_DATA)
    add("usize-1", _patch(d, cens[2] + 24, "<I", lambda v: v - 1), 2, INSUFFICIENT_SPACE)
    add("usize+1", _patch(d, cens[2] + 24, "<I", lambda v: v + 1), 2, SHORT_OUTPUT)
    add("flag_bit0", _patch(d, cens[2] + 8, "<H", lambda v: v | 1), 2, UNSUPPORTED)
    add("method12", _patch(d, cens[4] + 10, "<H", lambda v: 12), 4, UNSUPPORTED)
    return out


def crc32(b):
    return zlib.crc32(b) & 0xFFFFFFFF
