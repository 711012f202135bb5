"""tar archives for the tests of the tar reader: the good files are written by
Python's tarfile in its three formats, what tarfile will not write is packed by
hand, and the defect files are patched by hand, one defect per file.
Everything is built once per process and kept."""
import gzip
import io
import tarfile
from collections import namedtuple

import numpy as np

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
MORE_RECORDS, MORE_CANDIDATES, UNSUPPORTED = 16, 17, 18
BLOCK = 512
TILE = 65536
FORMATS = {"ustar": tarfile.USTAR_FORMAT, "gnu": tarfile.GNU_FORMAT, "pax": tarfile.PAX_FORMAT}

# data: the archive; readable: tarfile reads it and must agree
Good = namedtuple("Good", "name data readable")
# an archive whose chain breaks: LIBDEFLATE_BAD_DATA as a whole
Defect = namedtuple("Defect", "name data")

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
    rng = np.random.default_rng(seed)
    return rng.integers(1, 256, size=n, dtype=np.uint8).tobytes()


def text(n, seed):
    """n bytes of text that gzip shortens well"""
    rng = np.random.default_rng(seed)
    words = [b"tar", b"header", b"block", b"entry", b"prefix", b"checksum", b"octal", b"walk",
             b"chain", b"device", b"index", b"range", b"\n"]
    picks = rng.integers(0, len(words), size=n // 3 + 1)
    return b" ".join(words[i] for i in picks)[:n].ljust(n, b".")


# ---- hand-packed records ----

def header(name, size=0, typeflag=b"0", prefix=b"", magic=b"ustar\x0000", mtime=0o14567,
           size_field=None, signed=False, linkname=b""):
    """one 512-byte header; size_field overrides the octal size, signed stores
    the checksum as the sum of signed chars"""
    h = bytearray(BLOCK)
    h[0:len(name)] = name
    h[100:108] = b"0000644\0"
    h[108:116] = b"0000000\0"
    h[116:124] = b"0000000\0"
    h[124:136] = size_field if size_field is not None else b"%011o\0" % size
    h[136:148] = b"%011o\0" % mtime
    h[148:156] = b" " * 8
    h[156:157] = typeflag
    h[157:157 + len(linkname)] = linkname
    h[257:257 + len(magic)] = magic
    h[345:345 + len(prefix)] = prefix
    s = sum(h)
    if signed:
        s -= 256 * sum(1 for b in h if b >= 0x80)
    h[148:156] = b"%06o\0 " % s
    return bytes(h)


def pad(data):
    return data + bytes(-len(data) % BLOCK)


def member(name, data=b"", **kw):
    return header(name, size=len(data), **kw) + pad(data)


def pax_record(key, value):
    body = b" " + key + b"=" + value + b"\n"
    n = len(body) + 1
    while len(b"%d" % n) + len(body) != n:
        n = len(b"%d" % n) + len(body)
    return b"%d" % n + body


END = bytes(2 * BLOCK)


# ---- the good files ----

def _add(tf, name, data=None, kind=tarfile.REGTYPE, link=""):
    ti = tarfile.TarInfo(name)
    ti.type = kind
    ti.mtime = 1700000000 + len(name)
    ti.linkname = link
    if data is not None:
        ti.size = len(data)
    tf.addfile(ti, io.BytesIO(data) if data is not None else None)


@_once
def inner_tar():
    """a complete little archive: the data of the nested entry"""
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=tarfile.USTAR_FORMAT) as tf:
        _add(tf, "inner/a.txt", payload(700, 1))
        _add(tf, "inner/empty")
        _add(tf, "inner/b.bin", payload(5, 2))
        _add(tf, "inner/dir", kind=tarfile.DIRTYPE)
    return b.getvalue()


def _write_mixed(tf, fmt):
    _add(tf, "dir", kind=tarfile.DIRTYPE)
    for i, n in enumerate((0, 1, 511, 512, 513, 4096)):
        _add(tf, "dir/e%d.bin" % n, payload(n, i))
    _add(tf, "d" * 60 + "/" + "s" * 50 + "/" + "f" * 40, payload(33, 20))      # prefix-split
    if fmt != "ustar":
        _add(tf, "long/" + "n" * 295, payload(77, 21))                             # 300 characters
        _add(tf, "long/" + "m" * 150 + "/", kind=tarfile.DIRTYPE)
    _add(tf, "naïve-ü中.txt", payload(100, 22))
    _add(tf, "sym", kind=tarfile.SYMTYPE, link="dir/e1.bin")
    _add(tf, "hard", kind=tarfile.LNKTYPE, link="dir/e511.bin")
    _add(tf, "nested.tar", inner_tar())
    _add(tf, "zeros-middle", bytes(3 * BLOCK))
    _add(tf, "after", payload(1000, 23))
    _add(tf, "zeros-end", bytes(2 * BLOCK + 7))


@_once
def mixed(fmt):
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=FORMATS[fmt]) as tf:
        _write_mixed(tf, fmt)
    return Good("mixed_" + fmt, b.getvalue(), True)


def body_end(data):
    """where the last record of a tarfile-written archive ends"""
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:") as tf:
        last = tf.getmembers()[-1]
    return last.offset_data + (last.size + BLOCK - 1) // BLOCK * BLOCK if last.isreg() \
        else last.offset_data


@_once
def cut(fmt):
    d = mixed(fmt).data
    return Good("cut_" + fmt, d[:body_end(d)], True)


@_once
def one_zero(fmt):
    d = mixed(fmt).data
    return Good("onezero_" + fmt, d[:body_end(d) + BLOCK], True)


@_once
def garbage(fmt):
    d = mixed(fmt).data
    e = body_end(d)
    return Good("garbage_" + fmt, d[:e + 2 * BLOCK] + inner_tar() + payload(700, 30), True)


@_once
def empty():
    return Good("empty", bytes(20 * BLOCK), True)


@_once
def wg_edges():
    """one scan workgroup covers 32 blocks: a header in block 31 whose
    look-ahead block is block 32, and a header in block 32"""
    d = member(b"a", payload(30 * BLOCK, 40)) + member(b"b31") + member(b"c32", payload(600, 41))
    d += member(b"d", payload(28 * BLOCK - 3, 42))      # header at 35, data to 63
    d += member(b"e63", payload(BLOCK, 43))             # header at 63, data at 64
    assert len(member(b"a", payload(30 * BLOCK, 40))) == 31 * BLOCK
    return Good("wg_edges", d + END, True)


@_once
def many():
    """1100 one-block records: the chain crosses a jump block of 1024"""
    return Good("many", b"".join(member(b"f%04d" % i) for i in range(1100)) + END, True)


@_once
def straddle(fmt):
    """records 0 .. 1022 are one-block files, record 1023 is the L (gnu) or x
    (pax) record of the entry that is record 1024"""
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=FORMATS[fmt]) as tf:
        for i in range(1023):
            _add(tf, "f%04d" % i)
        _add(tf, "long/" + "q" * 200, payload(900, 50))
        _add(tf, "tail", payload(10, 51))
    return Good("straddle_" + fmt, b.getvalue(), True)


@_once
def hand():
    """headers tarfile reads but does not write"""
    d = member(b"first", payload(100, 60))
    d += header(b"base256", size_field=b"\x80" + (700).to_bytes(11, "big")) + pad(payload(700, 61))
    d += member(b"sign\xe9\xfc\xff", payload(50, 62), signed=True)
    d += member(b"v7", payload(513, 63), magic=b"")
    d += header(b"hardlink", size=1234, typeflag=b"1", linkname=b"first")   # no data blocks
    d += member(b"odd-type", payload(20, 64), typeflag=b"Z")                # unknown: a regular file
    d += member(b"last", payload(1, 65))
    return Good("hand", d + END, True)


@_once
def unsupported():
    """nine extension records in front of one entry, a pax size= key and
    typeflag S: each refused alone, the neighbours extracted"""
    d = member(b"n0", payload(300, 70))
    for i in range(9):
        d += member(b"././@LongLink", b"nine/%d\0" % i, typeflag=b"L")
    d += member(b"nine", payload(400, 71))
    d += member(b"n1", payload(10, 72))
    d += member(b"pax", pax_record(b"path", b"with/size") + pax_record(b"size", b"20"),
                typeflag=b"x")
    d += member(b"sized", payload(20, 73))
    d += member(b"n2", payload(513, 74))
    d += member(b"sparse", payload(100, 75), typeflag=b"S")
    d += member(b"pax", pax_record(b"path", b"first/path") + pax_record(b"mtime", b"1.5") +
                pax_record(b"path", b"pax/named"), typeflag=b"x")
    d += member(b"n3", payload(30, 76))
    d += member(b"pax", b"12 path=oops", typeflag=b"x")                     # does not parse
    d += member(b"badpax", payload(40, 77))
    d += member(b"n4", payload(2, 78))
    return Good("unsupported", d + END, False)


@_once
def tiles():
    """entries of one tile, one tile + 1 and three tiles - 1 bytes next to
    empty and 1-byte entries"""
    d = member(b"one", payload(1, 80)) + member(b"tile", payload(TILE, 81)) + member(b"none")
    d += member(b"tile+1", payload(TILE + 1, 82)) + member(b"x", payload(1, 83))
    d += member(b"3tiles-1", payload(3 * TILE - 1, 84)) + member(b"none2")
    d += member(b"end", payload(17, 85))
    return Good("tiles", d + END, True)


@_once
def nested_big():
    """one entry whose data is an archive of 1100 records: more than 1024
    false candidates"""
    inner = b"".join(member(b"i%04d" % i) for i in range(1100)) + END
    return Good("nested_big", member(b"outer.tar", inner) + member(b"after", payload(9, 90)) + END,
                True)


GOOD = {}
for _f in FORMATS:
    for _fn in (mixed, cut, one_zero, garbage):
        GOOD[_fn.__name__ + "_" + _f] = (_fn, _f)
for _fn in (empty, wg_edges, hand, unsupported, tiles):
    GOOD[_fn.__name__] = (_fn,)
GOOD_NAMES = list(GOOD)
BIG_NAMES = ["many", "straddle_gnu", "straddle_pax", "nested_big"]
GOOD.update({"many": (many,), "straddle_gnu": (straddle, "gnu"), "straddle_pax": (straddle, "pax"),
             "nested_big": (nested_big,)})


def good(name):
    fn = GOOD[name]
    return fn[0](*fn[1:])


def expected(g):
    """-> [(TarInfo, bytes or None)] as tarfile reads the archive"""
    out = []
    with tarfile.open(fileobj=io.BytesIO(g.data), mode="r:") as tf:
        for ti in tf.getmembers():
            # (what has bytes: regular files and types tarfile does not know)
            regular = ti.isreg() or ti.type not in tarfile.SUPPORTED_TYPES
            out.append((ti, tf.extractfile(ti).read() if regular else None))
    return out


# ---- defects ----

@_once
def defects():
    base = mixed("ustar").data
    with tarfile.open(fileobj=io.BytesIO(base), mode="r:") as tf:
        ms = tf.getmembers()
    mid = ms[len(ms) // 2]
    out = []
    d = bytearray(base)
    d[mid.offset + 150] ^= 1
    out.append(Defect("checksum", bytes(d)))
    big = next(m for m in ms if m.size == 4096)
    d = bytearray(base[:big.offset_data + 1024])        # cut inside an entry's data
    out.append(Defect("cut_in_data", bytes(d)))
    d = member(b"ok", payload(10, 95)) + header(b"huge", size=1 << 30) + bytes(4 * BLOCK)
    out.append(Defect("size_past_file", d))
    d = bytearray(base)
    d[mid.offset + 124] = 0xFF                           # a negative base-256 size
    out.append(Defect("size_field", bytes(d)))
    return out


# ---- a .tar.gz ----

@_once
def targz():
    """about 1 MiB of text files, gzip level 6 -> (tar bytes, gz bytes)"""
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=tarfile.PAX_FORMAT) as tf:
        for i in range(30):
            _add(tf, "docs/chapter-%02d.txt" % i, text(20000 + 997 * i, 100 + i))
        _add(tf, "docs/" + "t" * 120 + ".txt", text(5000, 200))
    tar = b.getvalue()
    return tar, gzip.compress(tar, compresslevel=6, mtime=0)
