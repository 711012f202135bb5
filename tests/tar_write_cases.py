"""What the tar writer's tests share: the reference archive - Python's tarfile
in its default (pax) format, regular files with size and an integer mtime set
and everything else at TarInfo's defaults -, names at every edge of the name
rule, and the host arrays of a call."""
import io
import tarfile

import numpy as np

MTIME = 1700000000
BLOCK, RECORD, TILE = 512, 10240, 65536


def tarfile_bytes(names, datas, mtime=MTIME):
    """the archive tarfile writes for these entries (datas: bytes per entry)"""
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.PAX_FORMAT) as t:
        for name, data in zip(names, datas):
            ti = tarfile.TarInfo(name)
            ti.size = len(data)
            ti.mtime = mtime
            t.addfile(ti, io.BytesIO(data))
    return buf.getvalue()


def pax_len(name_bytes):
    """the length of the record "%d path=%s\\n", which counts itself"""
    n = name_bytes + 7
    while len(str(n)) + name_bytes + 7 != n:
        n += 1
    return n


def name_for_pax_len(n):
    """an ASCII name of more than 100 characters whose pax record is n bytes
    long, or None where no name gives that length"""
    length = n - 7 - len(str(n))
    return "p" * length if length > 100 and pax_len(length) == n else None


def edge_names():
    """names on every side of the name rule, all different"""
    names = ["a", "b" * 99, "c" * 100, "d" * 101,
             "e" * 98 + "é",                        # 100 bytes, one of them not ASCII
             "é€" * 60,                        # 120 characters of 2 and 3 bytes
             "\U0001F600" + "f" * 120 + "é",        # a 4-byte character in front
             "g" * 600,                                  # two blocks of pax data
             "h" * 65535]
    # the record's length on each side of the 99 -> 100 and 999 -> 1000 steps
    # of its decimal: 100 and 1000 themselves are no length, and a name needs
    # more than 100 characters (or a byte >= 0x80) to have a record at all
    assert name_for_pax_len(100) is None and name_for_pax_len(1000) is None
    for n in (999, 1001, 1002, 9999, 10001):
        names.append(name_for_pax_len(n))
    for nbytes, want in ((90, 99), (91, 101)):          # with a non-ASCII byte: short names
        names.append("q" * (nbytes - 2) + "é")
        assert pax_len(nbytes) == want
    assert all(names) and len(set(names)) == len(names)
    return names


def call_arrays(names, sizes, offsets=None):
    """(blob, name_offsets, in_offsets, in_nbytes) as numpy arrays; offsets
    default to the entries back to back"""
    raw = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in names]
    offs = np.zeros(len(raw) + 1, dtype=np.uint64)
    if raw:
        offs[1:] = np.cumsum([len(x) for x in raw], dtype=np.uint64)
    blob = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)
    inn = np.asarray(sizes, dtype=np.uint64).reshape(-1)
    if offsets is None:
        ino = np.zeros(len(raw), dtype=np.uint64)
        if len(raw) > 1:
            ino[1:] = np.cumsum(inn[:-1], dtype=np.uint64)
    else:
        ino = np.asarray(offsets, dtype=np.uint64).reshape(-1)
    return blob, offs, ino, inn


def payload(k, n):
    """entry k's n bytes: text-like, different per entry"""
    rng = np.random.default_rng(1000 + k)
    return bytes(rng.integers(32, 127, size=n, dtype=np.uint8))
