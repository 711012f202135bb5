"""BGZF files read on the GPU (libdeflate_amd_bgzf_decompress_batch,
_index_batch, _read_batch and the host call).  No tolerance anywhere: decoded
bytes equal gzip.decompress(file), index pairs equal the offsets recorded
while the file was built (tests/bgzf_files.py), result words equal what each
case states.  Every file goes through the parallel finder and through the
serial walk (LDA_BGZF_SERIAL)."""
import contextlib
import gzip
import os
import random
import struct

import numpy as np
import pytest

from libdeflate_amd import binding
from tests import bgzf_files, bgzf_walk, datagen

pytestmark = pytest.mark.gpu

B = 65280
SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE, MORE = 0, 1, 2, 3, 16
HAS_EOF = 1


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec():
    from libdeflate_amd import api
    d = api.Decompressor()
    yield d
    d.close()


_comps = {}


def _comp(level):
    from libdeflate_amd import api
    if level not in _comps:
        _comps[level] = api.Compressor(level)
    return _comps[level]


@contextlib.contextmanager
def _serial_walk():
    """the finder's serial path (the switch is read through reload_env)"""
    os.environ["LDA_BGZF_SERIAL"] = "1"
    binding.reload_env()
    try:
        yield
    finally:
        os.environ.pop("LDA_BGZF_SERIAL", None)
        binding.reload_env()


def _up(torch, data):
    return torch.frombuffer(bytearray(data) + bytearray(16), dtype=torch.uint8).cuda()


def _read(torch, dec, data, max_members, out_avail, index=True, canary=64, decode=True):
    """-> (result words, output as numpy (out_avail + canary bytes, 0xA5
    where nothing was written), index rows or None)"""
    d_in = _up(torch, data)
    out = torch.full((out_avail + canary,), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((2 * (max_members + 1),), -1, dtype=torch.int64, device="cuda") \
        if index else None
    if decode:
        dec.decompress_bgzf_batch(d_in, max_members, out, res, index=idx, in_nbytes=len(data),
                                  out_avail=out_avail)
    else:
        dec.index_bgzf_batch(d_in, max_members, res, index=idx, in_nbytes=len(data))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert not (host[out_avail:] != 0xA5).any(), "bytes written past out_avail"
    words = [int(x) for x in res.cpu().tolist()]
    rows = idx.cpu().numpy().astype(np.uint64).reshape(-1, 2) if index else None
    return words, host, rows


def _both_paths(torch, dec, data, max_members, out_avail, **kw):
    """the parallel finder and the serial walk must agree on everything"""
    a = _read(torch, dec, data, max_members, out_avail, **kw)
    with _serial_walk():
        b = _read(torch, dec, data, max_members, out_avail, **kw)
    assert a[0] == b[0], (a[0], b[0])
    assert np.array_equal(a[1], b[1])
    if a[2] is not None and a[0][0] in (SUCCESS, INSUFFICIENT_SPACE):
        m = a[0][1]
        assert np.array_equal(a[2][:m + 1], b[2][:m + 1])
    return a


def _check_file(torch, dec, f, max_members=None):
    """a good file: bytes, words, index - through both finders"""
    mm = f.m + 1 if max_members is None else max_members
    n = len(f.plain)
    words, host, rows = _both_paths(torch, dec, f.data, max(mm, 1), n)
    assert words == [SUCCESS, f.m, len(f.data), n, HAS_EOF if f.has_eof else 0], f.name
    assert host[:n].tobytes() == f.plain, f.name
    assert np.array_equal(rows[:f.m + 1], f.rows()), f.name
    return words, host, rows


_base = {}


def _own_data(n, seed):
    if seed not in _base:
        _base[seed] = b"".join(datagen.chunk(i, 65536, seed) for i in range(64))
    b = _base[seed]
    return (b * (n // len(b) + 1))[:n]


def _own_file(torch, level, data, eof=True):
    """our own writer -> (file bytes, its index rows)"""
    c = _comp(level)
    n, m = len(data), -(-len(data) // B)
    out = torch.zeros(c.bgzf_bound(n) + 64, dtype=torch.uint8, device="cuda")
    nb = torch.zeros(1, dtype=torch.int64, device="cuda")
    idx = torch.zeros(2 * (m + 1), dtype=torch.int64, device="cuda")
    c.compress_bgzf_batch(_up(torch, data), out, nb, index=idx, eof=eof, in_nbytes=n,
                          out_avail=c.bgzf_bound(n))
    torch.cuda.synchronize()
    size = int(nb.item())
    return out[:size].cpu().numpy().tobytes(), \
        idx.cpu().numpy().astype(np.uint64).reshape(m + 1, 2)


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("n", [0, 1, 65279, 65280, 65281, 5 * 65280 + 7, -4])
def test_round_trip_of_our_own_files(torch, dec, n, level):
    """result = (0, m + 1, len(file), n, HAS_EOF); index pairs 0..m are the
    compress call's, the closing pair is right.  n = -4: four members per CU"""
    if n < 0:
        n = -n * torch.cuda.get_device_properties(0).multi_processor_count * B - 1000
    data = _own_data(n, 0xB62F1000 + level)
    f, crow = _own_file(torch, level, data)
    m = -(-n // B)
    words, host, rows = _both_paths(torch, dec, f, m + 1, n)
    assert words == [SUCCESS, m + 1, len(f), n, HAS_EOF]
    assert host[:n].tobytes() == data
    assert np.array_equal(rows[:m + 1], crow)
    assert [int(x) for x in rows[m + 1]] == [len(f), n]
    if n <= 5 * B + 7:
        assert gzip.decompress(f) == data
        r, got, nm, fl, hrows = dec.decompress_bgzf(f, n, index=True)
        assert (r, got, nm, fl) == (SUCCESS, data, m + 1, HAS_EOF)
        assert np.array_equal(hrows, rows[:m + 2])


def test_no_eof_file_has_the_flag_clear(torch, dec):
    data = _own_data(3 * B + 17, 0xB62F1010)
    f, crow = _own_file(torch, 6, data, eof=False)
    words, host, rows = _both_paths(torch, dec, f, 4, len(data))
    assert words == [SUCCESS, 4, len(f), len(data), 0]
    assert host[:len(data)].tobytes() == data
    assert np.array_equal(rows[:5], crow)
    assert dec.decompress_bgzf(f, len(data))[2:] == (4, 0)


@pytest.mark.parametrize("f", bgzf_files.all_files(), ids=lambda f: f.name)
def test_files_not_written_by_us(torch, dec, f):
    """zlib at levels 0 / 1 / 9, members cut at random sizes, `cat` of two
    files, ISIZE 65 536, MTIME / OS set, and the adversarial files (a) - (e):
    parallel finder and serial walk, same index"""
    _check_file(torch, dec, f)
    r, got, nm, fl, rows = dec.decompress_bgzf(f.data, len(f.plain), index=True)
    assert (r, got, nm, fl) == (SUCCESS, f.plain, f.m, HAS_EOF if f.has_eof else 0)
    assert np.array_equal(rows, f.rows())


def test_overflowing_candidates_fall_back_to_the_walk_and_agree(torch, dec):
    """(e): with max_members = m + 1 the candidates overflow their space (the
    walk runs inside the normal call), with 4000 they fit and the parallel
    chain crosses several blocks of candidates"""
    f, false = bgzf_files.adversarial("e")
    assert f.m + false > 4 * (f.m + 1) + 1024
    a = _check_file(torch, dec, f)
    b = _check_file(torch, dec, f, max_members=4000)
    assert a[0] == b[0] and np.array_equal(a[2][:f.m + 1], b[2][:f.m + 1])


def test_index_call_gives_the_same_index_and_words(torch, dec):
    for f in (bgzf_files.cut_file(400000, 21), bgzf_files.cat_file(22),
              bgzf_files.adversarial("c")[0], bgzf_files.File([], False, "empty")):
        n = len(f.plain)
        full = _read(torch, dec, f.data, f.m + 3, n)
        only = _both_paths(torch, dec, f.data, f.m + 3, n, decode=False)
        assert only[0] == full[0] == [SUCCESS, f.m, len(f.data), n, HAS_EOF if f.has_eof else 0]
        assert np.array_equal(only[2][:f.m + 1], full[2][:f.m + 1])
        assert not (only[1] != 0xA5).any()      # nothing is decoded


def test_space_rule_and_max_members(torch, dec):
    f = bgzf_files.cut_file(500000, 23, lo=3000, hi=40000)
    n = len(f.plain)
    assert _check_file(torch, dec, f, max_members=f.m)[0][1] == f.m     # exact
    _check_file(torch, dec, f, max_members=16 * f.m)
    # one byte short: decided before the decode, the whole output untouched
    words, host, rows = _both_paths(torch, dec, f.data, f.m, n - 1)
    assert words == [INSUFFICIENT_SPACE, f.m, len(f.data), n, 0]
    assert not (host != 0xA5).any()
    assert np.array_equal(rows[:f.m + 1], f.rows())     # the index is still there
    # one member too many for max_members: the count is the file's
    words, host, _ = _both_paths(torch, dec, f.data, f.m - 1, n)
    assert words == [MORE, f.m, 0, 0, 0]
    assert not (host != 0xA5).any()
    # precedence: MORE_MEMBERS before INSUFFICIENT_SPACE
    assert _both_paths(torch, dec, f.data, f.m - 1, 10)[0][0] == MORE
    # the host call: the same rule
    assert dec.decompress_bgzf(f.data, n - 1)[0] == INSUFFICIENT_SPACE
    assert dec.decompress_bgzf(f.data, n, index=True, index_avail=2 * f.m)[0] == MORE


def _damage(f):
    """-> [(name, file bytes, stated result, decided before the decode)]"""
    b = f.data
    k = 2
    off, size, isize = f.members[k]
    end = off + size

    def edit(at, new):
        x = bytearray(b)
        x[at:at + len(new)] = new
        return bytes(x)
    crc = edit(end - 8, bytes([b[end - 8] ^ 0x55]))
    # a deflate body that ends one byte early: a pad byte before the trailer
    mem = b[off:end]
    padded = mem[:16] + struct.pack("<H", size) + mem[18:-8] + b"\0" + mem[-8:]
    early = b[:off] + padded + b[end:]
    return [
        ("bsize", edit(off + 16, bytes([b[off + 16] ^ 1])), BAD_DATA, True),
        ("cut", b[:end - 100], BAD_DATA, True),
        ("junk", b + b"junk" * 9, BAD_DATA, True),
        ("xlen7", edit(off + 10, b"\x07"), BAD_DATA, True),
        ("isize-huge", edit(end - 4, struct.pack("<I", 0x7FFFFFFF)), BAD_DATA, True),
        ("crc", crc, BAD_DATA, False),
        ("isize+1", edit(end - 4, struct.pack("<I", isize + 1)), SHORT_OUTPUT, False),
        ("isize-1", edit(end - 4, struct.pack("<I", isize - 1)), INSUFFICIENT_SPACE, False),
        ("early-end", early, BAD_DATA, False),
    ]


def test_damaged_files_end_in_their_stated_results(torch, dec):
    """input validation that ends in result codes: the canary past out_avail
    stays intact (checked in _read), nothing is decoded where the verdict
    precedes the decode, and the host call returns the same value"""
    f = bgzf_files.cut_file(300000, 24, lo=5000, hi=40000)
    avail = len(f.plain) + 64
    for name, data, want, early in _damage(f):
        words, host, _ = _both_paths(torch, dec, data, f.m + 2, avail)
        assert words[0] == want, (name, words)
        if early:
            assert words == [BAD_DATA, 0, 0, 0, 0], (name, words)
            assert not (host != 0xA5).any(), name
        else:
            # the members in front of the damaged one are decoded, in place
            u = int(f.rows()[2][1])
            assert host[:u].tobytes() == f.plain[:u], name
        assert dec.decompress_bgzf(data, avail)[0] == want, name


@pytest.fixture(scope="module")
def ranged():
    """a file of some hundred members, two of them empty"""
    rng = random.Random(0xB62F2000)
    data = bgzf_files.text(3_000_000, 25)
    pieces, k = [], 0
    while k < len(data):
        size = rng.randrange(1000, 20001)
        pieces.append(bgzf_files.piece(data[k:k + size], rng.choice([0, 1, 6])))
        if len(pieces) in (40, 41):
            pieces.append((bgzf_walk.EOF_MEMBER, b""))
        k += size
    f = bgzf_files.File(pieces, True, "ranged")
    assert 200 < f.m < 1000
    return f


def _ranges(torch, dec, f, ranges, data=None, voffsets=False, avail=None):
    """-> (per-range results, per-range bytes)"""
    blob = f.data if data is None else data
    plain = [(int(b), int(n)) for b, n in ranges]
    arg = [(f.voffset(b), f.voffset(b + n)) for b, n in plain] if voffsets else plain
    need = sum(n for _, n in plain)
    avail = need if avail is None else avail
    out = torch.full((avail + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.full((max(len(plain), 1),), -1, dtype=torch.int32, device="cuda")
    dec.read_bgzf_batch(_up(torch, blob), f.rows(), np.array(arg, dtype=np.uint64).reshape(-1, 2),
                        out, res, voffsets=voffsets, in_nbytes=len(blob), out_avail=avail)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert not (host[need:] != 0xA5).any(), "bytes written past the ranges"
    got, at = [], 0
    for _, n in plain:
        got.append(host[at:at + n].tobytes())
        at += n
    return [int(x) for x in res.cpu().tolist()][:len(plain)], got


def _range_cases(f):
    rows = f.rows()
    u = [int(x) for x in rows[:, 1]]
    total = len(f.plain)
    rng = random.Random(0xB62F2001)
    cases = [
        (u[5] + 10, 100),                       # inside one member
        (u[7], u[8] - u[7]),                    # exactly one member
        (u[7] + 1, u[9] - u[7] - 1),            # ends exactly on a boundary
        (u[10], u[12] - u[10] + 5),             # begins on one
        (u[30] + 17, u[60] - u[30]),            # many members, the empty ones among them
        (u[20], 0), (total, 0), (0, 0),         # empty
        (u[30], u[33] - u[30]), (u[31] + 5, u[34] - u[31]),     # overlapping each other
        (0, total),                             # the whole file
        (total - 1, 1), (0, 1),
    ]
    many = []
    for _ in range(1000):
        n = rng.randrange(0, 50001)
        many.append((rng.randrange(0, total - n + 1), n))
    return cases, many


@pytest.mark.parametrize("voffsets", [False, True], ids=["bytes", "voffsets"])
def test_ranged_reads_against_slices_of_the_plain_bytes(torch, dec, ranged, voffsets):
    f = ranged
    cases, many = _range_cases(f)
    for batch in (cases, many, cases[:1], []):
        res, got = _ranges(torch, dec, f, batch, voffsets=voffsets)
        assert res == [0] * len(batch)
        for (b, n), g in zip(batch, got):
            assert g == f.plain[b:b + n], (b, n)


def test_ranged_reads_fail_exactly_the_ranges_that_touch_a_bad_member(torch, dec, ranged):
    f = ranged
    k = 50
    off, size, isize = f.members[k]
    assert isize
    bad = bytearray(f.data)
    bad[off + size - 8] ^= 0x55     # its CRC
    cases, many = _range_cases(f)
    u0 = int(f.rows()[k][1])
    batch = cases + many[:300] + [(u0 - 1, 1), (u0, 1), (u0 + isize - 1, 1), (u0 + isize, 1)]
    for voffsets in (False, True):
        res, got = _ranges(torch, dec, f, batch, data=bytes(bad), voffsets=voffsets)
        for (b, n), r, g in zip(batch, res, got):
            touches = n > 0 and b < u0 + isize and b + n > u0
            assert r == (BAD_DATA if touches else 0), (b, n, r)
            if not touches:
                assert g == f.plain[b:b + n], (b, n)
        assert res[-4:] == [0, BAD_DATA, BAD_DATA, 0]


def test_both_inflate_mappings_agree_on_a_mixed_file(torch, dec, monkeypatch, ranged):
    a = bgzf_files.cat_file(26)
    b = bgzf_files.adversarial("b")[0]
    members = [(f.data[o:o + s], f.plain[u:u + i]) for f in (a, b, ranged)
               for (o, s, i), u in zip(f.members[:60], f.rows()[:, 1].astype(int))]
    f = bgzf_files.File(members, False, "mixed")
    first = _check_file(torch, dec, f)
    cases = [(0, len(f.plain)), (1000, 200000), (77777, 3)]
    r1 = _ranges(torch, dec, f, cases)
    monkeypatch.setenv("LDA_INFLATE_PAR", "0")
    binding.reload_env()
    second = _check_file(torch, dec, f)
    r2 = _ranges(torch, dec, f, cases)
    assert first[0] == second[0] and np.array_equal(first[1], second[1])
    assert r1 == r2 and r1[1] == [f.plain[b:b + n] for b, n in cases]
