"""CPU-side checks of the BGZF reader: the four calls declared, exported and
bound with the header's constants; arguments and ranges refused before any
device is touched; what the host call decides from the headers alone; the CPU
model of the member finder (tools/models/bgzf_chain.py) against the member
lists recorded while the files were built (tests/bgzf_files.py), adversarial
files included; and the new kernels' compile report."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import bgzf_files, bgzf_walk
from tools.models import bgzf_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
READ_SYMBOLS = ("libdeflate_amd_bgzf_decompress_batch", "libdeflate_amd_bgzf_index_batch",
                "libdeflate_amd_bgzf_read_batch", "libdeflate_amd_bgzf_decompress")
KERNELS = ["lda_bgzf_scan_kernel", "lda_bgzf_jump_kernel", "lda_bgzf_top_kernel",
           "lda_bgzf_members_kernel", "lda_bgzf_walk_kernel", "lda_bgzf_isize_kernel",
           "lda_bgzf_rdesc_kernel", "lda_bgzf_rfinal_kernel", "lda_bgzf_trim_kernel",
           "lda_bgzf_range_kernel"]
BAD_ARG = -2
BAD_DATA, INSUFFICIENT_SPACE, MORE_MEMBERS = 1, 3, 16


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from libdeflate_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    return binding.load()


def _header():
    return open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()


def test_read_symbols_declared_exported_and_bound(lib):
    from libdeflate_amd import binding
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", _header(), re.M))
    assert set(READ_SYMBOLS) <= declared
    assert set(READ_SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(READ_SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    for s in READ_SYMBOLS:
        assert getattr(lib, s).argtypes, s
    assert not binding.MISSING


def test_read_constants_match_the_header():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name):
        return int(re.search(rf"#define {name}\s+(\d+)", hdr).group(1))
    assert define("LIBDEFLATE_AMD_BGZF_MORE_MEMBERS") == binding.BGZF_MORE_MEMBERS == 16
    assert define("LIBDEFLATE_AMD_BGZF_HAS_EOF") == binding.BGZF_HAS_EOF == 1
    assert define("LIBDEFLATE_AMD_BGZF_RESULT_WORDS") == binding.BGZF_RESULT_WORDS == 5
    assert define("LIBDEFLATE_AMD_BGZF_VOFFSETS") == binding.BGZF_VOFFSETS == 2
    # the device side's copies (kernels.h) are the header's
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert int(re.search(r"#define LDA_BR_MORE (\d+)", k).group(1)) == 16
    assert int(re.search(r"#define LDA_BR_HAS_EOF (\d+)", k).group(1)) == 1
    assert int(re.search(r"#define LDA_BR_RESULT_WORDS (\d+)", k).group(1)) == 5
    assert int(re.search(r"#define LDA_BR_JUMP (\d+)", k).group(1)) == bgzf_chain.BLOCK


def _ptr(arr):
    return arr.ctypes.data_as(ctypes.c_void_p)


def test_read_calls_check_their_arguments(lib):
    """Refused before any device is touched: a NULL object or pointer,
    max_members == 0 for a file that has bytes, unknown flags, an index_avail
    that cannot hold one pair."""
    from libdeflate_amd import binding
    buf = (ctypes.c_uint8 * 4096)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    dec, idx = lib.libdeflate_amd_bgzf_decompress_batch, lib.libdeflate_amd_bgzf_index_batch
    read, host = lib.libdeflate_amd_bgzf_read_batch, lib.libdeflate_amd_bgzf_decompress
    assert dec(None, d, 28, 1, d, 64, d, None, None) == BAD_ARG
    assert "NULL" in binding.last_error()
    assert dec(fake, None, 28, 1, d, 64, d, None, None) == BAD_ARG
    assert dec(fake, d, 28, 1, None, 64, d, None, None) == BAD_ARG
    assert dec(fake, d, 28, 1, d, 64, None, None, None) == BAD_ARG
    assert dec(fake, d, 28, 0, d, 64, d, None, None) == BAD_ARG
    assert "max_members" in binding.last_error()
    assert dec(fake, d, 28, 1 << 40, d, 64, d, None, None) == BAD_ARG
    assert idx(None, d, 28, 1, d, None, None) == BAD_ARG
    assert idx(fake, None, 28, 1, d, None, None) == BAD_ARG
    assert idx(fake, d, 28, 1, None, None, None) == BAD_ARG
    assert idx(fake, d, 28, 0, d, None, None) == BAD_ARG
    assert "max_members" in binding.last_error()
    # the ranged read: pointers, flags, an index that is no index
    f = bgzf_files.plain_file(150000, 11)
    rows = f.rows()
    rng = np.array([[0, 10]], dtype=np.uint64)
    n, m = len(f.data), f.m
    args = lambda **kw: [kw.get("obj", fake), d, n, kw.get("index", _ptr(rows)), m,     # noqa: E731
                         1, kw.get("ranges", _ptr(rng)), kw.get("flags", 0),
                         kw.get("out", d), kw.get("avail", 4096), kw.get("res", d), None]
    assert read(*args(obj=None)) == BAD_ARG
    assert read(*args(index=None)) == BAD_ARG
    assert read(*args(ranges=None)) == BAD_ARG
    assert read(*args(out=None)) == BAD_ARG
    assert read(*args(res=None)) == BAD_ARG
    assert "NULL" in binding.last_error()
    assert read(*args(flags=1)) == BAD_ARG and "flags" in binding.last_error()
    assert read(*args(flags=4)) == BAD_ARG
    bad = rows.copy()
    bad[1][0] = bad[0][0] + 20          # a member of 20 bytes
    assert read(*args(index=_ptr(bad))) == BAD_ARG and "index" in binding.last_error()
    bad = rows.copy()
    bad[-1][0] = n + 1                  # ends past the file
    assert read(*args(index=_ptr(bad))) == BAD_ARG
    # the host call
    assert host(None, d, 28, d, 64, None, None, None, 0, None) == BAD_DATA
    assert "NULL" in binding.last_error()
    assert host(fake, None, 28, d, 64, None, None, None, 0, None) == BAD_DATA
    assert host(fake, d, 28, None, 64, None, None, None, 0, None) == BAD_DATA
    assert host(fake, d, 28, d, 64, None, None, d, 1, None) == BAD_DATA
    assert "index_avail" in binding.last_error()


def test_read_batch_checks_its_ranges_on_the_host(lib):
    """host arithmetic on host arrays, before any device work: a range past
    the end, an output that does not fit, a virtual offset whose coffset is
    no member start or whose uoffset lies past the member's data"""
    from libdeflate_amd import binding
    f = bgzf_files.cut_file(300000, 12, lo=5000, hi=30000)
    rows, n, total = f.rows(), len(f.data), len(f.plain)
    d = ctypes.cast((ctypes.c_uint8 * 64)(), ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    read = lib.libdeflate_amd_bgzf_read_batch

    def call(ranges, flags=0, avail=1 << 30):
        r = np.array(ranges, dtype=np.uint64).reshape(-1, 2)
        return read(fake, d, n, _ptr(rows), f.m, len(r), _ptr(r), flags, d, avail, d, None)
    assert call([(total - 5, 6)]) == BAD_ARG and "past the end" in binding.last_error()
    assert call([(total + 1, 0)]) == BAD_ARG
    assert call([(0, 10), (1 << 63, 1 << 63)]) == BAD_ARG
    assert call([(0, 100), (50, 100)], avail=199) == BAD_ARG
    assert "out_avail" in binding.last_error()
    v = f.voffset
    assert call([(v(0) + (1 << 16), v(100))], flags=2) == BAD_ARG   # coffset 1
    assert "virtual offset" in binding.last_error()
    assert call([(v(0), (int(rows[1][0]) + 3) << 16)], flags=2) == BAD_ARG
    isize0 = f.members[0][2]
    assert call([(v(0), int(rows[0][0]) << 16 | (isize0 + 1))], flags=2) == BAD_ARG
    assert call([(v(500), v(100))], flags=2) == BAD_ARG             # end before begin
    # no ranges: nothing to do, and nothing is touched
    assert read(fake, d, n, _ptr(rows), f.m, 0, None, 0, None, 0, None, None) == 0


def _damaged(f):
    """(name, bytes) of files whose chain or headers are broken: BAD_DATA
    before anything is decoded"""
    b = f.data
    off1 = f.members[1][0]
    x7 = bytearray(b)
    x7[off1 + 10] = 7
    bs = bytearray(b)
    bs[off1 + 16] ^= 1
    big = bytearray(b)
    end1 = off1 + f.members[1][1]
    big[end1 - 4:end1] = struct.pack("<I", 0x7FFFFFFF)
    return [("bsize", bytes(bs)), ("cut", b[:end1 - 100]), ("junk", b + b"junk" * 9),
            ("xlen7", bytes(x7)), ("isize", bytes(big)), ("short", b[:20]),
            ("gzip", __import__("gzip").compress(b"plain gzip is not BGZF"))]


def test_host_call_decides_from_the_headers_before_any_device_work(lib):
    """a stand-in object again: BAD_DATA for a broken chain / header / ISIZE,
    then MORE_MEMBERS (the index does not fit), then INSUFFICIENT_SPACE"""
    f = bgzf_files.plain_file(200000, 13)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    host = lib.libdeflate_amd_bgzf_decompress
    out = np.zeros(8, dtype=np.uint8)
    idx = np.zeros(2 * (f.m + 1), dtype=np.uint64)
    nm = ctypes.c_size_t(0)
    for name, b in _damaged(f):
        a = np.frombuffer(b, dtype=np.uint8)
        assert host(fake, _ptr(a), len(b), _ptr(out), 1 << 30, None, None, None, 0,
                    None) == BAD_DATA, name
    a = np.frombuffer(f.data, dtype=np.uint8)
    # BAD_DATA comes before the two others, MORE_MEMBERS before the space
    b = np.frombuffer(_damaged(f)[0][1], dtype=np.uint8)
    assert host(fake, _ptr(b), b.size, _ptr(out), 8, None, None, _ptr(idx), 2, None) == BAD_DATA
    assert host(fake, _ptr(a), a.size, _ptr(out), 8, None, ctypes.byref(nm), _ptr(idx),
                2 * f.m, None) == MORE_MEMBERS
    assert nm.value == f.m
    assert host(fake, _ptr(a), a.size, _ptr(out), len(f.plain) - 1, None, None, _ptr(idx),
                idx.size, None) == INSUFFICIENT_SPACE
    # an empty file: 0 members, SUCCESS, the closing pair alone
    fl = ctypes.c_uint32(7)
    idx[:2] = 9
    assert host(fake, None, 0, None, 0, None, ctypes.byref(nm), _ptr(idx), 2,
                ctypes.byref(fl)) == 0
    assert (nm.value, fl.value, list(idx[:2])) == (0, 0, [0, 0])


# ---- the CPU model of the finder ----

def _want(f, mm):
    return [(o, s) for o, s, _ in f.members][:mm]


@pytest.mark.parametrize("f", bgzf_files.all_files(), ids=lambda f: f.name)
def test_model_finds_the_recorded_members(f):
    """both paths of the model, on every file, with max_members exact, short
    by one (the count is still the file's) and generous; blocks of 4
    candidates put every file's chain across many blocks"""
    for mm in (f.m + 1, max(f.m - 1, 1), 16 * f.m + 16):
        runs = [bgzf_chain.find(f.data, mm, block=blk) for blk in (bgzf_chain.BLOCK, 4, 1)]
        runs.append(bgzf_chain.find(f.data, mm, force_serial=True))
        for ok, count, members, _ in runs:
            assert ok and count == f.m and members == _want(f, mm), (f.name, mm)


def test_model_on_the_adversarial_files():
    """the false candidates are there, behave as described, and are not
    members; (e) overflows the candidate space of a small max_members and
    goes through the parallel path with a large one - same members"""
    for kind in "abcd":
        f, false = bgzf_files.adversarial(kind)
        cands = bgzf_chain.candidates(f.data)
        starts = {o for o, _, _ in f.members}
        extra = [c for c in cands if c[0] not in starts]
        assert len(extra) == false and len(cands) == f.m + false, kind
        ends = {o + s for o, s in extra}
        if kind == "a":     # a real member in a payload: its end is nowhere
            assert not ends & (starts | {c[0] for c in cands} | {len(f.data)})
        if kind == "b":     # ends exactly on the next true member
            assert ends <= starts
        if kind == "c":     # the first points at the second
            assert extra[0][0] + extra[0][1] == extra[1][0]
        if kind == "d":     # ends exactly at the end of the file
            assert ends == {len(f.data)}
        assert bgzf_chain.find(f.data, f.m)[3] == "parallel"
    f, false = bgzf_files.adversarial("e")
    cands = bgzf_chain.candidates(f.data)
    assert len(cands) >= f.m + false > bgzf_chain.cand_cap(len(f.data), f.m + 1)
    small = bgzf_chain.find(f.data, f.m + 1)
    large = bgzf_chain.find(f.data, 4000)
    assert (small[3], large[3]) == ("serial", "parallel")
    assert small[:3] == large[:3] == (True, f.m, _want(f, f.m))
    # two headers cannot stand closer than 16 bytes: the bound of the space
    assert all(b[0] - a[0] >= 16 for a, b in zip(cands, cands[1:]))
    assert len(cands) <= len(f.data) // 16 + 1


def test_model_refuses_broken_chains_on_both_paths():
    f = bgzf_files.adversarial("b")[0]
    for name, b in _damaged(f)[:4] + _damaged(f)[5:]:
        for kw in ({}, {"block": 4}, {"force_serial": True}):
            assert bgzf_chain.find(b, 64, **kw)[0] is False, (name, kw)
    # a chain that does not start at offset 0
    assert bgzf_chain.find(b"\0" + f.data, 64)[0] is False
    assert bgzf_chain.find(b"\0" + f.data, 64, force_serial=True)[0] is False
    # the walker agrees where it applies (single-writer files)
    g = bgzf_files.plain_file(200000, 14)
    assert [(x.offset, x.size) for x in bgzf_walk.walk(g.data)[0]] == _want(g, g.m - 1)


# ---- the kernels as the compiler reports them ----

def test_read_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "bgzf_read_kernels.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == KERNELS
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", rep)]
    sspills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", rep)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", rep)]
    assert spills == [0] * len(KERNELS), spills
    assert sspills == [0] * len(KERNELS), sspills
    assert scratch == [0] * len(KERNELS), scratch
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert [x for x in KERNELS if f"\n{x}(" not in k] == []


def test_gzi_from_the_readers_index():
    from libdeflate_amd import api
    f = bgzf_files.plain_file(3 * 65280 + 1, 15)
    rows = f.rows()         # 4 data members, the EOF member, the closing row
    blob = api.bgzf_index_gzi(rows)
    assert np.array_equal(api.bgzf_gzi_parse(blob), rows[1:4])
    flat = np.concatenate([rows.reshape(-1), np.zeros(10, dtype=np.uint64)])
    assert api.bgzf_index_gzi(flat, members=f.m) == blob
    g = bgzf_files.plain_file(3 * 65280 + 1, 15, eof=False)
    assert api.bgzf_index_gzi(g.rows()) == blob
