"""CPU-side checks of the ZIP writer: the two calls declared, exported and
bound with the header's constants; every refusal that comes before any device
work, with its reason; libdeflate_amd_zip_compress_bound against the CPU model
(tools/models/zip_write.py), the three ZIP64 triggers included; the model's
archives against Python's zipfile and against the reader's model
(tools/models/zip_walk.py); and the new kernels' compile report."""
import ctypes
import io
import os
import re
import struct
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

from tools.models import zip_walk, zip_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_zip_compress_bound", "libdeflate_amd_zip_compress_batch")
KERNELS = ["lda_zipw_entry_kernel", "lda_zipw_place_kernel", "lda_zipw_copy_kernel",
           "lda_zipw_final_kernel"]
BAD_ARG = -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from libdeflate_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    return binding.load()


def _header():
    return open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()


def _u64(*v):
    a = np.array(v, dtype=np.uint64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_declared_exported_and_bound(lib):
    from libdeflate_amd import api, binding
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", _header(), re.M))
    assert set(SYMBOLS) <= declared
    assert set(SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    assert len(lib.libdeflate_amd_zip_compress_bound.argtypes) == 4
    assert len(lib.libdeflate_amd_zip_compress_batch.argtypes) == 15
    assert not binding.MISSING
    for name in ("zip_bound", "compress_zip_batch"):
        assert callable(getattr(api.Compressor, name))


def test_constants_match_the_header():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name):
        return int(re.search(rf"#define {name}\s+(\d+)", hdr).group(1))
    assert define("LIBDEFLATE_AMD_ZIP_STORE") == binding.ZIP_STORE == zip_write.STORE == 1
    assert define("LIBDEFLATE_AMD_ZIP_FORCE_ZIP64") == binding.ZIP_FORCE_ZIP64 == \
        zip_write.FORCE_ZIP64 == 2
    assert define("LIBDEFLATE_AMD_ZIPW_RESULT_WORDS") == binding.ZIPW_RESULT_WORDS == \
        zip_write.RESULT_WORDS == 4
    assert define("LIBDEFLATE_AMD_ZIP_WORDS") == zip_write.WORDS == 8
    plan = open(os.path.join(CSRC, "zip_write_plan.h")).read()
    assert re.search(r"ZIPW_STORE = 1,", plan) and re.search(r"ZIPW_FORCE_ZIP64 = 2,", plan)
    assert re.search(r"ZIPW_RESULT_WORDS = 4,", plan)


def test_the_call_checks_its_arguments(lib):
    """Refused before any device is touched, with a reason: a NULL object or
    pointer (d_in only with in_avail != 0, the host arrays only with
    n_entries != 0, d_index never), unknown flags, n_entries above 2^28, a
    name of 0 or more than 65 535 bytes, decreasing name_offsets, an entry of
    4 GiB or more, an entry outside in_avail, out_avail below the directory
    and end records alone."""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    call = lib.libdeflate_amd_zip_compress_batch
    names = ctypes.cast(ctypes.create_string_buffer(b"x" * 70000), ctypes.c_void_p)
    _a, noff = _u64(0, 1, 3)
    _b, ioff = _u64(0, 100)
    _c, inn = _u64(100, 50)
    big = 1 << 20

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
        assert "zip_compress_batch" in binding.last_error()
    refused(call(None, 2, names, noff, d, 150, ioff, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, None, noff, d, 150, ioff, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, None, d, 150, ioff, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, noff, None, 150, ioff, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, noff, d, 150, None, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, noff, d, 150, ioff, None, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, noff, d, 150, ioff, inn, None, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, noff, d, 150, ioff, inn, d, big, None, None, 0, 0, None), "NULL")
    refused(call(None, 0, None, None, None, 0, None, None, d, big, d, None, 0, 0, None), "NULL")
    for flags in (4, 8, 0x80000000, 7):
        refused(call(fake, 2, names, noff, d, 150, ioff, inn, d, big, d, None, 0, flags, None),
                "flags")
    refused(call(fake, (1 << 28) + 1, names, noff, d, 150, ioff, inn, d, big, d, None, 0, 0, None),
            "n_entries")
    _d, bad = _u64(0, 0, 3)
    refused(call(fake, 2, names, bad, d, 150, ioff, inn, d, big, d, None, 0, 0, None),
            "entry 0: an empty name")
    _d, bad = _u64(0, 3, 3)
    refused(call(fake, 2, names, bad, d, 150, ioff, inn, d, big, d, None, 0, 0, None),
            "entry 1: an empty name")
    _d, bad = _u64(0, 3, 2)
    refused(call(fake, 2, names, bad, d, 150, ioff, inn, d, big, d, None, 0, 0, None),
            "name_offsets decrease")
    _d, bad = _u64(0, 1, 65537)
    refused(call(fake, 2, names, bad, d, 150, ioff, inn, d, big, d, None, 0, 0, None), "65535")
    _d, bad = _u64(100, 1 << 32)
    refused(call(fake, 2, names, noff, d, 1 << 40, ioff, bad, d, 1 << 40, d, None, 0, 0, None),
            "4 GiB")
    refused(call(fake, 2, names, noff, d, 149, ioff, inn, d, big, d, None, 0, 0, None), "in_avail")
    _d, bad = _u64(0, 151)
    refused(call(fake, 2, names, noff, d, 150, bad, inn, d, big, d, None, 0, 0, None),
            "entry 1: its bytes do not lie inside in_avail")
    _d, bad = _u64(0, (1 << 64) - 10)
    refused(call(fake, 2, names, noff, d, 150, bad, inn, d, big, d, None, 0, 0, None), "in_avail")
    # the directory and end records alone: 2 x 46 + 3 bytes of names + 22
    refused(call(fake, 2, names, noff, d, 150, ioff, inn, d, 116, d, None, 0, 0, None), "out_avail")
    # ... and in ZIP64 mode 2 x 12 + 76 more
    refused(call(fake, 2, names, noff, d, 150, ioff, inn, d, 216, d, None, 0, 2, None), "out_avail")
    refused(call(fake, 0, None, None, None, 0, None, None, d, 21, d, None, 0, 0, None), "out_avail")


def _lib_bound(lib, name_lens, sizes, flags):
    offs = np.zeros(len(sizes) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.array(name_lens, dtype=np.uint64), dtype=np.uint64)
    offs += np.uint64(1000)     # only the differences count
    sz = np.array(sizes, dtype=np.uint64)
    return lib.libdeflate_amd_zip_compress_bound(len(sizes), offs.ctypes.data_as(ctypes.c_void_p),
                                                 sz.ctypes.data_as(ctypes.c_void_p), flags)


def test_bound_is_the_models_and_zip64_has_three_triggers(lib):
    rng = np.random.default_rng(0x21B)
    assert lib.libdeflate_amd_zip_compress_bound(0, None, None, 0) == 22
    assert lib.libdeflate_amd_zip_compress_bound(0, None, None, 2) == 98
    assert lib.libdeflate_amd_zip_compress_bound(0, None, None, 1) == 22
    for case in range(40):
        n = int(rng.integers(1, 50))
        nl = [int(x) for x in rng.integers(1, 65536, n)]
        hi = (0, 1000, 1 << 20, 1 << 32, 1 << 40)[case % 5]
        sz = [int(x) for x in rng.integers(0, hi + 1, n)]
        for flags in (0, 1, 2, 3):
            want, z, cd, end = zip_write.bound(nl, sz, flags)
            assert _lib_bound(lib, nl, sz, flags) == want
            assert z == bool(flags & 2) or want >= 0xFFFFFFFF
            assert want == sum(30 + a + b for a, b in zip(nl, sz)) + \
                sum(46 + a + 12 * z for a in nl) + 22 + 76 * z
    # the flag
    assert zip_write.bound([1], [0], 2)[:2] == (30 + 1 + 46 + 1 + 12 + 22 + 76, True)
    assert _lib_bound(lib, [1], [0], 2) == 188
    # the count
    for n, z in ((65534, False), (65535, True), (65536, True)):
        want = n * (30 + 1 + 46 + 1 + 12 * z) + 22 + 76 * z
        assert zip_write.bound([1] * n, [0] * n)[:2] == (want, z)
        assert _lib_bound(lib, [1] * n, [0] * n, 0) == want
    # the plain sum reaching 0xFFFFFFFF
    fixed = 2 * (30 + 5 + 46 + 5) + 22
    for total, z in ((0xFFFFFFFE, False), (0xFFFFFFFF, True), (0x100000000, True), (1 << 40, True)):
        sz = [0xFFFFFFF0 // 2, total - fixed - 0xFFFFFFF0 // 2]
        want = total + (2 * 12 + 76) * z
        assert zip_write.bound([5, 5], sz)[:2] == (want, z)
        assert _lib_bound(lib, [5, 5], sz, 0) == want


# ---- the model against zipfile and against the reader's model ----

def _deflate(raw, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(raw) + c.flush()


def _check_model(names, entries, flags=0, dt=0, streams=None):
    """the archive as zipfile reads it - names, CRCs, sizes, header_offset,
    bytes, testzip() - and as the reader's model indexes it: its rows are the
    writer's rows"""
    if streams is None:
        streams = [_deflate(x) for x in entries]
    a = zip_write.build(names, entries, streams, dt, flags)
    n = len(names)
    want_bound, z, cd, end = zip_write.bound([len(x) for x in names], [len(x) for x in entries],
                                             flags)
    assert a.zip64 == z and a.words[0] == 0 and a.words[1] == len(a.data) <= want_bound
    assert a.words[2] + cd + end == len(a.data)
    zfile = zipfile.ZipFile(io.BytesIO(a.data))
    assert zfile.testzip() is None
    infos = zfile.infolist()
    assert len(infos) == n and zfile.comment == b""
    deflated = 0
    for zi, name, raw, s, row in zip(infos, names, entries, streams, a.rows):
        use = not (flags & 1) and len(s) < len(raw)
        deflated += use
        utf8 = any(b >= 0x80 for b in name)
        assert zi.orig_filename == name.decode("utf-8" if utf8 else "cp437")
        assert zi.flag_bits == (0x800 if utf8 else 0)
        assert zi.compress_type == (8 if use else 0)
        assert (zi.CRC, zi.file_size) == (zlib.crc32(raw), len(raw))
        assert zi.compress_size == (len(s) if use else len(raw))
        assert zi.extract_version == zi.create_version == (45 if z else 20)
        assert zi.create_system == 0 and zi.external_attr == 0 and zi.internal_attr == 0
        assert zi.comment == b""
        assert zi.extra == (struct.pack("<HHQ", 1, 8, zi.header_offset) if z else b"")
        assert zi.date_time == ((1980, 1, 1, 0, 0, 0) if dt == 0 else
                                ((dt >> 25) + 1980, dt >> 21 & 15, dt >> 16 & 31,
                                 dt >> 11 & 31, dt >> 5 & 63, (dt & 31) * 2))
        assert zi.header_offset + 30 + len(name) == row[4]
        assert zfile.open(zi).read() == raw
    assert a.words[3] == deflated
    # entries lie back to back from offset 0, the directory follows directly
    at = 0
    for zi, name in zip(infos, names):
        assert zi.header_offset == at
        at += 30 + len(name) + zi.compress_size
    assert at == a.words[2]
    r = zip_walk.read(a.data, max(n, 1))
    assert r.words == [0, n, a.words[2], sum(len(x) for x in entries), 1 if z else 0]
    assert r.rows == a.rows and r.results == [0] * n and r.plain == list(entries)
    return a


def _mixed():
    rng = np.random.default_rng(0x21C)
    text = (b"the quick brown fox jumps over the lazy dog; " * 3000)
    entries = [b"", b"a", text[:100], text[:70000], rng.bytes(1000), bytes(5000), text[:4097]]
    names = [b"e", b"ab", b"dir/fifteen.txt", b"dir/sixteen_.txt", b"dir/seventeen.txt",
             b"n" * 255, "déjà vu/漢字.txt".encode("utf-8")]
    return names, entries


def test_model_plain_archive():
    names, entries = _mixed()
    a = _check_model(names, entries)
    assert not a.zip64 and a.words[3] == 4      # empty, 1 byte and random are stored
    assert a.data[-22:-18] == b"PK\5\6"
    b = _check_model(names, entries, dt=(2024 - 1980) << 25 | 2 << 21 | 29 << 16 | 13 << 11 | 7 << 5 | 9)
    assert len(b.data) == len(a.data) and b.data != a.data


def test_model_store_flag_and_missing_streams():
    names, entries = _mixed()
    a = _check_model(names, entries, flags=1)
    assert a.words[3] == 0 and len(a.data) == zip_write.bound([len(x) for x in names],
                                                              [len(x) for x in entries])[0]
    b = zip_write.build(names, entries, [None] * len(names))
    assert b.data == a.data and b.words == a.words and b.rows == a.rows
    # a stream as long as the entry does not win
    c = zip_write.build([b"x"], [b"abcd"], [b"wxyz"])
    assert c.words[3] == 0 and c.data[30 + 1:30 + 5] == b"abcd"


def test_model_forced_zip64():
    names, entries = _mixed()
    a = _check_model(names, entries, flags=2)
    assert a.zip64 and a.data[-22:] == b"PK\5\6" + b"\0" * 4 + b"\xff" * 12 + b"\0\0"
    assert a.data[-42:-38] == b"PK\6\7" and a.data[-98:-94] == b"PK\6\6"
    _check_model(names, entries, flags=3)


def test_model_65535_entries_are_zip64():
    n = 65535
    names = [b"%05d" % k for k in range(n)]
    entries = [b"%d" % k * (k % 5) for k in range(n)]
    a = _check_model(names, entries)
    assert a.zip64 and 0 < a.words[3] < n     # (both methods among them)


def test_model_empty_archive_and_long_name():
    a = _check_model([], [])
    assert a.data == b"PK\5\6" + b"\0" * 18 and a.words == [0, 22, 0, 0] and a.rows == []
    b = _check_model([], [], flags=2)
    assert len(b.data) == 98 and b.words == [0, 98, 0, 0]
    _check_model([b"p" * 65535, b"q"], [b"hello hello hello hello hello", b""])


def test_model_insufficient_space():
    names, entries = _mixed()
    streams = [_deflate(x) for x in entries]
    a = zip_write.build(names, entries, streams)
    b = zip_write.build(names, entries, streams, out_avail=len(a.data))
    assert b == a
    c = zip_write.build(names, entries, streams, out_avail=len(a.data) - 1)
    assert c.data is None and c.rows is None
    assert c.words == [3] + a.words[1:]


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "zip_write_kernels.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == KERNELS
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", rep)]
    sspills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", rep)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", rep)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", rep)]
    assert spills == [0] * len(KERNELS), spills
    assert sspills == [0] * len(KERNELS), sspills
    assert scratch == [0] * len(KERNELS), scratch
    # the final kernel's 16 wave sums
    assert lds == [0, 0, 0, 128], lds
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert [x for x in KERNELS if f"\n{x}(" not in k] == []
