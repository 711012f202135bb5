"""CPU-side checks of the gzip-members writer: the two calls declared, exported
and bound with the header's constants; every refusal that comes before any
device work, with its reason; libdeflate_amd_gzip_members_compress_bound
against the CPU model (tools/models/gzip_members_write.py); the model's files
against Python's gzip and a zlib member walk; and the new kernels' compile
report."""
import ctypes
import gzip
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from tools.models import gzip_members_write as gzmw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_gzip_members_compress_bound",
           "libdeflate_amd_gzip_members_compress_batch")
KERNELS = ["lda_gzmw_member_kernel", "lda_gzmw_place_kernel", "lda_gzmw_final_kernel"]
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
    assert len(lib.libdeflate_amd_gzip_members_compress_bound.argtypes) == 4
    assert len(lib.libdeflate_amd_gzip_members_compress_batch.argtypes) == 15
    assert not binding.MISSING
    for name in ("gzip_members_compress_bound", "gzip_members_compress"):
        assert callable(getattr(api.Compressor, name))


def test_constants_match_the_header():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name):
        return int(re.search(rf"#define {name}\s+(\d+)", hdr).group(1))
    assert define("LIBDEFLATE_AMD_GZMW_RESULT_WORDS") == binding.GZMW_RESULT_WORDS == \
        gzmw.RESULT_WORDS == 4
    # the longest name, with its terminator, is a name the reader accepts
    assert binding.GZMW_NAME_MAX == gzmw.NAME_MAX == 65534
    assert binding.GZMW_NAME_MAX + 1 < define("LIBDEFLATE_AMD_GZM_NAME_MAX") == binding.GZM_NAME_MAX
    plan = open(os.path.join(CSRC, "gzip_members_write_plan.h")).read()
    assert re.search(r"GZMW_RESULT_WORDS = 4,", plan) and re.search(r"GZMW_NAME_MAX = 65534,", plan)
    assert re.search(r"GZMW_EMPTY_STREAM = 5,", plan) and len(gzmw.EMPTY_STREAM) == 5
    assert zlib.decompress(gzmw.EMPTY_STREAM, -15) == b""


def test_the_call_checks_its_arguments(lib):
    """Refused before any device is touched, with a reason: a NULL object or
    pointer (d_in only with in_avail != 0, the host arrays only with
    n_records != 0, names and name_offsets unless both are, d_index never),
    unknown flags, n_records above 2^28, decreasing name_offsets, a name with
    a 0 byte or of more than 65 534 bytes, a record of 4 GiB or more, a record
    outside in_avail."""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    # (its level reads as 0)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    call = lib.libdeflate_amd_gzip_members_compress_batch
    buf = ctypes.create_string_buffer(b"x" * 70000)
    names = ctypes.cast(buf, ctypes.c_void_p)
    _a, noff = _u64(0, 1, 3)
    _b, ioff = _u64(0, 100)
    _c, inn = _u64(100, 50)
    big = 1 << 20

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
        assert "gzip_members_compress_batch" in binding.last_error()
    refused(call(None, 2, names, noff, d, 150, ioff, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(None, 2, None, None, d, 150, ioff, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, None, noff, d, 150, ioff, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, None, d, 150, ioff, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, noff, None, 150, ioff, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, noff, d, 150, None, inn, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, noff, d, 150, ioff, None, d, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, noff, d, 150, ioff, inn, None, big, d, None, 0, 0, None), "NULL")
    refused(call(fake, 2, names, noff, d, 150, ioff, inn, d, big, None, None, 0, 0, None), "NULL")
    refused(call(None, 0, None, None, None, 0, None, None, d, big, d, None, 0, 0, None), "NULL")
    for flags in (1, 2, 0x80000000, 7):
        refused(call(fake, 2, names, noff, d, 150, ioff, inn, d, big, d, None, 0, flags, None),
                "flags")
        refused(call(fake, 2, None, None, d, 150, ioff, inn, d, big, d, None, 0, flags, None),
                "flags")
    refused(call(fake, (1 << 28) + 1, names, noff, d, 150, ioff, inn, d, big, d, None, 0, 0, None),
            "n_records")
    _d, bad = _u64(0, 3, 2)
    refused(call(fake, 2, names, bad, d, 150, ioff, inn, d, big, d, None, 0, 0, None),
            "record 1: name_offsets decrease")
    _d, bad = _u64(0, 1, 65536)
    refused(call(fake, 2, names, bad, d, 150, ioff, inn, d, big, d, None, 0, 0, None),
            "record 1: a name of more than 65534 bytes")
    buf[2] = b"\0"
    refused(call(fake, 2, names, noff, d, 150, ioff, inn, d, big, d, None, 0, 0, None),
            "record 1: a name that holds a 0 byte")
    buf[2] = b"x"
    _d, bad = _u64(100, 1 << 32)
    refused(call(fake, 2, names, noff, d, 1 << 40, ioff, bad, d, 1 << 40, d, None, 0, 0, None),
            "4 GiB")
    refused(call(fake, 2, None, None, d, 1 << 40, ioff, bad, d, 1 << 40, d, None, 0, 0, None),
            "4 GiB")
    refused(call(fake, 2, names, noff, d, 149, ioff, inn, d, big, d, None, 0, 0, None), "in_avail")
    _d, bad = _u64(0, 151)
    refused(call(fake, 2, names, noff, d, 150, bad, inn, d, big, d, None, 0, 0, None),
            "record 1: its bytes do not lie inside in_avail")
    _d, bad = _u64(0, (1 << 64) - 10)
    refused(call(fake, 2, None, None, d, 150, bad, inn, d, big, d, None, 0, 0, None), "in_avail")


def _lib_bound(lib, sizes, name_lens=None):
    sz = np.array(sizes, dtype=np.uint64)
    offs = None
    if name_lens is not None:
        offs = np.zeros(len(sizes) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(np.array(name_lens, dtype=np.uint64), dtype=np.uint64)
        offs += np.uint64(1000)     # only the differences count
    return lib.libdeflate_amd_gzip_members_compress_bound(
        None, len(sizes), offs.ctypes.data_as(ctypes.c_void_p) if offs is not None else None,
        sz.ctypes.data_as(ctypes.c_void_p))


def test_bound_is_the_models(lib):
    rng = np.random.default_rng(0x2A1)
    assert lib.libdeflate_amd_gzip_members_compress_bound(None, 0, None, None) == 0
    assert _lib_bound(lib, [0]) == 18 + 5 == gzmw.bound([0])
    assert _lib_bound(lib, [0], [0]) == 23 and _lib_bound(lib, [0], [1]) == 25
    for n in (1, 4999, 5000, 5001, 10000, 10001):
        blocks = -(-n // 5000)
        assert _lib_bound(lib, [n]) == gzmw.bound([n]) == 18 + n + 5 * blocks
        assert lib.libdeflate_gzip_compress_bound(None, n) == 18 + n + 5 * blocks
    for case in range(40):
        n = int(rng.integers(1, 50))
        nl = [int(x) * int(rng.integers(0, 2)) for x in rng.integers(1, 65535, n)]
        hi = (0, 1000, 1 << 20, (1 << 32) - 1)[case % 4]
        sz = [int(x) for x in rng.integers(0, hi + 1, n)]
        want = sum(lib.libdeflate_gzip_compress_bound(None, s) + (a + 1 if a else 0)
                   for s, a in zip(sz, nl))
        assert _lib_bound(lib, sz, nl) == gzmw.bound(sz, nl) == want
        assert _lib_bound(lib, sz) == gzmw.bound(sz) == want - sum(a + 1 for a in nl if a)


# ---- the model against gzip and against a zlib member walk ----

def _deflate(raw, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(raw) + c.flush()


def _mixed():
    rng = np.random.default_rng(0x2A2)
    text = (b"the quick brown fox jumps over the lazy dog; " * 3000)
    records = [b"", b"a", text[:100], text[:70000], rng.bytes(1000), bytes(5000), text[:4097], b""]
    names = [b"e", None, b"dir/fifteen.txt", b"", "déjà vu/漢字.txt".encode("utf-8"),
             b"n" * 65534, b"\xff", b""]
    return names, records


def _check_model(records, names, mtime=0, level=6):
    streams = [_deflate(x) if x else None for x in records]
    f = gzmw.build(records, streams, names, mtime, level)
    n = len(records)
    nl = [len(x or b"") for x in names] if names is not None else None
    assert f.words == [0, len(f.data), sum(len(x) for x in records), n]
    assert len(f.data) <= gzmw.bound([len(x) for x in records], nl)
    if n:
        assert gzip.decompress(f.data) == b"".join(records)
    index, plain = gzmw.walk(f.data)
    assert index == f.index and plain == list(records)
    # every member alone: the fixed bytes, the name field, the footer
    for k, (raw, (at, uoff)) in enumerate(zip(records, f.index)):
        m = f.data[at:f.index[k + 1][0]]
        name = (names[k] or b"") if names is not None else b""
        assert m[:4] == b"\x1f\x8b\x08" + (b"\x08" if name else b"\0")
        assert int.from_bytes(m[4:8], "little") == mtime
        assert m[8] == gzmw.xfl(level) and m[9] == 0xFF
        body = m[10:]
        if name:
            assert body[:len(name) + 1] == name + b"\0"
            body = body[len(name) + 1:]
        assert body[:-8] == (streams[k] if raw else gzmw.EMPTY_STREAM)
        assert body[-8:] == zlib.crc32(raw).to_bytes(4, "little") + len(raw).to_bytes(4, "little")
    return f


def test_model_files_read_back():
    names, records = _mixed()
    a = _check_model(records, None)
    b = _check_model(records, names, mtime=1700000000)
    assert len(b.data) == len(a.data) + sum(len(x) + 1 for x in names if x)
    _check_model(records, [None] * len(records), mtime=5, level=1)
    _check_model(records, names, level=9)
    assert {gzmw.xfl(lv) for lv in (0, 1)} == {4} and {gzmw.xfl(lv) for lv in range(2, 8)} == {0}
    assert {gzmw.xfl(lv) for lv in range(8, 13)} == {2}


def test_model_unnamed_member_is_the_plain_gzip_stream():
    """with mtime 0 and no name a member is header + stream + footer and
    nothing else: the shape of libdeflate_gzip_compress's output"""
    raw = b"hello hello hello hello"
    s = _deflate(raw)
    m = gzmw.member(raw, s)
    assert m == b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + s + zlib.crc32(raw).to_bytes(4, "little") + \
        len(raw).to_bytes(4, "little")
    assert gzmw.build([raw], [s]).data == m
    assert gzmw.build([b""], [None]).data == \
        b"\x1f\x8b\x08\0\0\0\0\0\0\xff\x01\0\0\xff\xff" + b"\0" * 8


def test_model_no_records_and_insufficient_space():
    f = gzmw.build([], [])
    assert f.data == b"" and f.words == [0, 0, 0, 0] and f.index == [[0, 0]]
    names, records = _mixed()
    streams = [_deflate(x) if x else None for x in records]
    a = gzmw.build(records, streams, names)
    assert gzmw.build(records, streams, names, out_avail=len(a.data)) == a
    c = gzmw.build(records, streams, names, out_avail=len(a.data) - 1)
    assert c.data is None and c.index is None and c.words == [3] + a.words[1:]


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "gzip_members_write_kernels.hip", "-o", os.devnull],
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
    assert lds == [0] * len(KERNELS), lds
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert [x for x in KERNELS if f"\n{x}(" not in k] == []
