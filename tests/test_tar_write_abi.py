"""CPU-side checks of the tar writer: the three calls declared, exported and
bound; every refusal before any device is touched; the size query and the
plan's index rows against what Python's tarfile writes (walked by
tools/models/tar_walk.py); and the new kernel's compile report."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import tar_write_cases as tw
from tools.models import tar_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_tar_write_size", "libdeflate_amd_tar_write_batch",
           "libdeflate_amd_targz_compress_batch")
BAD_ARG = -2
GZIP = 2
SIZES = [0, 1, 15, 16, 17, 511, 512, 513, 4096, 65024, 65535, 65536, 65537, 200000]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from libdeflate_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    return binding.load()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _size(lib, names, sizes):
    blob, offs, _, inn = tw.call_arrays(names, sizes)
    return lib.libdeflate_amd_tar_write_size(len(names), _p(offs), _p(blob), _p(inn))


def test_symbols_declared_exported_and_bound(lib):
    from libdeflate_amd import api, binding
    hdr = open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", hdr, re.M))
    assert set(SYMBOLS) <= declared
    assert set(SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    # the argument counts are the header's
    for name, count in zip(SYMBOLS, (4, 14, 16)):
        decl = re.search(rf"^{name}\(([^;]*)\);", hdr, re.M | re.S).group(1)
        assert decl.count(",") + 1 == count == len(getattr(lib, name).argtypes), name
    assert not binding.MISSING
    for name in ("tar_write_size", "write_tar_batch", "compress_targz_batch"):
        assert callable(getattr(api.Compressor, name))


def test_constants_match_the_header():
    from libdeflate_amd import binding
    hdr = open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()
    k = open(os.path.join(CSRC, "kernels.h")).read()
    plan = open(os.path.join(CSRC, "tar_write_plan.h")).read()

    def define(name, text):
        return int(re.search(rf"#define {name}\s+(\d+)", text).group(1))
    assert define("LIBDEFLATE_AMD_TAR_WORDS", hdr) == binding.TAR_WORDS == 8
    assert re.search(r"TARW_ROW_WORDS = 8,", plan)
    assert re.search(r"TARW_BLOCK = 512,", plan) and re.search(r"TARW_RECORD = 10240,", plan)
    assert (tw.BLOCK, tw.RECORD) == (512, 10240)
    assert define("LDA_TARW_TILE", k) == tw.TILE == tar_walk.COPY_TILE
    # an entry's row, as the kernel reads it and as the plan writes it
    words = ["OFF", "PAX", "NAME_OFF", "NAME_LEN", "SRC", "SIZE"]
    assert [define(f"LDA_TARW_E_{w}", k) for w in words] == list(range(6))
    assert define("LDA_TARW_ECOLS", k) == 6
    body = re.search(r"TARW_E_OFF = 0,(.*?)TARW_ECOLS", plan, re.S).group(1)
    assert re.findall(r"TARW_E_(\w+),", body) == words[1:]
    # the name sources of the rows are the reader's
    assert (tar_walk.NAME_HEADER, tar_walk.NAME_PAX) == (0, 2)


def test_calls_check_their_arguments(lib):
    """Refused before any device is touched, with a reason: a NULL object or
    pointer, unknown flags, n_entries above 2^28, decreasing name_offsets, a
    name that is empty, too long, holds a 0 byte or is not UTF-8, an entry of
    8^11 bytes, mtime of 8^11, an entry outside in_avail, out_avail below the
    size; for the .tar.gz call the format and its own out_avail rule."""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    wr = lib.libdeflate_amd_tar_write_batch
    gz = lib.libdeflate_amd_targz_compress_batch
    big = 1 << 40

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()

    def both(word, names=("a",), sizes=(4,), offsets=None, in_avail=4096, mtime=0, flags=0,
             n=None, arrays=None):
        blob, offs, ino, inn = arrays or tw.call_arrays(list(names), list(sizes), offsets)
        n = len(inn) if n is None else n
        refused(wr(fake, n, _p(blob), _p(offs), d, in_avail, _p(ino), _p(inn), d, big, None,
                   mtime, flags, None), word)
        assert "tar_write_batch" in binding.last_error()
        refused(gz(fake, GZIP, n, _p(blob), _p(offs), d, in_avail, _p(ino), _p(inn), d, big, d,
                   None, mtime, flags, None), word)
        assert "targz_compress_batch" in binding.last_error()
    blob, offs, ino, inn = tw.call_arrays(["a"], [4])
    ok = (_p(blob), _p(offs), d, 4096, _p(ino), _p(inn))
    refused(wr(None, 1, *ok, d, big, None, 0, 0, None), "NULL")
    refused(wr(fake, 1, *ok, None, big, None, 0, 0, None), "NULL")
    refused(wr(fake, 1, _p(blob), _p(offs), None, 4096, _p(ino), _p(inn), d, big, None, 0, 0, None),
            "NULL")
    for hole in range(4):       # names, name_offsets, in_offsets, in_nbytes
        a = [_p(blob), _p(offs), _p(ino), _p(inn)]
        a[hole] = None
        refused(wr(fake, 1, a[0], a[1], d, 4096, a[2], a[3], d, big, None, 0, 0, None), "NULL")
        refused(gz(fake, GZIP, 1, a[0], a[1], d, 4096, a[2], a[3], d, big, d, None, 0, 0, None),
                "NULL")
    refused(gz(None, GZIP, 1, *ok, d, big, d, None, 0, 0, None), "NULL")
    refused(gz(fake, GZIP, 1, *ok, None, big, d, None, 0, 0, None), "NULL")
    refused(gz(fake, GZIP, 1, *ok, d, big, None, None, 0, 0, None), "NULL")
    refused(gz(fake, 7, 1, *ok, d, big, d, None, 0, 0, None), "format")
    refused(gz(fake, GZIP, 1, *ok, d, 18, d, None, 0, 0, None), "out_avail")
    both("flags", flags=1)
    both("2^28", n=(1 << 28) + 1)
    both("mtime", mtime=1 << 33)
    both("empty name", names=("a", ""), sizes=(1, 1))
    both("65535", names=("n" * 65536,))
    both("0 byte", names=(b"a\0b",))
    for bad in (b"a\x80", b"\xC3", b"\xC0\xAF", b"\xED\xA0\x80", b"\xF4\x90\x80\x80", b"\xFF"):
        both("UTF-8", names=(bad,))
    both("8 GiB", sizes=(1 << 33,), in_avail=1 << 34)
    # 128 entries of 8 GiB - 1 (the same bytes): more than one launch writes
    both("1 TiB", names=["big"] * 128, sizes=[(1 << 33) - 1] * 128, offsets=[0] * 128,
         in_avail=1 << 33)
    both("in_avail", sizes=(4097,))
    both("in_avail", offsets=(4093,))
    both("entry 1", names=("a", "b"), sizes=(4, 4), offsets=(0, 4093))
    dec = tw.call_arrays(["ab", "cd"], [1, 1])
    dec[1][:] = (2, 4, 3)
    both("decrease", arrays=dec)
    # out_avail below the archive's size, one byte
    refused(wr(fake, 1, *ok, d, 10239, None, 0, 0, None), "out_avail")
    refused(wr(fake, 0, None, None, None, 0, None, None, d, 10239, None, 0, 0, None), "out_avail")
    # the size query: 0 and a reason
    assert lib.libdeflate_amd_tar_write_size(1, None, _p(blob), _p(inn)) == 0
    assert "NULL" in binding.last_error()
    assert lib.libdeflate_amd_tar_write_size((1 << 28) + 1, _p(offs), _p(blob), _p(inn)) == 0
    assert lib.libdeflate_amd_tar_write_size(2, _p(dec[1]), _p(dec[0]), _p(dec[3])) == 0
    assert lib.libdeflate_amd_tar_write_size(0, None, None, None) == 10240
    # one check serves the query and the calls: a name they refuse has no size
    for bad in (b"a\x80", b"a\0b", b"n" * 65536):
        assert _size(lib, [bad], [1]) == 0
    assert _size(lib, ["big"] * 128, [(1 << 33) - 1] * 128) == 0
    assert _size(lib, ["big"] * 127, [(1 << 33) - 1] * 127) > 1 << 39


def test_size_is_tarfiles(lib):
    """libdeflate_amd_tar_write_size == len() of the tarfile archive: every
    size alone and all together, every edge name, and archives that end at a
    multiple of 10 240 minus 1024, minus 512 and minus 0"""
    for s in SIZES:
        assert _size(lib, ["f"], [s]) == len(tw.tarfile_bytes(["f"], [bytes(s)]))
    names = [f"dir/f{k}" for k in range(len(SIZES))]
    assert _size(lib, names, SIZES) == len(tw.tarfile_bytes(names, [bytes(s) for s in SIZES]))
    names = tw.edge_names()
    sizes = [(37 * k) % 1500 for k in range(len(names))]
    assert _size(lib, names, sizes) == len(tw.tarfile_bytes(names, [bytes(s) for s in sizes]))
    for name in names:
        assert _size(lib, [name], [5]) == len(tw.tarfile_bytes([name], [b"12345"]))
    assert _size(lib, [], []) == len(tw.tarfile_bytes([], [])) == 10240
    for data, want in ((10240 - 512 - 1024, 10240), (10240 - 512 - 512, 20480), (10240 - 512, 20480),
                       (10240 - 512 - 1024 - 1, 10240), (10240 - 512 - 1024 + 1, 20480)):
        assert _size(lib, ["e"], [data]) == len(tw.tarfile_bytes(["e"], [bytes(data)])) == want


def test_plan_rows_are_what_the_reader_finds_in_tarfiles_bytes(tmp_path):
    """the writer's index rows (tools/test_tar_write_plan.cpp prints the
    plan's) equal, word for word, the rows the reader's model finds in the
    archive tarfile wrote for the same entries"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "tar_write_rows")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tools", "test_tar_write_plan.cpp")], check=True)
    names = tw.edge_names() + [f"f{s}" for s in SIZES]
    sizes = [(37 * k) % 1500 for k in range(len(tw.edge_names()))] + SIZES
    ref = tw.tarfile_bytes(names, [bytes(s) for s in sizes])
    blob, offs, _, inn = tw.call_arrays(names, sizes)
    path = tmp_path / "entries.bin"
    path.write_bytes(struct.pack("<QQ", len(names), tw.MTIME) + offs.tobytes() + inn.tobytes() +
                     blob.tobytes())
    out = subprocess.run([exe, "rows", str(path)], capture_output=True, text=True, check=True).stdout
    lines = out.split("\n")
    assert int(lines[0]) == len(ref)
    rows = [[int(x) for x in line.split()] for line in lines[1:1 + len(names)]]
    model = tar_walk.read(ref, 4 * len(names), extract=False)
    assert model.words[0] == 0 and model.words[1] == len(names)
    assert model.words[4] == tar_walk.EOF | tar_walk.HAS_PAX
    assert rows == [list(r) for r in model.rows]
    got = [tar_walk.name_of(ref, r).decode("utf-8") for r in rows]
    assert got == names


# ---- the kernel as the compiler reports it ----

KERNELS = ["lda_tarw_pack_kernel"]


def test_kernels_compile_without_spills_or_scratch():
    """with the Makefile's flags for this object (it is built without the
    machine-level loop-invariant hoisting): no scratch, no spills, and the
    registers and LDS of DESIGN 3.18"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "tar_write_kernels" in re.search(r"^NOLICM \?= (.*)$", mk, re.M).group(1).split()
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off", "-mllvm",
                        "-disable-machine-licm", "-Rpass-analysis=kernel-resource-usage",
                        "--cuda-device-only", "-c", "tar_write_kernels.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == KERNELS

    def figures(what):
        return [int(x) for x in re.findall(what + r": (\d+)", rep)]
    assert figures("VGPRs Spill") == [0]
    assert figures("SGPRs Spill") == [0]
    assert figures(r"ScratchSize \[bytes/lane\]") == [0]
    # four waves' 104 bytes of name staging; 32 VGPRs: eight waves per SIMD
    assert figures(r"LDS Size \[bytes/block\]") == [4 * 13 * 8]
    assert figures(" VGPRs") == [32]
    assert figures("TotalSGPRs") == [96]
    assert figures(r"Occupancy \[waves/SIMD\]") == [8]
    # the declaration the host side launches through is the definition's
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert [x for x in KERNELS if f"\n{x}(" not in k] == []
    # the reader's gather still takes its copy from the shared header
    assert "copy_tile(" in open(os.path.join(CSRC, "tar_copy.h")).read()
    assert '#include "tar_copy.h"' in open(os.path.join(CSRC, "tar_kernels.hip")).read()
