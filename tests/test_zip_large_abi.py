"""CPU-side checks of libdeflate_amd_zip_read_large: the call declared, exported
and bound; LIBDEFLATE_AMD_ZIP_PIECE the same in the header, the binding and
kernels.h; every BAD_ARG refused before any device is touched, with its
reason; the test archive (tests/zip_large_files.py) as the tests need it; the
condition under which the GPU tests may cap their selections at 64 entries;
and the new kernel's compile report."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import zip_files as zf
from tests import zip_large_files as zl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOL = "libdeflate_amd_zip_read_large"
BAD_ARG = -2
CAP = 64        # entries per selection in tests/test_zip_large_gpu.py


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from libdeflate_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    return binding.load()


def _header():
    return open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()


def test_symbol_declared_exported_and_bound(lib):
    from libdeflate_amd import api, binding
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", _header(), re.M))
    assert SYMBOL in declared and SYMBOL in binding.BATCH_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert SYMBOL in set(re.findall(r" T (libdeflate_\w+)", out))
    # the sibling's arguments and large_min
    assert len(lib.libdeflate_amd_zip_read_large.argtypes) == 14
    assert len(lib.libdeflate_amd_zip_read_batch.argtypes) == 13
    assert not binding.MISSING
    assert callable(api.Decompressor.read_zip_large)


def test_piece_constant_matches_everywhere():
    from libdeflate_amd import binding

    def shift(name, text):
        return 1 << int(re.search(rf"#define {name}\s+\(1u << (\d+)\)", text).group(1))
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert shift("LIBDEFLATE_AMD_ZIP_PIECE", _header()) == shift("LDA_ZIP_PIECE", k) \
        == binding.ZIP_PIECE == zl.PIECE == 1 << 20
    # the plan's copies of the kernel's constants
    plan = open(os.path.join(CSRC, "zip_large_plan.h")).read()
    for name, value in (("OWNED", 48), ("MANY_WAVE", 1), ("PIECED", 2)):
        assert int(re.search(rf"#define LDA_ZIPL_{name} (\d+)", k).group(1)) == value
        assert re.search(rf"ZIPL_{name} = {value},", plan)
    # the kernel's declaration is its definition's
    assert "\nlda_zip_lfinal_kernel(" in k


def test_call_checks_its_arguments(lib):
    """What libdeflate_amd_zip_read_batch refuses, refused here too before any
    device is touched, under this call's name: a NULL object or pointer (d_out
    only with out_avail != 0, d_in only with in_nbytes != 0), an out_align that
    is no power of two in 1 .. 256, in_nbytes above 2^36, entries or n_sel
    above 2^28, rows outside the file, sizes of 4 GiB, entry numbers, room -
    whatever large_min says."""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    rd = lib.libdeflate_amd_zip_read_large

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
        assert "zip_read_large" in binding.last_error()
    # rows of a file of 1000 bytes
    rows = np.array([[900, 4, 8, 0x1234, 40, 100, 500, 0],
                     [950, 4, 0, 0x1234, 200, 30, 30, 500]], dtype=np.uint64)
    rp = rows.ctypes.data_as(ctypes.c_void_p)

    def sel(*s):
        a = np.array(s, dtype=np.uint64)
        return a, a.ctypes.data_as(ctypes.c_void_p)
    a, sp = sel(0, 1)
    for lm in (0, 1, 50, 1 << 40):
        refused(rd(None, d, 1000, rp, 2, 2, sp, d, 4096, 1, lm, None, d, None), "NULL")
        refused(rd(fake, None, 1000, rp, 2, 2, sp, d, 4096, 1, lm, None, d, None), "NULL")
        refused(rd(fake, d, 1000, None, 2, 2, sp, d, 4096, 1, lm, None, d, None), "NULL")
        refused(rd(fake, d, 1000, rp, 2, 2, None, d, 4096, 1, lm, None, d, None), "NULL")
        refused(rd(fake, d, 1000, rp, 2, 2, sp, None, 4096, 1, lm, None, d, None), "NULL")
        refused(rd(fake, d, 1000, rp, 2, 2, sp, d, 4096, 1, lm, None, None, None), "NULL")
        for align in (0, 3, 48, 512, 1 << 20):
            refused(rd(fake, d, 1000, rp, 2, 2, sp, d, 4096, align, lm, None, d, None),
                    "out_align")
        refused(rd(fake, d, (1 << 36) + 1, rp, 2, 2, sp, d, 4096, 1, lm, None, d, None),
                "in_nbytes")
        refused(rd(fake, d, 1000, rp, (1 << 28) + 1, 2, sp, d, 4096, 1, lm, None, d, None),
                "2^28")
        refused(rd(fake, d, 1000, rp, 2, (1 << 28) + 1, sp, d, 4096, 1, lm, None, d, None),
                "2^28")
        refused(rd(fake, d, 1000, rp, 2, 2, sp, d, 529, 1, lm, None, d, None), "out_avail")
        refused(rd(fake, d, 1000, rp, 2, 2, sp, d, 530 + 13, 16, lm, None, d, None), "out_avail")
        refused(rd(fake, d, 949, rp, 2, 2, sp, d, 4096, 1, lm, None, d, None), "in_nbytes")
        refused(rd(fake, d, 139, rp, 2, 1, sp, d, 4096, 1, lm, None, d, None), "in_nbytes")
    a, sp = sel(1, 2)
    refused(rd(fake, d, 1000, rp, 2, 2, sp, d, 4096, 1, 0, None, d, None), "sel[1] = 2")
    big = rows.copy()
    big[0, 6] = 1 << 32
    a, sp = sel(0)
    refused(rd(fake, d, 1000, big.ctypes.data_as(ctypes.c_void_p), 2, 1, sp, d, 1 << 40, 1, 1,
               None, d, None), "4 GiB")
    # nothing selected: nothing to do, and the offsets say so
    offs = np.full(1, 77, dtype=np.uint64)
    assert rd(fake, d, 1000, rp, 2, 0, None, d, 0, 1, 0, offs.ctypes.data_as(ctypes.c_void_p),
              None, None) == 0
    assert offs[0] == 0


def test_the_large_archive_is_what_the_tests_need():
    a = zl.archive()
    rows = {n: r for n, r in zip(zl.NAMES, zl.rows_of(a))}
    assert 13 * zl.MIB < sum(len(b) for b in a.datas) < 16 * zl.MIB

    def sizes(name):
        return rows[name][2] & 0xFFFF, rows[name][5], rows[name][6]
    assert sizes("text3m")[0] == 8 and sizes("text3m")[2] == 3 * zl.MIB + 17
    assert 65536 < sizes("text3m")[1] < 2 * zl.MIB
    # exactly one piece: many-wave but not pieced; one byte more: two pieces
    assert sizes("text1m")[0] == 8 and sizes("text1m")[2] == zl.PIECE
    assert sizes("text1m")[1] > 20000
    assert sizes("text1m+1")[2] == zl.PIECE + 1
    # random bytes under method 8: stored blocks inside DEFLATE
    m, cs, us = sizes("random")
    assert m == 8 and us == 3 * zl.MIB // 2 and us < cs < us + 1024
    # pieced but not many-wave
    m, cs, us = sizes("zeros")
    assert m == 8 and us == 4 * zl.MIB and cs < 20000
    assert sizes("stored2m+1") == (0, 2 * zl.MIB + 1, 2 * zl.MIB + 1)
    assert sizes("stored2m") == (0, 2 * zl.MIB, 2 * zl.MIB)
    assert sizes("empty")[2] == 0
    small = [sizes(n)[2] for n in zl.NAMES if n.startswith("small")]
    assert len(small) == 5 and min(small) == 100 and max(small) == 60000
    assert [zl.NAMES[k] for k in zl.LARGE] == ["text3m", "text1m", "text1m+1", "random", "zeros",
                                               "stored2m+1", "stored2m"]
    # room behind the stored entry's data for the csize + 1 case of the GPU tests
    assert rows["text3m"][4] + rows["text3m"][5] < len(a.data)


def test_the_cap_of_64_entries_loses_no_defect():
    """The GPU tests compare read_zip_large with read_zip_batch on the first
    min(m, 64) entries of every existing file, to keep the 65 600-entry file
    from making 65 600 blocking calls.  That is sound as long as every file
    but `many` fits the cap whole and every per-entry defect lies within it."""
    for name in zf.GOOD_NAMES:
        m = len(zf.expected(zf.good(name))[0])
        assert m <= CAP or name == "many", (name, m)
    for d in zf.defects():
        m = len(zf.expected(d.base)[0])
        assert m <= CAP and (d.entry is None or d.entry < CAP), d.name


def test_kernel_compiles_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "zip_large_kernels.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == ["lda_zip_lfinal_kernel"]
    for what in ("VGPRs Spill", "SGPRs Spill", r"ScratchSize \[bytes/lane\]",
                 r"LDS Size \[bytes/block\]"):
        assert [int(x) for x in re.findall(what + r": (\d+)", rep)] == [0], what
