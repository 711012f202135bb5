"""CPU-side checks of the call that reads Parquet BYTE_ARRAY pages: declared,
exported and bound, its constants equal in the header, kernels.h, the plan, the
binding and the model; every argument it refuses beyond the old call's, refused
before any device is touched, with its reason and row - and the old call still
refusing bit 14; the plan header free of HIP; and the compile report of
parquet_strings_kernels.hip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tools.models import parquet_model as pm
from tools.models import parquet_strings_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOL = "libdeflate_amd_parquet_decode_batch_ex"
KERNELS = ["lda_pqs_walk_kernel", "lda_pqs_sum_kernel", "lda_pqs_offsets_kernel",
           "lda_pqs_copy_kernel", "lda_pqs_final_kernel"]
BAD_ARG = -2
GZIP = 2


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
    assert SYMBOL in re.findall(r" T (libdeflate_\w+)", out)
    fn = lib.libdeflate_amd_parquet_decode_batch_ex
    assert len(fn.argtypes) == 16 and fn.argtypes[14 - 1] is ctypes.c_uint64      # the flags
    assert not binding.MISSING
    assert callable(api.Decompressor.parquet_decode_batch_ex)


def test_constants_are_equal_everywhere():
    from libdeflate_amd import binding
    hdr = _header()
    k = open(os.path.join(CSRC, "kernels.h")).read()
    plan = open(os.path.join(CSRC, "parquet_strings_plan.h")).read()
    assert re.search(r"#define LIBDEFLATE_AMD_PARQUET_BYTE_ARRAY \(\(uint64_t\)1 << 14\)", hdr)
    assert re.search(r"#define PQ_BYTE_ARRAY \(\(uint64_t\)1 << 14\)", plan)
    assert binding.PARQUET_BYTE_ARRAY == sm.BYTE_ARRAY == 1 << 14
    assert int(re.search(r"PQS_SCAN_BLOCK = (\d+),", plan).group(1)) == \
        int(re.search(r"#define LDA_SCAN_BLOCK (\d+)", k).group(1))
    # the columns' names stand in the same order in the plan and in kernels.h
    enum = re.sub(r"/\*.*?\*/", "", plan[plan.index("enum {"):plan.index("};")], flags=re.S)
    names = re.findall(r"\bPQS_([WSV]_[A-Z_]+|[WSV]COLS)\b", enum)
    assert names == re.findall(r"\bLDA_PQS_([WSV]_[A-Z_]+|[WSV]COLS)\b",
                               k[k.index("LDA_PQS_W_SEC = 0"):k.index("lda_pqs_walk_kernel")])
    # the plan is free of HIP
    assert "hip/" not in plan and "__device__" not in plan and "__global__" not in plan
    assert '"kernels.h"' not in plan and "device_common.h" not in plan


def _rows():
    """four rows the call takes with in_nbytes 100, out_avail 400, valid_avail
    50: a string dictionary, a page coded with it, a PLAIN string page, a
    fixed-width page"""
    from libdeflate_amd import api
    return api.parquet_rows(
        [0, 20, 50, 90], [20, 30, 40, 10], [40, 90, 40, 10],
        [pm.DICT, pm.DATA_V1, pm.DATA_V2, pm.DATA_V1], [5, 20, 6, 2], [1, 1, 1, 5],
        encodings=[0, 8, 0, 0], compressed=[1, 1, 0, 0], max_def=[0, 1, 1, 0], def_lens=[0, 0, 3, 0],
        out_offsets=[0, 0, 168, 390], valid_offsets=[0, 0, 30, 0], dict_rows=[0, 0, 0, 0],
        byte_array=[1, 1, 1, 0])


S = 1 << 14
# (row, word, value, the reason, the row it names)
BAD = [(1, 3, 0 | 8 << 4 | 1 << 12 | 1 << 13 | 1 << 16 | S, "non-zero width field", 1),
       (0, 3, 2 | 1 << 12 | 255 << 16 | S, "non-zero width field", 0),
       (1, 5, 4, "not a multiple of 8", 1), (2, 5, 172, "not a multiple of 8", 2),
       (1, 3, 0 | 8 << 4 | 1 << 12 | 1 << 13, "BYTE_ARRAY on one side only", 1),
       (0, 3, 2 | 1 << 12, "BYTE_ARRAY on one side only", 1),
       (1, 5, 240, "offsets do not lie inside out_avail", 1),
       (2, 5, 392, "offsets do not lie inside out_avail", 2),
       (1, 5, (1 << 64) - 8, "out_avail", 1),
       (1, 3, 0 | 8 << 4 | 1 << 12 | 1 << 13 | S | 1 << 15, "unknown bits", 1),
       (1, 7, 1, "not an earlier row", 1), (2, 6, 45, "valid_avail", 2)]


def test_the_call_checks_its_arguments(lib):
    """LIBDEFLATE_AMD_BAD_ARG before any device work, with a reason and the
    row, on a stand-in object"""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    dec = lib.libdeflate_amd_parquet_decode_batch_ex

    def refused(rc, word, row=None):
        assert rc == BAD_ARG, (rc, word, row, binding.last_error())
        assert word in binding.last_error(), binding.last_error()
        assert row is None or "row %d:" % row in binding.last_error(), binding.last_error()

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    rows = _rows()
    rp = ptr(rows)
    assert dec(fake, GZIP, 0, None, None, 0, None, 0, None, 0, None, 0, None, 0, None, None) == 0
    refused(dec(None, GZIP, 4, rp, d, 100, d, 400, d, 50, d, 10, d, 0, d, None), "NULL")
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 400, d, 50, d, 10, d, 0, None, None), "NULL")
    assert "parquet_decode_batch_ex" in binding.last_error()
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 400, d, 50, d, 10, d, 1, d, None), "flags")
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 400, d, 50, d, 10, d, 1 << 63, d, None), "flags")
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 400, d, 50, None, 10, d, 0, d, None), "d_bytes is NULL")
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 400, d, 50, d, 10, None, 0, d, None),
            "d_bytes_total is NULL", 0)
    refused(dec(fake, 3, 4, rp, d, 100, d, 400, d, 50, d, 10, d, 0, d, None), "format")
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 400, None, 50, d, 10, d, 0, d, None), "d_valid is NULL", 1)
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 399, d, 50, d, 10, d, 0, d, None), "out_avail", 3)
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 400, d, 35, d, 10, d, 0, d, None), "valid_avail", 2)
    for r, word, value, why, at in BAD:
        bad = rows.copy()
        bad[r, word] = value
        refused(dec(fake, GZIP, 4, ptr(bad), d, 100, d, 400, d, 50, d, 10, d, 0, d, None), why, at)
    # the old call goes on refusing the bit, on every row that has it
    old = lib.libdeflate_amd_parquet_decode_batch
    refused(old(fake, GZIP, 4, rp, d, 100, d, 400, d, 50, d, None), "unknown bits", 0)
    refused(old(fake, GZIP, 1, ptr(rows[2:3].copy()), d, 100, d, 400, d, 50, d, None), "unknown bits", 0)


def test_kernels_compile_without_spills_or_scratch():
    assert re.search(r"^NOLICM \?= .*\bparquet_strings_kernels\b",
                     open(os.path.join(CSRC, "Makefile")).read(), re.M)
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-mllvm", "-disable-machine-licm",      # the Makefile's NOLICM
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "parquet_strings_kernels.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == KERNELS
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", rep)]
    sspills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", rep)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", rep)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", rep)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", rep)]
    assert spills == [0] * 5 and sspills == [0] * 5 and scratch == [0] * 5
    # the walk's windows, one per wave: 1040 bytes, 1040 jumps of 2 bytes, 1040 marks;
    # the tile scans' wave sums; the copy's 1025 places and, at the next 16 bytes, 1024 sources
    assert lds == [4 * (1040 + 2 * 1040 + 1040), 32, 32, 8 * (1026 + 1024), 0]
    assert max(vgprs) <= 128        # four waves a SIMD at least
    k = open(os.path.join(CSRC, "kernels.h")).read()
    src = open(os.path.join(CSRC, "parquet_strings_kernels.hip")).read()
    for name in KERNELS:
        assert re.search(rf"^{name}\(", k, re.M) and re.search(rf"^{name}\(", src, re.M)
    # no inline assembly, and nothing spins
    assert "asm" not in src and "while (1)" not in src and "for (;;)" not in src
