"""CPU-side checks of the call that reads Parquet pages: declared, exported and
bound, with the constants equal in the header, kernels.h, the plan, the binding
and the model; every argument it refuses, refused before any device is touched,
with its reason and row; the plan header free of HIP; and the compile report of
parquet_kernels.hip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tools.models import parquet_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOL = "libdeflate_amd_parquet_decode_batch"
KERNELS = ["lda_pq_runs_kernel", "lda_pq_expand_kernel", "lda_pq_final_kernel"]
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
    from libdeflate_amd import api, binding, parquet
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", _header(), re.M))
    assert SYMBOL in declared and SYMBOL in binding.BATCH_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert SYMBOL in re.findall(r" T (libdeflate_\w+)", out)
    fn = lib.libdeflate_amd_parquet_decode_batch
    assert len(fn.argtypes) == 12 and fn.argtypes[1] is ctypes.c_int      # the format
    assert not binding.MISSING
    assert callable(api.Decompressor.parquet_decode_batch) and callable(api.parquet_rows)
    assert callable(parquet.parse) and callable(parquet.pages) and callable(parquet.read_columns)
    src = open(os.path.join(ROOT, "libdeflate_amd", "parquet.py")).read()
    assert "pyarrow" not in src


def test_constants_are_equal_everywhere():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name}\s+(\w+)", text).group(1), 0)

    def enum(name, text):
        return int(re.search(rf"\b{name} = (\w+),", text).group(1), 0)
    k = open(os.path.join(CSRC, "kernels.h")).read()
    plan = open(os.path.join(CSRC, "parquet_plan.h")).read()
    assert define("LIBDEFLATE_AMD_PARQUET_WORDS") == binding.PARQUET_WORDS == pm.WORDS == \
        enum("PQ_WORDS", plan) == 8
    assert define("LIBDEFLATE_AMD_PARQUET_DATA_V1") == binding.PARQUET_DATA_V1 == pm.DATA_V1 == 0
    assert define("LIBDEFLATE_AMD_PARQUET_DICT") == binding.PARQUET_DICT == pm.DICT == 2
    assert define("LIBDEFLATE_AMD_PARQUET_DATA_V2") == binding.PARQUET_DATA_V2 == pm.DATA_V2 == \
        define("LDA_PQ_DATA_V2", k) == 3
    assert define("LDA_PQ_TILE", k) == enum("PQ_TILE", plan) == pm.TILE == 256 * 4
    assert define("LDA_PQ_LEVEL_PIECE", k) == enum("PQ_LEVEL_PIECE", plan) == pm.LEVEL_PIECE == 512
    assert define("LDA_PQ_RUN_WORDS", k) == enum("PQ_RUN_WORDS", plan) == 4
    assert define("LDA_PQ_INFO_WORDS", k) == enum("PQ_INFO_WORDS", plan) == 8
    # the plan is free of HIP
    assert "hip/" not in plan and "__device__" not in plan and "__global__" not in plan
    assert "kernels.h" not in plan and "device_common.h" not in plan


def _rows():
    """four rows the call takes with in_nbytes 100, out_avail 400, valid_avail 50"""
    from libdeflate_amd import api
    return api.parquet_rows(
        [0, 20, 50, 90], [20, 30, 40, 10], [40, 90, 40, 10],
        [pm.DICT, pm.DATA_V1, pm.DATA_V2, pm.DATA_V1], [10, 50, 20, 2], [4, 4, 8, 5],
        encodings=[0, 8, 0, 0], compressed=[1, 1, 0, 0], max_def=[0, 1, 1, 0], def_lens=[0, 0, 3, 0],
        out_offsets=[0, 0, 200, 390], valid_offsets=[0, 0, 30, 0], dict_rows=[0, 0, 0, 0])


# (row, word, value, the reason)
BAD = [(1, 3, 1 << 24, "unknown bits"), (1, 3, 1 << 14, "unknown bits"), (3, 3, 1 | 4 << 16, "a kind"),
       (3, 3, 0 | 3 << 4 | 4 << 16, "an encoding"),
       (0, 3, 2 | 8 << 4 | 1 << 12 | 3 << 16, "dictionary encoding on a dictionary page"),
       (0, 2, 1 << 31, "2^31"), (1, 4, 50 | 1 << 32, "level bytes on a row"),
       (2, 4, 20 | 41 << 32, "level bytes beyond"), (2, 2, 41, "two sizes differ"),
       (3, 0, 91, "in_nbytes"), (3, 0, (1 << 64) - 1, "in_nbytes"), (1, 7, 1, "not an earlier row"),
       (1, 3, 0 | 8 << 4 | 1 << 12 | 1 << 13 | 7 << 16, "another width"),
       (1, 5, 201, "out_avail"), (1, 5, (1 << 64) - 4, "out_avail"), (2, 6, 31, "valid_avail"),
       (2, 6, (1 << 64) - 1, "valid_avail")]


def test_the_call_checks_its_arguments(lib):
    """LIBDEFLATE_AMD_BAD_ARG before any device work, with a reason and the
    row, on a stand-in object: every refusal the header lists"""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    dec = lib.libdeflate_amd_parquet_decode_batch

    def refused(rc, word, row=None):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
        assert row is None or "row %d:" % row in binding.last_error(), binding.last_error()

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    rows = _rows()
    rp = ptr(rows)
    assert dec(fake, GZIP, 0, None, None, 0, None, 0, None, 0, None, None) == 0      # nothing to do
    refused(dec(None, GZIP, 4, rp, d, 100, d, 400, d, 50, d, None), "NULL")
    refused(dec(fake, GZIP, 4, None, d, 100, d, 400, d, 50, d, None), "NULL")
    refused(dec(fake, GZIP, 4, rp, None, 100, d, 400, d, 50, d, None), "NULL")
    refused(dec(fake, GZIP, 4, rp, d, 100, None, 400, d, 50, d, None), "NULL")
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 400, d, 50, None, None), "NULL")
    assert "parquet_decode_batch" in binding.last_error()
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 400, None, 50, d, None), "d_valid is NULL", 1)
    refused(dec(fake, 3, 4, rp, d, 100, d, 400, d, 50, d, None), "format")
    refused(dec(fake, -1, 4, rp, d, 100, d, 400, d, 50, d, None), "format")
    refused(dec(fake, GZIP, (1 << 28) + 1, rp, d, 100, d, 400, d, 50, d, None), "n_pages")
    refused(dec(fake, GZIP, 4, rp, d, 99, d, 400, d, 50, d, None), "in_nbytes", 3)
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 399, d, 50, d, None), "out_avail", 3)
    refused(dec(fake, GZIP, 4, rp, d, 100, d, 400, d, 49, d, None), "valid_avail", 1)
    for r, word, value, why in BAD:
        bad = rows.copy()
        bad[r, word] = value
        refused(dec(fake, GZIP, 4, ptr(bad), d, 100, d, 400, d, 50, d, None), why, r)
    bad = np.concatenate([rows, rows[3:]])
    bad[4, 3] |= 2 << 4         # dictionary-coded, and its dictionary row is a data page
    bad[4, 7] = 3
    refused(dec(fake, GZIP, 5, ptr(bad), d, 100, d, 400, d, 50, d, None), "not a dictionary page", 4)


def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "parquet_kernels.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == KERNELS
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", rep)]
    sspills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", rep)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", rep)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", rep)]
    assert spills == [0] * 3 and sspills == [0] * 3 and scratch == [0] * 3
    assert lds == [4 * 4096, 0, 0]      # the run walk's windows, one per wave
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    src = open(os.path.join(CSRC, "parquet_kernels.hip")).read()
    for name in KERNELS:
        assert re.search(rf"^{name}\(", k, re.M) and re.search(rf"^{name}\(", src, re.M)
    # no inline assembly, and no workgroup waits for another
    assert "asm" not in src and "__syncthreads" not in src and "while (1)" not in src
