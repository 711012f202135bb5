"""CPU-side checks of the calls that read and write predictor-coded deflate
strips and tiles (TIFF, GeoTIFF): the three calls declared, exported and bound,
with the constants equal in the header, kernels.h, the plan, the binding and
the model; every argument they refuse, refused before any device is touched,
with its reason and row; the bound against the model and against
libdeflate_zlib_compress_bound; the plan header free of HIP; and the compile
report of tiff_kernels.hip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tools.models import tiff_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_tiff_decode_batch", "libdeflate_amd_tiff_encode_bound",
           "libdeflate_amd_tiff_encode_batch")
KERNELS = ["lda_tiff_unpredict_kernel", "lda_tiff_gather_kernel", "lda_tiff_predict_kernel",
           "lda_tiffw_index_kernel"]
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


def test_symbols_declared_exported_and_bound(lib):
    from libdeflate_amd import api, binding, tiff
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", _header(), re.M))
    assert set(SYMBOLS) <= declared
    assert set(SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    assert len(lib.libdeflate_amd_tiff_decode_batch.argtypes) == 9
    assert len(lib.libdeflate_amd_tiff_encode_bound.argtypes) == 3
    assert len(lib.libdeflate_amd_tiff_encode_batch.argtypes) == 10
    assert lib.libdeflate_amd_tiff_decode_batch.argtypes[1] is ctypes.c_size_t   # no format argument
    assert lib.libdeflate_amd_tiff_encode_bound.restype is ctypes.c_size_t
    assert not binding.MISSING
    assert callable(api.Decompressor.decode_tiff_batch)
    assert callable(api.Compressor.encode_tiff_batch)
    assert callable(api.Compressor.tiff_encode_bound) and callable(api.tiff_rows)
    assert callable(tiff.parse) and callable(tiff.build)


def test_constants_are_equal_everywhere():
    from libdeflate_amd import binding, tiff
    hdr = _header()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name}\s+(\w+)", text).group(1), 0)

    def enum(name, text):
        return int(re.search(rf"\b{name} = (\w+),", text).group(1), 0)
    k = open(os.path.join(CSRC, "kernels.h")).read()
    plan = open(os.path.join(CSRC, "tiff_plan.h")).read()
    assert define("LIBDEFLATE_AMD_TIFF_WORDS") == binding.TIFF_WORDS == tm.WORDS == tiff.WORDS == \
        enum("TIFF_WORDS", plan) == define("LDA_TIFF_WORDS", k) == 8
    assert define("LIBDEFLATE_AMD_TIFF_SPP_MAX") == binding.TIFF_SPP_MAX == tm.SPP_MAX == \
        enum("TIFF_SPP_MAX", plan) == define("LDA_TIFF_SPP_MAX", k) == 16
    assert define("LIBDEFLATE_AMD_TIFFW_RESULT_WORDS") == binding.TIFFW_RESULT_WORDS == \
        tm.RESULT_WORDS == enum("TIFF_RESULT_WORDS", plan) == 4
    assert define("LDA_TIFF_PTILE", k) == enum("TIFF_PTILE", plan) == tm.PTILE == 256 * 16
    # the strides the kernel keeps in registers: the plan's, the model's, the kernel's cases
    src = open(os.path.join(CSRC, "tiff_kernels.hip")).read()
    cases = {(int(sb), int(st)) for sb, st in re.findall(r"TIFF_SCAN_CASE\((\d+), (\d+)\)", src)}
    assert {st for _, st in cases} == set(tm.REG_STRIDES)
    for st in tm.REG_STRIDES:
        assert re.search(rf"st == {st}\b", plan)
        # every sample size that gives a whole number of at most 16 samples has its case
        assert {sb for sb in (1, 2, 4, 8) if st % sb == 0 and st // sb <= 16} == \
            {sb for sb, s in cases if s == st}
    # the plan is free of HIP
    assert "hip/" not in plan and "__device__" not in plan and "__global__" not in plan
    assert "kernels.h" not in plan and "device_common.h" not in plan


def _rows():
    """three rows the reader takes with in_nbytes 30 and out_avail 200"""
    return np.array([tm.row(3, 10, 0, 30, (10, 4), (10, 4), 3, 1, 2),
                     tm.row(13, 7, 120, 50, (8, 2), (5, 2), 1, 2, 3),
                     tm.row(20, 10, 180, 0, (5, 1), (5, 1), 1, 4, 1)], dtype=np.uint64)


BAD = [(6, 0 | 1 << 8 | 2 << 16, "samples per pixel"), (6, 17 | 1 << 8 | 2 << 16, "samples per pixel"),
       (6, 1 | 3 << 8 | 2 << 16, "bytes per sample"), (6, 1 | 0 << 8 | 2 << 16, "bytes per sample"),
       (6, 1 | 1 << 8 | 0 << 16, "predictor"), (6, 1 | 1 << 8 | 4 << 16, "predictor"),
       (6, 1 | 1 << 8 | 3 << 16, "floating-point"), (6, 1 | 1 << 8 | 1 << 16 | 1 << 24, "word 6"),
       (6, 1 | 1 << 8 | 1 << 16 | 1 << 63, "word 6"), (7, 1, "word 7"), (7, 1 << 40, "word 7"),
       (4, 0 | 4 << 32, "zero"), (4, 10, "zero"), (5, 0 | 1 << 32, "zero"), (5, 1, "zero"),
       (5, 11 | 1 << 32, "kept above coded"), (5, 1 | 5 << 32, "kept above coded"),
       (4, 65536 | 65536 << 32, "2^32"), (4, 0xFFFFFFFF | 0xFFFFFFFF << 32, "2^32")]
BAD_READER = [(0, 31, "in_nbytes"), (0, (1 << 64) - 1, "in_nbytes"), (1, 28, "in_nbytes")]
BAD_RAW = [(2, 201), (2, (1 << 64) - 4)]


def test_calls_check_their_arguments(lib):
    """LIBDEFLATE_AMD_BAD_ARG before any device work, with a reason and the
    row, on a stand-in object: every refusal the header lists"""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    dec = lib.libdeflate_amd_tiff_decode_batch
    enc = lib.libdeflate_amd_tiff_encode_batch
    bnd = lib.libdeflate_amd_tiff_encode_bound

    def refused(rc, word, row=None):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
        assert row is None or "row %d:" % row in binding.last_error(), binding.last_error()

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    rows = _rows()
    rp = ptr(rows)
    for r in rows:
        assert tm.row_why(r, True, 30, 200) is None
    assert dec(fake, 0, None, None, 0, None, 0, None, None) == 0      # nothing to do
    assert enc(fake, 0, None, None, 0, d, 4096, d, None, None) == 0
    refused(dec(None, 3, rp, d, 30, d, 200, d, None), "NULL")
    refused(dec(fake, 3, None, d, 30, d, 200, d, None), "NULL")
    refused(dec(fake, 3, rp, None, 30, d, 200, d, None), "NULL")
    refused(dec(fake, 3, rp, d, 30, None, 200, d, None), "NULL")
    refused(dec(fake, 3, rp, d, 30, d, 200, None, None), "NULL")
    assert "tiff_decode_batch" in binding.last_error()
    refused(dec(fake, (1 << 28) + 1, rp, d, 30, d, 200, d, None), "n_segments")
    refused(enc(fake, (1 << 28) + 1, rp, d, 200, d, 4096, d, None, None), "n_segments")
    refused(dec(fake, 3, rp, d, 29, d, 200, d, None), "in_nbytes", 2)
    refused(dec(fake, 3, rp, d, 30, d, 199, d, None), "out_avail", 2)
    refused(dec(fake, 3, rp, d, 30, d, 179, d, None), "out_avail", 1)
    for r in range(3):
        for col, value, word in BAD + BAD_READER + [(c, v, "out_avail") for c, v in BAD_RAW]:
            bad = rows.copy()
            if word == "kept above coded":
                bad[r, 4] = 10 | 4 << 32
            bad[r, col] = value
            assert tm.row_why(bad[r], True, 30, 200) == word
            refused(dec(fake, 3, ptr(bad), d, 30, d, 200, d, None), word, r)
    # the pitch: below the kept row's bytes; a last row outside, overflow included
    for value, word in ((29, "pitch"), (0, "pitch"), (57, "out_avail"), ((1 << 64) // 3 + 1, "out_avail"),
                        ((1 << 64) - 1, "out_avail")):
        bad = rows.copy()
        bad[0, 3] = value
        assert tm.row_why(bad[0], True, 30, 200) == word
        refused(dec(fake, 3, ptr(bad), d, 30, d, 200, d, None), word, 0)
    ok = rows.copy()
    ok[2, 3] = (1 << 64) - 1    # a single row: its pitch is not looked at
    assert tm.row_why(ok[2], True, 30, 200) is None
    # the writer: words 2 to 7, in_avail in the place of out_avail
    wrows = rows.copy()
    wrows[:, :2] = (1 << 64) - 1            # ignored
    wp = ptr(wrows)
    refused(enc(None, 3, wp, d, 200, d, 4096, d, None, None), "NULL")
    refused(enc(fake, 3, None, d, 200, d, 4096, d, None, None), "NULL")
    refused(enc(fake, 3, wp, None, 200, d, 4096, d, None, None), "NULL")
    refused(enc(fake, 3, wp, d, 200, None, 4096, d, None, None), "NULL")
    refused(enc(fake, 3, wp, d, 200, d, 4096, None, None, None), "NULL")
    assert "tiff_encode_batch" in binding.last_error()
    refused(enc(fake, 3, wp, d, 199, d, 4096, d, None, None), "in_avail", 2)
    for r in range(3):
        for col, value, word in BAD + [(c, v, "in_avail") for c, v in BAD_RAW] + [(3, 1, "pitch")]:
            if word == "pitch" and r == 2:
                continue
            bad = wrows.copy()
            if word == "kept above coded":
                bad[r, 4] = 10 | 4 << 32
            bad[r, col] = value
            assert tm.row_why(bad[r], False, 0, 200) == word
            refused(enc(fake, 3, ptr(bad), d, 200, d, 4096, d, None, None), word, r)
            assert bnd(fake, 3, ptr(bad)) == 0 or word == "in_avail"


def test_the_bound_is_the_models(lib):
    """libdeflate_amd_tiff_encode_bound (no device): the sum of
    libdeflate_zlib_compress_bound over the coded sizes, 0 for rows the writer
    refuses"""
    from libdeflate_amd import api
    shapes = [((1, 1), 1, 1), ((4999, 1), 1, 1), ((5000, 1), 1, 1), ((5001, 1), 1, 1), ((256, 256), 3, 1),
              ((256, 256), 1, 4), ((32768, 16), 1, 2), ((65535, 4095), 16, 1), ((7, 3), 5, 8)]
    rows = api.tiff_rows([7 * k for k in range(len(shapes))], 1 << 20, [s[0] for s in shapes],
                         [(1, 1)] * len(shapes), [s[1] for s in shapes], [s[2] for s in shapes], 2)
    sizes = [s[0][0] * s[0][1] * s[1] * s[2] for s in shapes]
    assert max(sizes) < 1 << 32 and max(sizes) > 1 << 31
    rp = rows.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    assert lib.libdeflate_amd_tiff_encode_bound(fake, len(shapes), rp) == tm.bound(rows) == \
        sum(lib.libdeflate_zlib_compress_bound(None, n) for n in sizes)
    assert lib.libdeflate_amd_tiff_encode_bound(fake, 0, None) == 0
    assert lib.libdeflate_amd_tiff_encode_bound(fake, 1, None) == 0
    rows[3, 7] = 1
    assert lib.libdeflate_amd_tiff_encode_bound(fake, len(shapes), rp) == tm.bound(rows) == 0


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "tiff_kernels.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == KERNELS
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", rep)]
    sspills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", rep)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", rep)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", rep)]
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", rep)]
    assert spills == [0] * len(KERNELS), spills
    assert sspills == [0] * len(KERNELS), sspills
    assert scratch == [0] * len(KERNELS), scratch
    assert lds == [0] * len(KERNELS), lds
    # memory-bound kernels want waves to hide their loads (DESIGN 3.25 quotes the figures)
    assert occ[0] >= 3 and min(occ[1:]) >= 8, occ
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    src = open(os.path.join(CSRC, "tiff_kernels.hip")).read()
    for name in KERNELS:
        assert re.search(rf"^{name}\(", k, re.M) and re.search(rf"^{name}\(", src, re.M)
    # no inline assembly, and nothing that waits: no atomics, no barriers
    assert "asm" not in src and "atomic" not in src and "__syncthreads" not in src
