"""CPU-side checks of the calls that read and write byte-shuffled deflate chunks
(HDF5, NetCDF-4, Zarr): the three calls declared, exported and bound, with the
constants equal in the header, kernels.h, the plan and the model; every
argument they refuse, refused before any device is touched, with its reason
and row; the bound against the model; the plan header free of HIP; and the
compile report of shuffle_kernels.hip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tools.models import shuffle_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_shuffle_decompress_batch", "libdeflate_amd_shuffle_compress_bound",
           "libdeflate_amd_shuffle_compress_batch")
KERNELS = ["lda_unshuffle_kernel", "lda_shuf_final_kernel", "lda_shuffle_kernel",
           "lda_shufw_chunk_kernel", "lda_shufw_place_kernel", "lda_shufw_final_kernel"]
BAD_ARG = -2
ZLIB = 1


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
    from libdeflate_amd import api, binding
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", _header(), re.M))
    assert set(SYMBOLS) <= declared
    assert set(SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    assert len(lib.libdeflate_amd_shuffle_decompress_batch.argtypes) == 10
    assert len(lib.libdeflate_amd_shuffle_compress_bound.argtypes) == 4
    assert len(lib.libdeflate_amd_shuffle_compress_batch.argtypes) == 11
    assert lib.libdeflate_amd_shuffle_decompress_batch.argtypes[1] is ctypes.c_int    # format
    assert lib.libdeflate_amd_shuffle_compress_bound.restype is ctypes.c_size_t
    assert not binding.MISSING
    assert callable(api.Decompressor.decompress_shuffle_batch)
    assert callable(api.Compressor.compress_shuffle_batch)
    assert callable(api.Compressor.shuffle_compress_bound) and callable(api.shuffle_rows)


def test_constants_are_equal_everywhere():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name}\s+(\w+)", text).group(1), 0)

    def enum(name, text):
        return int(re.search(rf"\b{name} = (\w+),", text).group(1), 0)
    k = open(os.path.join(CSRC, "kernels.h")).read()
    plan = open(os.path.join(CSRC, "shuffle_plan.h")).read()
    assert define("LIBDEFLATE_AMD_SHUF_WORDS") == binding.SHUF_WORDS == sm.WORDS == \
        enum("SHUF_WORDS", plan) == 6
    assert define("LIBDEFLATE_AMD_SHUF_ELEM_MAX") == binding.SHUF_ELEM_MAX == sm.ELEM_MAX == \
        enum("SHUF_ELEM_MAX", plan) == 256
    assert define("LIBDEFLATE_AMD_SHUF_NO_DEFLATE") == binding.SHUF_NO_DEFLATE == sm.NO_DEFLATE == \
        enum("SHUF_NO_DEFLATE", plan) == 1
    assert define("LIBDEFLATE_AMD_SHUF_NO_SHUFFLE") == binding.SHUF_NO_SHUFFLE == sm.NO_SHUFFLE == \
        enum("SHUF_NO_SHUFFLE", plan) == 2
    assert define("LIBDEFLATE_AMD_SHUFW_RESULT_WORDS") == binding.SHUFW_RESULT_WORDS == \
        sm.RESULT_WORDS == enum("SHUF_RESULT_WORDS", plan) == 4
    # the tile sizes: kernels.h, the plan, the model
    assert define("LDA_SHUF_TILE", k) == enum("SHUF_TILE", plan) == sm.TILE == 256 * 16
    assert define("LDA_SHUF_GEN_BYTES", k) == enum("SHUF_GEN_BYTES", plan) == sm.GEN_BYTES
    # the staging area of the kernels' generic path holds every element size's tile
    src = open(os.path.join(CSRC, "shuffle_kernels.hip")).read()
    lds = define("SHUF_LDS_BYTES", src)
    assert max(es * (sm.tile_elems(es) + 16) for es in range(1, 257) if es not in (1, 2, 4, 8)) <= lds
    # the plan is free of HIP, and so is what it shares with the other chunk codecs' plans
    for text in (plan, open(os.path.join(CSRC, "chunk_plan.h")).read()):
        assert "hip/" not in text and "__device__" not in text and "__global__" not in text
        assert "kernels.h" not in text and "device_common.h" not in text


def _rows():
    """three rows the reader takes with in_nbytes 20 and out_avail 47"""
    return np.array([[3, 10, 0, 40, 4, 0], [13, 7, 40, 7, 3, sm.NO_DEFLATE],
                     [20, 0, 47, 0, 256, sm.NO_DEFLATE | sm.NO_SHUFFLE]], dtype=np.uint64)


def test_calls_check_their_arguments(lib):
    """LIBDEFLATE_AMD_BAD_ARG before any device work, with a reason and the
    row, on a stand-in object: NULL arguments, an unknown format, n_chunks
    above 2^28, an element size of 0 or above 256, unknown mask bits, a raw
    size of 2^32, a stored range outside in_nbytes, a room outside out_avail"""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    dec = lib.libdeflate_amd_shuffle_decompress_batch
    enc = lib.libdeflate_amd_shuffle_compress_batch
    bnd = lib.libdeflate_amd_shuffle_compress_bound

    def refused(rc, word, row=None):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
        assert row is None or "row %d:" % row in binding.last_error(), binding.last_error()
    rows = _rows()
    rp = rows.ctypes.data_as(ctypes.c_void_p)
    assert dec(fake, ZLIB, 0, None, None, 0, None, 0, None, None) == 0      # nothing to do
    refused(dec(None, ZLIB, 3, rp, d, 20, d, 47, d, None), "NULL")
    refused(dec(fake, ZLIB, 3, None, d, 20, d, 47, d, None), "NULL")
    refused(dec(fake, ZLIB, 3, rp, None, 20, d, 47, d, None), "NULL")
    refused(dec(fake, ZLIB, 3, rp, d, 20, None, 47, d, None), "NULL")
    refused(dec(fake, ZLIB, 3, rp, d, 20, d, 47, None, None), "NULL")
    assert "shuffle_decompress_batch" in binding.last_error()
    for fmt in (-1, 3, 4, 99):
        refused(dec(fake, fmt, 3, rp, d, 20, d, 47, d, None), "format")
        refused(enc(fake, fmt, 0, None, d, 47, d, 4096, d, None, None), "format")
    refused(dec(fake, ZLIB, (1 << 28) + 1, rp, d, 20, d, 47, d, None), "n_chunks")
    refused(enc(fake, ZLIB, (1 << 28) + 1, rp, d, 47, d, 4096, d, None, None), "n_chunks")
    refused(dec(fake, ZLIB, 3, rp, d, 19, d, 47, d, None), "in_nbytes", 1)
    refused(dec(fake, ZLIB, 3, rp, d, 20, d, 46, d, None), "out_avail", 1)
    for r in range(3):
        for col, value, word in ((4, 0, "element size"), (4, 257, "element size"),
                                 (4, 1 << 40, "element size"), (5, 4, "mask"), (5, 7, "mask"),
                                 (5, 1 << 63, "mask"), (3, 1 << 32, "2^32"),
                                 (0, 21, "in_nbytes"), (0, (1 << 64) - 1, "in_nbytes"),
                                 (1, 18, "in_nbytes"), (2, 48, "out_avail"),
                                 (2, (1 << 64) - 2, "out_avail"), (3, 48, "out_avail")):
            bad = rows.copy()
            bad[r, col] = value
            want = sm.row_why(bad[r], True, 20, 47)
            assert want == word
            refused(dec(fake, ZLIB, 3, bad.ctypes.data_as(ctypes.c_void_p), d, 20, d, 47, d, None),
                    word, r)
    # the writer: words 2 to 5, NO_SHUFFLE alone, in_avail in the place of out_avail
    wrows = rows.copy()
    wrows[:, 5] = [0, sm.NO_SHUFFLE, 0]
    wrows[:, :2] = (1 << 64) - 1            # ignored
    wp = wrows.ctypes.data_as(ctypes.c_void_p)
    refused(enc(None, ZLIB, 3, wp, d, 47, d, 4096, d, None, None), "NULL")
    refused(enc(fake, ZLIB, 3, None, d, 47, d, 4096, d, None, None), "NULL")
    refused(enc(fake, ZLIB, 3, wp, None, 47, d, 4096, d, None, None), "NULL")
    refused(enc(fake, ZLIB, 3, wp, d, 47, None, 4096, d, None, None), "NULL")
    refused(enc(fake, ZLIB, 3, wp, d, 47, d, 4096, None, None, None), "NULL")
    assert "shuffle_compress_batch" in binding.last_error()
    refused(enc(fake, ZLIB, 3, wp, d, 46, d, 4096, d, None, None), "in_avail", 1)
    refused(enc(fake, ZLIB, 3, rp, d, 47, d, 4096, d, None, None), "mask", 1)   # NO_DEFLATE
    for r in range(3):
        for col, value, word in ((4, 0, "element size"), (4, 257, "element size"), (5, 1, "mask"),
                                 (5, 6, "mask"), (3, 1 << 32, "2^32"), (2, 48, "in_avail"),
                                 (3, 48, "in_avail")):
            bad = wrows.copy()
            bad[r, col] = value
            assert sm.row_why(bad[r], False, 0, 47) == word
            bp = bad.ctypes.data_as(ctypes.c_void_p)
            refused(enc(fake, ZLIB, 3, bp, d, 47, d, 4096, d, None, None), word, r)
            assert bnd(fake, ZLIB, 3, bp) == 0 or word == "in_avail"


def test_the_bound_is_the_models(lib):
    """libdeflate_amd_shuffle_compress_bound (no device): the sum of
    libdeflate_<format>_compress_bound over the raw sizes, 0 for rows the
    writer refuses"""
    from libdeflate_amd import api
    sizes = [0, 1, 4999, 5000, 5001, 65536, 1 << 20, (1 << 32) - 1, 123457]
    rows = api.shuffle_rows([7 * k for k in range(len(sizes))], sizes, [1, 2, 3, 4, 8, 16, 255, 256, 5],
                            mask=[0, 2] * 4 + [0])
    assert rows.tolist() == sm.rows([7 * k for k in range(len(sizes))], sizes,
                                    [1, 2, 3, 4, 8, 16, 255, 256, 5], mask=[0, 2] * 4 + [0]).tolist()
    rp = rows.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    for fmt, name in enumerate(("deflate", "zlib", "gzip")):
        one = getattr(lib, "libdeflate_%s_compress_bound" % name)
        assert lib.libdeflate_amd_shuffle_compress_bound(fake, fmt, len(sizes), rp) == \
            sm.bound(name, rows) == sum(one(None, n) for n in sizes)
        assert lib.libdeflate_amd_shuffle_compress_bound(fake, fmt, 0, None) == 0
    assert lib.libdeflate_amd_shuffle_compress_bound(fake, 3, len(sizes), rp) == 0
    assert lib.libdeflate_amd_shuffle_compress_bound(fake, 1, 1, None) == 0


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "shuffle_kernels.hip", "-o", os.devnull],
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
    # the staging area of the generic path: eight workgroups of it fit a CU's LDS
    assert lds == [20480, 0, 20480, 0, 0, 0], lds
    # memory-bound transposes want waves to hide their loads (DESIGN 3.24 quotes
    # the figures: 7 and 4 waves per SIMD)
    assert occ[0] >= 7 and occ[2] >= 4, occ
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    src = open(os.path.join(CSRC, "shuffle_kernels.hip")).read()
    for name in KERNELS:
        assert re.search(rf"^{name}\(", k, re.M) and re.search(rf"^{name}\(", src, re.M)
    # no inline assembly
    assert "asm" not in src
