"""CPU-side checks of the calls that read and write OpenEXR ZIP / ZIPS chunks:
the three calls declared, exported and bound, with the constants equal in the
header, kernels.h, the plan, the binding and the model; every argument they
refuse, refused before any device is touched, with its reason and row; the bound
against the model; the plan header free of HIP; and the compile report of
exr_kernels.hip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tools.models import exr_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_exr_decode_batch", "libdeflate_amd_exr_encode_bound",
           "libdeflate_amd_exr_encode_batch")
KERNELS = ["lda_exr_sums_kernel", "lda_exr_carry_kernel", "lda_exr_undo_kernel",
           "lda_exr_layout_kernel", "lda_exr_gather_kernel", "lda_exr_code_kernel",
           "lda_exrw_choose_kernel", "lda_exrw_place_kernel"]
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
    from libdeflate_amd import api, binding, exr
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", _header(), re.M))
    assert set(SYMBOLS) <= declared
    assert set(SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    assert len(lib.libdeflate_amd_exr_decode_batch.argtypes) == 9
    assert len(lib.libdeflate_amd_exr_encode_bound.argtypes) == 3
    assert len(lib.libdeflate_amd_exr_encode_batch.argtypes) == 10
    assert lib.libdeflate_amd_exr_decode_batch.argtypes[1] is ctypes.c_size_t   # no format argument
    assert lib.libdeflate_amd_exr_encode_bound.restype is ctypes.c_size_t
    assert not binding.MISSING
    assert callable(api.Decompressor.decode_exr_batch)
    assert callable(api.Compressor.encode_exr_batch)
    assert callable(api.Compressor.exr_encode_bound) and callable(api.exr_rows)
    assert callable(exr.parse) and callable(exr.build)


def test_constants_are_equal_everywhere():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name}\s+(\w+)", text).group(1), 0)

    def enum(name, text):
        return int(re.search(rf"\b{name} = (\w+),", text).group(1), 0)
    k = open(os.path.join(CSRC, "kernels.h")).read()
    plan = open(os.path.join(CSRC, "exr_plan.h")).read()
    assert define("LIBDEFLATE_AMD_EXR_WORDS") == binding.EXR_WORDS == em.WORDS == \
        enum("EXR_WORDS", plan) == define("LDA_EXR_WORDS", k) == 10
    assert define("LIBDEFLATE_AMD_EXR_CHANNELS_MAX") == binding.EXR_CHANNELS_MAX == em.CHANNELS_MAX == \
        enum("EXR_CHANNELS_MAX", plan) == 16
    assert define("LIBDEFLATE_AMD_EXRW_RESULT_WORDS") == binding.EXRW_RESULT_WORDS == \
        em.RESULT_WORDS == enum("EXR_RESULT_WORDS", plan) == 4
    assert define("LIBDEFLATE_AMD_EXR_LINES") == binding.EXR_LINES == em.LINES == 0
    assert define("LIBDEFLATE_AMD_EXR_PIXELS") == binding.EXR_PIXELS == em.PIXELS == 1
    assert define("LDA_EXR_LANE", k) == enum("EXR_LANE", plan) == em.LANE == 32
    assert define("LDA_EXR_TILE", k) == enum("EXR_TILE", plan) == em.TILE == 64 * em.LANE
    assert define("LDA_EXR_WG_TILES", k) == enum("EXR_WG_TILES", plan) == em.WG_TILES == 4
    assert define("LDA_EXR_LTILE", k) == enum("EXR_LTILE", plan) == 256
    assert define("LDA_EXR_CTILE", k) == enum("EXR_CTILE", plan) == 256 * 16
    # the plan is free of HIP
    assert "hip/" not in plan and "__device__" not in plan and "__global__" not in plan
    assert "kernels.h" not in plan and "device_common.h" not in plan


def _rows():
    """three rows the reader takes with in_nbytes 30 and out_avail 200"""
    return np.array([em.row(3, 10, 0, 30, (5, 4), [False] * 3, head=(0,)),
                     em.row(13, 7, 120, 50, (1, 2), [False, True], em.PIXELS, [1, 0], head=(1, 2, 0, 0)),
                     em.row(20, 10, 180, 0, (5, 1), [True], em.PIXELS, [0])], dtype=np.uint64)


# (word, value, the reason) for a row of 3 HALF channels in LINES
BAD = [(5, 0, "channels"), (5, 17, "channels"), (5, 3 | 8 << 8, "wide-mask"),
       (5, 3 | 1 << 24, "unknown bits"), (5, 3 | 2 << 32, "unknown bits"), (5, 3 | 1 << 63, "unknown bits"),
       (4, 0 | 4 << 32, "zero"), (4, 5, "zero"), (6, 1, "word 6"),
       (5, 3 | 1 << 32, "permutation"),                 # PIXELS with the slots 0 0 0
       (7, 4, "head length"), (7, 12, "head length"), (7, 1 << 40, "head length"),
       (4, 0x40000000 | 4 << 32, "2^32"), (4, 5 | 0xFFFFFFFF << 32, "2^32")]
BAD_READER = [(0, 31, "in_nbytes"), (0, (1 << 64) - 1, "in_nbytes"), (1, 28, "in_nbytes")]
BAD_PIX = [(2, 201), (2, (1 << 64) - 4)]


def test_calls_check_their_arguments(lib):
    """LIBDEFLATE_AMD_BAD_ARG before any device work, with a reason and the
    row, on a stand-in object: every refusal the header lists"""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    dec = lib.libdeflate_amd_exr_decode_batch
    enc = lib.libdeflate_amd_exr_encode_batch
    bnd = lib.libdeflate_amd_exr_encode_bound

    def refused(rc, word, row=None):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
        assert row is None or "row %d:" % row in binding.last_error(), binding.last_error()

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    rows = _rows()
    rp = ptr(rows)
    for r in rows:
        assert em.row_why(r, True, 30, 200) is None
    assert dec(fake, 0, None, None, 0, None, 0, None, None) == 0      # nothing to do
    assert enc(fake, 0, None, None, 0, d, 4096, d, None, None) == 0
    refused(dec(None, 3, rp, d, 30, d, 200, d, None), "NULL")
    refused(dec(fake, 3, None, d, 30, d, 200, d, None), "NULL")
    refused(dec(fake, 3, rp, None, 30, d, 200, d, None), "NULL")
    refused(dec(fake, 3, rp, d, 30, None, 200, d, None), "NULL")
    refused(dec(fake, 3, rp, d, 30, d, 200, None, None), "NULL")
    assert "exr_decode_batch" in binding.last_error()
    refused(dec(fake, (1 << 28) + 1, rp, d, 30, d, 200, d, None), "n_chunks")
    refused(enc(fake, (1 << 28) + 1, rp, d, 200, d, 4096, d, None, None), "n_chunks")
    refused(dec(fake, 3, rp, d, 29, d, 200, d, None), "in_nbytes", 2)
    refused(dec(fake, 3, rp, d, 30, d, 199, d, None), "out_avail", 2)
    refused(dec(fake, 3, rp, d, 30, d, 175, d, None), "out_avail", 1)
    for r in range(3):
        for col, value, word in BAD + BAD_READER + [(c, v, "out_avail") for c, v in BAD_PIX]:
            bad = rows.copy()
            if col in (4, 5, 6):        # the table's values are for 3 HALF channels in LINES
                bad[r] = rows[0]
                bad[r, 0], bad[r, 1] = 0, 0
            bad[r, col] = value
            assert em.row_why(bad[r], True, 30, 200) == word, (r, col, value)
            refused(dec(fake, 3, ptr(bad), d, 30, d, 200, d, None), word, r)
    # slots that are no permutation
    for value in (0x00, 0x21, 0x110, 0x02):
        bad = rows.copy()
        bad[1, 6] = value
        assert em.row_why(bad[1], True, 30, 200) == "permutation"
        refused(dec(fake, 3, ptr(bad), d, 30, d, 200, d, None), "permutation", 1)
    # the pitch: below the line's bytes; a last line outside, overflow included
    for value, word in ((29, "pitch"), (0, "pitch"), (57, "out_avail"), ((1 << 64) // 3 + 1, "out_avail"),
                        ((1 << 64) - 1, "out_avail")):
        bad = rows.copy()
        bad[0, 3] = value
        assert em.row_why(bad[0], True, 30, 200) == word
        refused(dec(fake, 3, ptr(bad), d, 30, d, 200, d, None), word, 0)
    ok = rows.copy()
    ok[2, 3] = (1 << 64) - 1    # a single line: its pitch is not looked at
    assert em.row_why(ok[2], True, 30, 200) is None
    # the writer: words 2 to 9, in_avail in the place of out_avail
    wrows = rows.copy()
    wrows[:, :2] = (1 << 64) - 1            # ignored
    wp = ptr(wrows)
    refused(enc(None, 3, wp, d, 200, d, 4096, d, None, None), "NULL")
    refused(enc(fake, 3, None, d, 200, d, 4096, d, None, None), "NULL")
    refused(enc(fake, 3, wp, None, 200, d, 4096, d, None, None), "NULL")
    refused(enc(fake, 3, wp, d, 200, None, 4096, d, None, None), "NULL")
    refused(enc(fake, 3, wp, d, 200, d, 4096, None, None, None), "NULL")
    assert "exr_encode_batch" in binding.last_error()
    refused(enc(fake, 3, wp, d, 199, d, 4096, d, None, None), "in_avail", 2)
    for r in range(3):
        for col, value, word in BAD + [(c, v, "in_avail") for c, v in BAD_PIX] + [(3, 1, "pitch")]:
            if word == "pitch" and r == 2:
                continue
            bad = wrows.copy()
            if col in (4, 5, 6):
                bad[r] = wrows[0]
            bad[r, col] = value
            assert em.row_why(bad[r], False, 0, 200) == word
            refused(enc(fake, 3, ptr(bad), d, 200, d, 4096, d, None, None), word, r)
            assert bnd(fake, 3, ptr(bad)) == 0 or word == "in_avail"


def test_the_bound_is_the_models(lib):
    """libdeflate_amd_exr_encode_bound (no device): the sum of head + raw size,
    0 for rows the writer refuses"""
    from libdeflate_amd import api
    shapes = [((1, 1), [False], ()), ((4999, 1), [True], (5,)), ((256, 256), [False] * 4, (1, 2, 0, 0)),
              ((65535, 4095), [False, True, False, True, True], (0,)), ((7, 3), [True] * 16, ())]
    rows = np.concatenate([api.exr_rows([7 * k], 1 << 20, s[0], s[1], heads=[s[2]])
                           for k, s in enumerate(shapes)])
    sizes = [s[0][0] * s[0][1] * sum(em.sizes_of(s[1])) for s in shapes]
    heads = [4 * len(s[2]) + 4 if s[2] else 0 for s in shapes]
    assert max(sizes) < 1 << 32 and max(sizes) > 1 << 31
    rp = rows.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    assert lib.libdeflate_amd_exr_encode_bound(fake, len(shapes), rp) == em.bound(rows) == \
        sum(sizes) + sum(heads)
    assert lib.libdeflate_amd_exr_encode_bound(fake, 0, None) == 0
    assert lib.libdeflate_amd_exr_encode_bound(fake, 1, None) == 0
    rows[3, 7] = 1
    assert lib.libdeflate_amd_exr_encode_bound(fake, len(shapes), rp) == em.bound(rows) == 0


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "exr_kernels.hip", "-o", os.devnull],
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
    # memory-bound kernels want waves to hide their loads (DESIGN 3.26 quotes the figures)
    assert min(occ) >= 8, occ
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    src = open(os.path.join(CSRC, "exr_kernels.hip")).read()
    for name in KERNELS:
        assert re.search(rf"^{name}\(", k, re.M) and re.search(rf"^{name}\(", src, re.M)
    # no inline assembly, and nothing that waits: no atomics, no barriers
    assert "asm" not in src and "atomic" not in src and "__syncthreads" not in src
