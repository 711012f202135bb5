"""CPU-side checks of the PNG writer: the two calls declared, exported and bound
with the header's constants; every refusal that comes before any device work,
with its reason; libdeflate_amd_png_encode_bound against the CPU model
(tools/models/png_write.py); api.png_image_rows; and the new kernels' compile
report, pinned."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tools.models import png_model as pm
from tools.models import png_write as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_png_encode_bound", "libdeflate_amd_png_encode_batch")
KERNELS = ["lda_pngw_filter4_kernel", "lda_pngw_filter16_kernel", "lda_pngw_filter64_kernel",
           "lda_pngw_image_kernel", "lda_pngw_place_kernel", "lda_pngw_final_kernel"]
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


def _rows(*rows):
    a = np.array(rows, dtype=np.uint64).reshape(-1, 8)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_declared_exported_and_bound(lib):
    from libdeflate_amd import api, binding
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", _header(), re.M))
    assert set(SYMBOLS) <= declared
    assert set(SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    assert len(lib.libdeflate_amd_png_encode_bound.argtypes) == 3
    assert len(lib.libdeflate_amd_png_encode_batch.argtypes) == 12
    assert lib.libdeflate_amd_png_encode_batch.argtypes[9] is ctypes.c_uint32     # filter
    assert lib.libdeflate_amd_png_encode_batch.argtypes[10] is ctypes.c_uint32    # flags
    assert not binding.MISSING
    for name in ("png_encode_bound", "encode_png_batch"):
        assert callable(getattr(api.Compressor, name))
    assert callable(api.png_image_rows)


def test_constants_match_the_header():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name):
        return int(re.search(rf"#define {name}\s+(\d+)", hdr).group(1))
    assert define("LIBDEFLATE_AMD_PNG_FILTER_ADAPTIVE") == binding.PNG_FILTER_ADAPTIVE == \
        pw.ADAPTIVE == 5
    assert define("LIBDEFLATE_AMD_PNGW_RESULT_WORDS") == binding.PNGW_RESULT_WORDS == \
        pw.RESULT_WORDS == 4
    plan = open(os.path.join(CSRC, "png_write_plan.h")).read()
    assert re.search(r"PNGW_RESULT_WORDS = 4,", plan)
    assert re.search(r"PNGW_FILTER_ADAPTIVE = 5,", plan)
    # the plan is free of HIP
    assert "hip/" not in plan and "__device__" not in plan and "__global__" not in plan
    # the reader's header no longer lists a writer among what is not covered
    assert "a writer" not in hdr


GOOD = [10, 45, 5 | 3 << 32, 8 | 2 << 8, 0, 0, 0, 0]
PAL = [60, 28, 13 | 4 << 32, 4 | 3 << 8, 0, 0, 88 | 5 << 48, 103 | 5 << 48]


def test_the_call_checks_its_arguments(lib):
    """LIBDEFLATE_AMD_BAD_ARG before any device is touched, with a reason."""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    # (its level reads as 0)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    call = lib.libdeflate_amd_png_encode_batch
    _a, rp = _rows(GOOD, PAL)
    big = 1 << 20

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
        assert "png_encode_batch" in binding.last_error()
    refused(call(None, 2, rp, d, 108, d, big, d, None, 5, 0, None), "NULL")
    refused(call(fake, 2, None, d, 108, d, big, d, None, 5, 0, None), "NULL")
    refused(call(fake, 2, rp, None, 108, d, big, d, None, 5, 0, None), "NULL")
    refused(call(fake, 2, rp, d, 108, None, big, d, None, 5, 0, None), "NULL")
    refused(call(fake, 2, rp, d, 108, d, big, None, None, 5, 0, None), "NULL")
    refused(call(None, 0, None, None, 0, d, big, d, None, 5, 0, None), "NULL")
    for filt in (6, 7, 255, 0x80000000):
        refused(call(fake, 2, rp, d, 108, d, big, d, None, filt, 0, None), "filter")
    for flags in (2, 3, 0x80000000):
        refused(call(fake, 2, rp, d, 108, d, big, d, None, 5, flags, None), "flags")
    refused(call(fake, (1 << 28) + 1, rp, d, 108, d, big, d, None, 5, 0, None), "n_images")
    refused(call(fake, 2, rp, d, 107, d, big, d, None, 5, 0, None),
            "image 1: its tRNS does not lie inside in_avail")
    # d_in NULL with in_avail 0: no pointer to refuse, the pixels are nowhere
    refused(call(fake, 2, rp, None, 0, d, big, d, None, 5, 0, None), "image 0: its pixels")

    def row(base, col, value, word, avail=2000):
        bad = list(base)
        bad[col] = value
        _b, bp = _rows(GOOD, bad)
        refused(call(fake, 2, bp, d, avail, d, big, d, None, 5, 0, None), "image 1: ")
        assert word in binding.last_error(), binding.last_error()
        assert pw.refusal(bad, avail, 0) is not None
        if "in_avail" not in word:
            assert lib.libdeflate_amd_png_encode_bound(fake, 2, bp) == 0
    for value in (3 << 32, 5, 1 << 31 | 3 << 32, 5 | 1 << 63):
        row(GOOD, 2, value, "width or height")
    for value in (4 | 2 << 8, 8 | 5 << 8, 16 | 3 << 8, 3):
        row(GOOD, 3, value, "bit depth and colour type")
    row(GOOD, 3, 8 | 2 << 8 | 1 << 16, "interlaced")
    row(GOOD, 1, 44, "word 1 is not height * rowbytes")
    row(GOOD, 1, 46, "word 1 is not height * rowbytes")
    row(GOOD, 0, 1956, "pixels do not lie inside in_avail")
    row(GOOD, 0, (1 << 64) - 1, "pixels do not lie inside in_avail")
    big_dims = list(GOOD)
    big_dims[1] = 65536 * 65536 * 4
    big_dims[3] = 8 | 6 << 8
    row(big_dims, 2, 65536 | 65536 << 32, "2^32", 1 << 40)
    # 3 rows of 1 + w bytes are 2^32 - 1: no level-0 compress call takes them
    # (the stand-in object's level reads as 0) ...
    w = 0xFFFFFFFF // 3 - 1
    wide = [0, 3 * w, w | 3 << 32, 8, 0, 0, 0, 0]
    row(wide, 0, 0, "level-0", 1 << 40)
    # ... and one IDAT holds 2^31 - 1 bytes
    tall = [0, 46340 * 46341, 46340 | 46341 << 32, 8, 0, 0, 0, 0]
    assert pw.zlib_bound(46341 * 46341) > (1 << 31) - 1
    row(tall, 0, 0, "zlib bound is above 2^31 - 1", 1 << 40)
    # PLTE and tRNS
    row(GOOD, 6, 60 | 257 << 48, "PLTE has no entry, above 256")
    row(GOOD, 6, 60, "PLTE has no entry")
    row(GOOD, 6, 1998 | 1 << 48, "PLTE does not lie inside in_avail")
    row(GOOD, 7, 60 | 5 << 48, "tRNS length")
    row(GOOD, 7, 1995 | 6 << 48, "tRNS does not lie inside in_avail")
    row(PAL, 6, 0, "palette image without a PLTE")
    row(PAL, 6, 88 | 17 << 48, "1 << depth")
    row(PAL, 7, 103 | 6 << 48, "tRNS length")
    grey = [0, 15, 5 | 3 << 32, 8, 0, 0, 20 | 1 << 48, 0]
    row(grey, 0, 0, "PLTE with a grey colour type")
    row(grey, 3, 8 | 4 << 8, "word 1")      # (grey + alpha has 30 bytes)
    ga = [0, 30, 5 | 3 << 32, 8 | 4 << 8, 0, 0, 0, 40 | 2 << 48]
    row(ga, 0, 0, "tRNS with an alpha colour type")
    rgba = [0, 60, 5 | 3 << 32, 8 | 6 << 8, 0, 0, 0, 40 | 6 << 48]
    row(rgba, 0, 0, "tRNS with an alpha colour type")


def test_bound_is_the_models(lib):
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    bound = lib.libdeflate_amd_png_encode_bound
    assert bound(fake, 0, None) == 0
    assert bound(None, 1, _rows(GOOD)[1]) == 0
    _a, rp = _rows(GOOD, PAL)
    want = (8 + 25 + 12 + lib.libdeflate_zlib_compress_bound(None, 3 * 16) + 12) + \
        (8 + 25 + 12 + 15 + 12 + 5 + 12 + lib.libdeflate_zlib_compress_bound(None, 4 * 8) + 12)
    assert bound(fake, 2, rp) == want == pw.bound([GOOD, PAL])
    rng = np.random.default_rng(0x5C1)
    for case in range(30):
        rows = []
        for _ in range(int(rng.integers(1, 40))):
            d, c = pm.COMBOS[int(rng.integers(len(pm.COMBOS)))]
            w, h = int(rng.integers(1, (5, 300, 70000)[case % 3])), int(rng.integers(1, 3000))
            r = [int(rng.integers(0, 1 << 40)), h * pm.rowbytes(w, d, c), w | h << 32,
                 d | c << 8 | int(rng.integers(0, 1 << 30)) << 24, 1, 2, 0, 0]
            if c == 3:
                r[6] = 7 | int(rng.integers(1, (1 << d) + 1)) << 48
                r[7] = 9 | int(rng.integers(0, (r[6] >> 48) + 1)) << 48 if rng.integers(2) else 0
                r[7] = r[7] if r[7] >> 48 else 0
            elif c in (0, 2) and rng.integers(2):
                r[7] = 11 | (2 if c == 0 else 6) << 48
            rows.append(r)
        _b, bp = _rows(*rows)
        assert bound(fake, len(rows), bp) == pw.bound(rows) != 0


def test_png_image_rows():
    from libdeflate_amd import api
    rows = api.png_image_rows([(3, 5), (3, 5, 1), (4, 6, 2), (2, 7, 3), (1, 9, 4)],
                              [0, 100, 200, 300, 400])
    assert [int(r[3]) for r in rows] == [8, 8, 8 | 4 << 8, 8 | 2 << 8, 8 | 6 << 8]
    assert [int(r[1]) for r in rows] == [15, 15, 48, 42, 36]
    assert [int(r[2]) for r in rows] == [5 | 3 << 32, 5 | 3 << 32, 6 | 4 << 32, 7 | 2 << 32,
                                         9 | 1 << 32]
    assert all(pw.refusal(r, 1000) is None for r in rows)
    rows = api.png_image_rows([(4, 13), (2, 3, 3)], [60, 5], depth=[4, 16], colour=[3, None],
                              plte=[(88, 5), None], trns=[(103, 5), (50, 6)])
    assert rows.tolist() == [PAL, [5, 36, 3 | 2 << 32, 16 | 2 << 8, 0, 0, 0, 50 | 6 << 48]]
    with pytest.raises(ValueError):
        api.png_image_rows([(4, 13, 3)], [0], colour=6)


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_report_is_pinned():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "png_write_kernels.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == KERNELS

    def column(what):
        return [int(x) for x in re.findall(what + r": (\d+)", rep)]
    assert column("VGPRs Spill") == [0] * len(KERNELS)
    assert column("SGPRs Spill") == [0] * len(KERNELS)
    assert column(r"ScratchSize \[bytes/lane\]") == [0] * len(KERNELS)
    assert column(r"LDS Size \[bytes/block\]") == [0] * len(KERNELS)
    # the figures of DESIGN 3.21
    assert column(" VGPRs") == [123, 123, 123, 54, 54, 8]
    assert column("TotalSGPRs") == [96, 98, 98, 77, 95, 18]
    assert column(r"Occupancy \[waves/SIMD\]") == [4, 4, 4, 8, 8, 8]
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert [x for x in KERNELS if f"\n{x}(" not in k] == []
    src = open(os.path.join(CSRC, "png_write_kernels.hip")).read()
    assert '#include "zip_write_device.h"' in src and "zw_place_pieces(" in src
