"""CPU-side checks of the PNG reader: the three calls declared, exported and
bound with the header's constants; every argument the two device calls refuse,
refused before any device is touched and with a reason; png_out_sizes and
png_shapes against the CPU model (tools/models/png_model.py) on the plan's edge
shapes; and the new kernels' compile report."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import png_files as pf
from tools.models import png_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_png_index_batch", "libdeflate_amd_png_out_sizes",
           "libdeflate_amd_png_decode_batch")
KERNELS = ["lda_png_index_kernel", "lda_png_gather_kernel", "lda_png_unfilter_kernel",
           "lda_png_final_kernel"]
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
    from libdeflate_amd import api, binding
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", _header(), re.M))
    assert set(SYMBOLS) <= declared
    assert set(SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    assert len(lib.libdeflate_amd_png_index_batch.argtypes) == 8
    assert len(lib.libdeflate_amd_png_out_sizes.argtypes) == 7
    assert len(lib.libdeflate_amd_png_decode_batch.argtypes) == 14
    assert lib.libdeflate_amd_png_decode_batch.argtypes[10] is ctypes.c_uint32   # flags
    assert not binding.MISSING
    for name in ("index_png_batch", "decode_png_batch"):
        assert callable(getattr(api.Decompressor, name))
    assert callable(api.png_out_sizes) and callable(api.png_shapes)


def test_constants_match_the_header():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name}\s+(\w+)", text).group(1), 0)
    assert define("LIBDEFLATE_AMD_PNG_UNSUPPORTED") == binding.PNG_UNSUPPORTED == 18
    assert define("LIBDEFLATE_AMD_PNG_UNSUPPORTED") == define("LIBDEFLATE_AMD_ZIP_UNSUPPORTED") \
        == define("LIBDEFLATE_AMD_TAR_UNSUPPORTED")
    assert define("LIBDEFLATE_AMD_PNG_WORDS") == binding.PNG_WORDS == 8
    assert define("LIBDEFLATE_AMD_PNG_LE16") == binding.PNG_LE16 == 1
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert define("LDA_PNG_UNSUPPORTED", k) == 18 and define("LDA_PNG_WORDS", k) == 8
    assert define("LDA_PNG_META_LE16", k) == 1 << 8
    plan = open(os.path.join(CSRC, "png_plan.h")).read()
    assert re.search(r"PNG_UNSUPPORTED = 18,", plan) and re.search(r"PNG_ROW_WORDS = 8,", plan)
    assert (pm.UNSUPPORTED, pm.WORDS, pm.LE16) == (18, 8, 1)
    assert pf.UNSUPPORTED == 18
    # the plan is free of HIP
    assert "hip/" not in plan and "__device__" not in plan and "__global__" not in plan


def _good_rows():
    """two files one behind the other in a buffer of in_nbytes bytes"""
    a = pf.make(5, 3, 8, 2, seed=1)
    b = pf.make(9, 4, 4, 3, seed=2, trns=bytes(5))
    buf = b"ab" + a.data + b"c" + b.data
    rows = [pm.index(buf, 2, len(a.data)), pm.index(buf, 3 + len(a.data), len(b.data))]
    assert [r[0] for r in rows] == [0, 0]
    return np.array([r[1] for r in rows], dtype=np.uint64), len(buf)


def test_calls_check_their_arguments(lib):
    """LIBDEFLATE_AMD_BAD_ARG before any device work, with a reason: a NULL
    argument, n_files above 2^28; and for a decode a bad out_align, an unknown
    flag, in_nbytes above 2^36, a sel at or above entries, every way a row can
    fail to lie inside in_nbytes or to be a valid IHDR, and a selection that
    needs more than out_avail."""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    idx = lib.libdeflate_amd_png_index_batch
    dec = lib.libdeflate_amd_png_decode_batch
    siz = lib.libdeflate_amd_png_out_sizes

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
    refused(idx(None, 1, d, d, d, d, d, None), "NULL")
    refused(idx(fake, 1, None, d, d, d, d, None), "NULL")
    refused(idx(fake, 1, d, None, d, d, d, None), "NULL")
    refused(idx(fake, 1, d, d, None, d, d, None), "NULL")
    refused(idx(fake, 1, d, d, d, None, d, None), "NULL")
    refused(idx(fake, 1, d, d, d, d, None, None), "NULL")
    refused(idx(fake, (1 << 28) + 1, d, d, d, d, d, None), "n_files")
    assert "png_index_batch" in binding.last_error()
    assert idx(fake, 0, None, None, None, None, None, None) == 0    # nothing to do

    rows, n = _good_rows()
    rp = rows.ctypes.data_as(ctypes.c_void_p)

    def sel(*s):
        a = np.array(s, dtype=np.uint64)
        return a, a.ctypes.data_as(ctypes.c_void_p)
    a, sp = sel(0, 1)
    need = 5 * 3 * 3 + 5 * 4
    refused(dec(None, d, n, rp, 2, 2, sp, d, 4096, 1, 0, None, d, None), "NULL")
    refused(dec(fake, None, n, rp, 2, 2, sp, d, 4096, 1, 0, None, d, None), "NULL")
    refused(dec(fake, d, n, None, 2, 2, sp, d, 4096, 1, 0, None, d, None), "NULL")
    refused(dec(fake, d, n, rp, 2, 2, None, d, 4096, 1, 0, None, d, None), "NULL")
    refused(dec(fake, d, n, rp, 2, 2, sp, None, 4096, 1, 0, None, d, None), "NULL")
    refused(dec(fake, d, n, rp, 2, 2, sp, d, 4096, 1, 0, None, None, None), "NULL")
    for align in (0, 3, 24, 512, 1 << 20):
        refused(dec(fake, d, n, rp, 2, 2, sp, d, 4096, align, 0, None, d, None), "out_align")
        refused(siz(rp, 2, 2, sp, align, d, None), "out_align")
    for flags in (2, 3, 0x80000000):
        refused(dec(fake, d, n, rp, 2, 2, sp, d, 4096, 1, flags, None, d, None), "flags")
    refused(dec(fake, d, (1 << 36) + 1, rp, 2, 2, sp, d, 4096, 1, 0, None, d, None), "in_nbytes")
    refused(dec(fake, d, n, rp, 2, 2, sp, d, need - 1, 1, 0, None, d, None), "out_avail")
    refused(dec(fake, d, n, rp, 2, 2, sp, d, 64 + 20 - 1, 64, 1, None, d, None), "out_avail")
    refused(dec(fake, d, n - 1, rp, 2, 2, sp, d, 4096, 1, 0, None, d, None), "in_nbytes")
    assert "row 1" in binding.last_error()
    a, sp = sel(1, 2)
    refused(dec(fake, d, n, rp, 2, 2, sp, d, 4096, 1, 0, None, d, None), "sel[1] = 2")
    refused(siz(rp, 2, 2, sp, 1, d, None), "sel[1] = 2")
    a, sp = sel(1)
    r1 = [int(x) for x in rows[1]]
    end = r1[0] + r1[1]
    for col, value, word in ((0, n + 1, "file"), (1, n, "file"),
                             (2, 4 << 32, "width"), (2, 9, "width"), (2, 1 << 31 | 4 << 32, "width"),
                             (3, r1[3] & ~0xFF | 16, "bit depth"), (3, r1[3] & ~0xFF00 | 7 << 8, "bit depth"),
                             (3, r1[3] | 1 << 16, "interlaced"), (3, r1[3] ^ 3 << 24, "filter unit"),
                             (3, r1[3] ^ 3 << 32, "channel"),
                             (4, r1[0] + 32, "IDAT"), (4, end - 11, "IDAT"),
                             (5, end - 12 - r1[4] + 1, "IDAT"),
                             (6, 0, "PLTE"), (6, r1[6] & (1 << 48) - 1 | 257 << 48, "PLTE"),
                             (6, end - 3 | 1 << 48, "PLTE"), (6, r1[0] + 8 | 1 << 48, "PLTE"),
                             (7, end + 1, "tRNS"), (7, end - 4 | 1 << 48, "tRNS")):
        bad = rows.copy()
        bad[1, col] = value
        bp = bad.ctypes.data_as(ctypes.c_void_p)
        refused(dec(fake, d, n, bp, 2, 1, sp, d, 1 << 40, 1, 0, None, d, None), word)
        assert "row 1" in binding.last_error()
        if col in (2, 3):
            refused(siz(bp, 2, 1, sp, 1, d, None), word)
    big = rows.copy()
    big[1, 2] = 65536 | 65536 << 32
    big[1, 3] = 8 | 6 << 8 | 4 << 24 | 4 << 32
    bp = big.ctypes.data_as(ctypes.c_void_p)
    refused(dec(fake, d, n, bp, 2, 1, sp, d, 1 << 40, 1, 0, None, d, None), "2^32")
    refused(siz(bp, 2, 1, sp, 1, d, None), "2^32")
    refused(siz(None, 2, 1, sp, 1, d, None), "NULL")
    refused(siz(rp, 2, 1, None, 1, d, None), "NULL")
    refused(siz(rp, 2, 1, sp, 1, None, None), "NULL")
    # nothing selected: nothing to do, and the offsets say so
    offs = np.full(1, 77, dtype=np.uint64)
    assert dec(fake, d, n, rp, 2, 0, None, d, 0, 1, 0, offs.ctypes.data_as(ctypes.c_void_p),
               None, None) == 0
    assert offs[0] == 0


def test_out_sizes_and_shapes_are_the_models(lib):
    """libdeflate_amd_png_out_sizes (no device) on the model's rows of the
    plan's edge shapes - heights and rowbytes around the band and the 16-byte
    piece, all 15 depth and colour pairs, the largest image below 2^32 raw
    bytes - with failed files among them, a selection out of order and with
    duplicates, for every alignment"""
    from libdeflate_amd import api
    files = [pf.make(w, h, 8, 0, seed=w + h, filters=0).data
             for h in (1, 63, 64, 65, 130) for w in (1, 15, 16, 17, 33)]
    files += [pf.make(67, 65, d, c, seed=d, filters=0).data for d, c in pm.COMBOS]
    files += [data for data, _ in pf.defects().values()][:6]
    # (only the header of the largest one is there: the index needs no more)
    files.append(pm.SIGNATURE + pf.ihdr(65535, 16384, 8, 6) + pf.chunk(b"IDAT", b"x") +
                 pf.chunk(b"IEND"))
    results = [pm.index(f) for f in files]
    rows = [r[1] for r in results]
    assert results[-1][0] == 0 and sum(r[0] != 0 for r in results) == 6
    shapes = api.png_shapes(rows)
    assert shapes == [tuple(pm.shape(r)) for r in rows]
    assert shapes[-1] == (16384, 65535, 4, 8, 6) and shapes[-2] == (0, 0, 0, 0, 0)
    rng = np.random.RandomState(5)
    sel = list(rng.permutation(len(rows))) + [0, 0, len(rows) - 1, 3]
    for align in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        offs, total = api.png_out_sizes(rows, sel, align)
        want = pm.out_sizes(rows, sel, align)
        assert offs.tolist() == want and total == want[-1]
    offs, total = api.png_out_sizes(rows, [], 1)
    assert offs.tolist() == [0] and total == 0


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "png_kernels.hip", "-o", os.devnull],
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
    # the gather's chunk head; the unfilter keeps its pieces in registers
    assert lds == [0, 8, 0, 0], lds
    # several waves per SIMD for the unfilter (DESIGN 3.20 quotes the figure)
    assert occ[2] >= 4, occ
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    src = open(os.path.join(CSRC, "png_kernels.hip")).read()
    for name in KERNELS:
        assert re.search(rf"^{name}\(", k, re.M) and re.search(rf"^{name}\(", src, re.M)
    assert '#include "tar_copy.h"' in src and "copy_tile(" in src
