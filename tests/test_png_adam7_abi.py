"""CPU-side checks of the PNG reader's calls that take Adam7-interlaced files:
the three calls declared, exported and bound, with the flag's value everywhere
it is copied; every argument they refuse, refused before any device is touched
and with a reason; png_out_sizes_ex and the shape helpers against the CPU model
(tools/models/png_adam7.py); the new kernels' compile report; and the plan
header free of HIP."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import png_adam7_files as p7
from tests import png_files as pf
from tools.models import png_adam7 as m7
from tools.models import png_model as pm
from tools.models import png_pixels_model as px

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_png_index_batch_ex", "libdeflate_amd_png_out_sizes_ex",
           "libdeflate_amd_png_decode_batch_ex")
KERNELS = ["lda_png7_deinterlace_kernel", "lda_png7_final_kernel"]
BAD_ARG = -2
ADAM7 = 2


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
    assert len(lib.libdeflate_amd_png_index_batch_ex.argtypes) == 9
    assert len(lib.libdeflate_amd_png_out_sizes_ex.argtypes) == 9
    assert len(lib.libdeflate_amd_png_decode_batch_ex.argtypes) == 15
    assert lib.libdeflate_amd_png_index_batch_ex.argtypes[5] is ctypes.c_uint32     # flags
    assert lib.libdeflate_amd_png_out_sizes_ex.argtypes[4] is ctypes.c_uint32       # format
    assert lib.libdeflate_amd_png_out_sizes_ex.argtypes[6] is ctypes.c_uint32       # flags
    assert lib.libdeflate_amd_png_decode_batch_ex.argtypes[7] is ctypes.c_uint32    # format
    assert lib.libdeflate_amd_png_decode_batch_ex.argtypes[11] is ctypes.c_uint32   # flags
    assert not binding.MISSING
    for name in ("index_png_batch_ex", "decode_png_batch_ex"):
        assert callable(getattr(api.Decompressor, name))
    assert callable(api.png_out_sizes_ex)


def test_the_flag_is_2_everywhere():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name}\s+(\w+)", text).group(1), 0)
    assert define("LIBDEFLATE_AMD_PNG_ADAM7") == binding.PNG_ADAM7 == m7.ADAM7 == ADAM7
    assert define("LIBDEFLATE_AMD_PNG_ADAM7") & define("LIBDEFLATE_AMD_PNG_LE16") == 0
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert define("LDA_PNG_ADAM7", k) == 2
    plan = open(os.path.join(CSRC, "png_adam7_plan.h")).read()
    assert re.search(r"PNG_ADAM7 = 2,", plan)
    assert define("LDA_PNG7_TILE", k) == m7.TILE == int(re.search(r"PNG7_TILE = (\d+),", plan).group(1))
    assert define("LDA_PNG7_KIND_ALT", k) == int(re.search(r"PNG7_KIND_ALT = (\w+)", plan).group(1), 0)
    # the plan is free of HIP
    assert "hip/" not in plan and "__device__" not in plan and "__global__" not in plan


def _rows():
    """an interlaced and a plain file one behind the other -> (rows, in_nbytes)"""
    a = p7.make7(5, 3, 8, 2, seed=1)
    b = pf.make(9, 4, 4, 3, seed=2, trns=bytes(5))
    buf = b"ab" + a.data + b"c" + b.data
    rows = [m7.index(buf, 2, len(a.data), ADAM7), m7.index(buf, 3 + len(a.data), len(b.data), ADAM7)]
    assert [r[0] for r in rows] == [0, 0] and rows[0][1][3] >> 16 & 0xFF == 1
    return np.array([r[1] for r in rows], dtype=np.uint64), len(buf)


def test_calls_check_their_arguments(lib):
    """LIBDEFLATE_AMD_BAD_ARG before any device work, with a reason, on a
    stand-in object: NULL arguments, unknown flags, an interlaced row without
    the flag, a format that is none, out_avail one byte short, in_nbytes, a bad
    out_align, a sel at or above entries, and a row that is no image"""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    idx = lib.libdeflate_amd_png_index_batch_ex
    dec = lib.libdeflate_amd_png_decode_batch_ex
    siz = lib.libdeflate_amd_png_out_sizes_ex

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
    refused(idx(None, 1, d, d, d, ADAM7, d, d, None), "NULL")
    refused(idx(fake, 1, None, d, d, ADAM7, d, d, None), "NULL")
    refused(idx(fake, 1, d, None, d, ADAM7, d, d, None), "NULL")
    refused(idx(fake, 1, d, d, None, ADAM7, d, d, None), "NULL")
    refused(idx(fake, 1, d, d, d, ADAM7, None, d, None), "NULL")
    refused(idx(fake, 1, d, d, d, ADAM7, d, None, None), "NULL")
    for flags in (1, 3, 4, 0x80000002):
        refused(idx(fake, 1, d, d, d, flags, d, d, None), "flags")
    refused(idx(fake, (1 << 28) + 1, d, d, d, ADAM7, d, d, None), "n_files")
    assert "png_index_batch_ex" in binding.last_error()
    assert idx(fake, 0, None, None, None, ADAM7, None, None, None) == 0     # nothing to do

    rows, n = _rows()
    rp = rows.ctypes.data_as(ctypes.c_void_p)

    def sel(*s):
        a = np.array(s, dtype=np.uint64)
        return a, a.ctypes.data_as(ctypes.c_void_p)
    a, sp = sel(0, 1)
    need = 5 * 3 * 3 + 5 * 4
    for fmt in (0, px.RGB):
        refused(dec(None, d, n, rp, 2, 2, sp, fmt, d, 4096, 1, ADAM7, None, d, None), "NULL")
        refused(dec(fake, None, n, rp, 2, 2, sp, fmt, d, 4096, 1, ADAM7, None, d, None), "NULL")
        refused(dec(fake, d, n, None, 2, 2, sp, fmt, d, 4096, 1, ADAM7, None, d, None), "NULL")
        refused(dec(fake, d, n, rp, 2, 2, None, fmt, d, 4096, 1, ADAM7, None, d, None), "NULL")
        refused(dec(fake, d, n, rp, 2, 2, sp, fmt, None, 4096, 1, ADAM7, None, d, None), "NULL")
        refused(dec(fake, d, n, rp, 2, 2, sp, fmt, d, 4096, 1, ADAM7, None, None, None), "NULL")
        for align in (0, 3, 24, 512, 1 << 20):
            refused(dec(fake, d, n, rp, 2, 2, sp, fmt, d, 4096, align, ADAM7, None, d, None),
                    "out_align")
            refused(siz(rp, 2, 2, sp, fmt, align, ADAM7, d, None), "out_align")
        for flags in (4, 7, 0x80000000):
            refused(dec(fake, d, n, rp, 2, 2, sp, fmt, d, 4096, 1, flags, None, d, None), "flags")
        for flags in (1, 3, 4):
            refused(siz(rp, 2, 2, sp, fmt, 1, flags, d, None), "flags")
        # an interlaced row without the flag: the older calls' word
        for flags in (0, 1):
            refused(dec(fake, d, n, rp, 2, 2, sp, fmt, d, 4096, 1, flags, None, d, None),
                    "interlaced")
            assert "row 0" in binding.last_error()
        refused(siz(rp, 2, 2, sp, fmt, 1, 0, d, None), "interlaced")
        refused(dec(fake, d, (1 << 36) + 1, rp, 2, 2, sp, fmt, d, 4096, 1, ADAM7, None, d, None),
                "in_nbytes")
        refused(dec(fake, d, n - 1, rp, 2, 2, sp, fmt, d, 4096, 1, ADAM7, None, d, None), "in_nbytes")
        assert "row 1" in binding.last_error()
    refused(dec(fake, d, n, rp, 2, 2, sp, 0, d, need - 1, 1, ADAM7, None, d, None), "out_avail")
    refused(dec(fake, d, n, rp, 2, 2, sp, 0, d, 64 + 20 - 1, 64, ADAM7 | 1, None, d, None),
            "out_avail")
    refused(dec(fake, d, n, rp, 2, 2, sp, px.RGBA, d, 4 * (15 + 36) - 1, 1, ADAM7, None, d, None),
            "out_avail")
    for fmt in (5, 0x10, 0x20, 0x43, 0x1F, 0x80000003):
        refused(dec(fake, d, n, rp, 2, 2, sp, fmt, d, 4096, 1, ADAM7, None, d, None), "format")
        refused(siz(rp, 2, 2, sp, fmt, 1, ADAM7, d, None), "format")
    a, sp = sel(1, 2)
    refused(dec(fake, d, n, rp, 2, 2, sp, 0, d, 4096, 1, ADAM7, None, d, None), "sel[1] = 2")
    refused(siz(rp, 2, 2, sp, 0, 1, ADAM7, d, None), "sel[1] = 2")
    a, sp = sel(0)
    r0 = [int(x) for x in rows[0]]
    end = r0[0] + r0[1]
    for col, value, word in ((0, n + 1, "file"), (1, n, "file"),
                             (2, 4 << 32, "width"), (2, 9, "width"),
                             (3, r0[3] & ~0xFF | 4, "bit depth"),
                             (3, r0[3] & ~(0xFF << 16) | 2 << 16, "interlace"),
                             (3, r0[3] ^ 1 << 24, "filter unit"), (3, r0[3] ^ 1 << 32, "channel"),
                             (4, r0[0] + 32, "IDAT"), (4, end - 11, "IDAT"),
                             (5, end - 12 - r0[4] + 1, "IDAT"), (7, end + 1, "tRNS")):
        bad = rows.copy()
        bad[0, col] = value
        bp = bad.ctypes.data_as(ctypes.c_void_p)
        refused(dec(fake, d, n, bp, 2, 1, sp, 0, d, 1 << 40, 1, ADAM7, None, d, None), word)
        assert "row 0" in binding.last_error()
    # raw7 at 2^32 where the image is below it
    big = rows.copy()
    big[0, 2] = 2 | 1300000000 << 32
    big[0, 3] = 8 | 0 << 8 | 1 << 16 | 1 << 24 | 1 << 32
    bp = big.ctypes.data_as(ctypes.c_void_p)
    refused(dec(fake, d, n, bp, 2, 1, sp, 0, d, 1 << 40, 1, ADAM7, None, d, None), "2^32")
    refused(siz(bp, 2, 1, sp, 0, 1, ADAM7, d, None), "2^32")
    big[0, 3] &= ~np.uint64(1 << 16)      # its twin is an image
    offs = np.zeros(2, dtype=np.uint64)
    assert siz(bp, 2, 1, sp, 0, 1, ADAM7, offs.ctypes.data_as(ctypes.c_void_p), None) == 0
    assert offs.tolist() == [0, 2 * 1300000000]
    refused(siz(None, 2, 1, sp, 0, 1, ADAM7, d, None), "NULL")
    refused(siz(rp, 2, 1, None, 0, 1, ADAM7, d, None), "NULL")
    refused(siz(rp, 2, 1, sp, 0, 1, ADAM7, None, None), "NULL")
    # nothing selected: nothing to do, and the offsets say so
    offs = np.full(1, 77, dtype=np.uint64)
    assert dec(fake, d, n, rp, 2, 0, None, 0, d, 0, 1, ADAM7,
               offs.ctypes.data_as(ctypes.c_void_p), None, None) == 0
    assert offs[0] == 0


def test_out_sizes_and_shapes_are_the_models(lib):
    """libdeflate_amd_png_out_sizes_ex (no device) on the model's rows:
    interlaced and plain files of all 15 pairs, failed files among them, a
    selection out of order and with duplicates, every alignment, format 0 and
    pixel formats; with flags 0 the older calls' offsets for plain rows; the
    shape helpers give an interlaced row the shape of its twin"""
    from libdeflate_amd import api
    files, twins = [], []
    for k, (depth, colour) in enumerate(pm.COMBOS):
        g = p7.make7(9 + k, 7 + k % 3, depth, colour, seed=k, filters=0)
        files += [g.data, pf.make(5 + k, 3, depth, colour, seed=k, filters=0).data]
        twins += [pf.make(g.width, g.height, depth, colour, pixels=g.pixels, filters=0).data,
                  files[-1]]
    files += [data for data, _ in pf.defects().values()][:6]
    twins += files[-6:]
    rows = [m7.index(f, flags=ADAM7)[1] for f in files]
    trows = [pm.index(f)[1] for f in twins]
    assert sum(pm.is_zero(r) for r in rows) == 6
    assert api.png_shapes(rows) == api.png_shapes(trows) == [tuple(pm.shape(r)) for r in trows]
    for fmt in (px.RGB, px.GRAY | px.OUT16):
        assert api.png_pixels_shapes(rows, fmt) == api.png_pixels_shapes(trows, fmt)
    rng = np.random.RandomState(5)
    sel = list(rng.permutation(len(rows))) + [0, 0, len(rows) - 1, 3]
    plain = [k for k in sel if not m7.is_interlaced(rows[k])]
    for align in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        for fmt in (0, px.GRAY, px.RGBA | px.OUT16):
            offs, total = api.png_out_sizes_ex(rows, sel, fmt, align, ADAM7)
            want = m7.out_sizes(rows, sel, fmt, align)
            assert offs.tolist() == want and total == want[-1]
            # the twins through the older call
            old = api.png_pixels_out_sizes(trows, sel, fmt, align) if fmt else \
                api.png_out_sizes(trows, sel, align)
            assert offs.tolist() == old[0].tolist() and total == old[1]
            offs, total = api.png_out_sizes_ex(rows, plain, fmt, align, 0)
            old = api.png_pixels_out_sizes(rows, plain, fmt, align) if fmt else \
                api.png_out_sizes(rows, plain, align)
            assert offs.tolist() == old[0].tolist() and total == old[1]
    offs, total = api.png_out_sizes_ex(rows, [], 0, 1, ADAM7)
    assert offs.tolist() == [0] and total == 0
    with pytest.raises(Exception):
        api.png_out_sizes_ex(rows, [0], 0, 1, 0)


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "png_adam7_kernels.hip", "-o", os.devnull],
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
    assert lds == [0, 0], lds
    # a memory-bound gather wants waves to hide its loads (DESIGN 3.23 quotes the figure)
    assert occ[0] >= 4, occ
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    src = open(os.path.join(CSRC, "png_adam7_kernels.hip")).read()
    for name in KERNELS:
        assert re.search(rf"^{name}\(", k, re.M) and re.search(rf"^{name}\(", src, re.M)
    # the index kernel took its flags argument without growing out of registers
    # (tests/test_png_abi.py reads png_kernels.hip's report)
    assert re.search(r"^lda_png_index_kernel\(uint64_t n_files, uint32_t flags,", k, re.M)
