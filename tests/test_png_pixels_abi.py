"""CPU-side checks of the PNG reader's decode to one pixel format: the two
calls declared, exported and bound with the header's constants; every argument
they refuse, refused before any device is touched and with a reason;
png_pixels_out_sizes and png_pixels_shapes against the CPU model
(tools/models/png_pixels_model.py); and the new kernels' compile report."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import png_files as pf
from tools.models import png_model as pm
from tools.models import png_pixels_model as px

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_png_pixels_out_sizes", "libdeflate_amd_png_decode_pixels_batch")
KERNELS = ["lda_pngx_convert_kernel", "lda_pngx_final_kernel"]
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
    exported = set(re.findall(r" T (\w+)", out))
    assert set(SYMBOLS) <= exported and "lda_png_pixels_stages" in exported
    assert len(lib.libdeflate_amd_png_pixels_out_sizes.argtypes) == 8
    assert len(lib.libdeflate_amd_png_decode_pixels_batch.argtypes) == 15
    assert lib.libdeflate_amd_png_pixels_out_sizes.argtypes[4] is ctypes.c_uint32      # format
    assert lib.libdeflate_amd_png_decode_pixels_batch.argtypes[7] is ctypes.c_uint32   # format
    assert lib.libdeflate_amd_png_decode_pixels_batch.argtypes[11] is ctypes.c_uint32  # flags
    assert not binding.MISSING
    assert callable(api.Decompressor.decode_png_pixels_batch)
    assert callable(api.png_pixels_out_sizes) and callable(api.png_pixels_shapes)


def test_constants_match_everywhere():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name}\s+(\w+)", text).group(1), 0)
    names = ("GRAY", "GRAY_ALPHA", "RGB", "RGBA", "OUT16")
    values = [define("LIBDEFLATE_AMD_PNG_" + n) for n in names]
    assert values == [1, 2, 3, 4, 0x10]
    assert values == [getattr(binding, "PNG_" + n) for n in names]
    assert values == [getattr(px, n) for n in names]
    plan = open(os.path.join(CSRC, "png_pixels_plan.h")).read()
    for n, v in zip(names, values):
        assert int(re.search(rf"PNGX_{n} = (\w+),", plan).group(1), 0) == v
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert define("LDA_PNGX_OUT16", k) == 0x10
    assert define("LDA_PNGX_TILE", k) == px.TILE == 4096
    assert int(re.search(r"PNGX_TILE = (\d+),", plan).group(1)) == 4096
    assert define("LDA_PNGX_KIND_KEY", k) == \
        int(re.search(r"PNGX_KIND_KEY = (\w+),", plan).group(1), 0)
    assert define("LDA_PNG_META_ALT", k) == \
        int(re.search(r"PNGX_META_ALT = (\w+),", plan).group(1), 0) == 0x200
    assert define("LIBDEFLATE_AMD_PNG_LE16") == px.LE16 == binding.PNG_LE16
    # the plan is free of HIP, and extends png_plan.h
    assert "hip/" not in plan and "__device__" not in plan and "__global__" not in plan
    assert '#include "png_plan.h"' in plan and "png_row_check(" in plan


def _good_rows():
    """two files one behind the other in a buffer of in_nbytes bytes"""
    a = pf.make(5, 3, 8, 2, seed=1)
    b = pf.make(9, 4, 4, 3, seed=2, trns=bytes(5))
    buf = b"ab" + a.data + b"c" + b.data
    rows = [pm.index(buf, 2, len(a.data)), pm.index(buf, 3 + len(a.data), len(b.data))]
    assert [r[0] for r in rows] == [0, 0]
    return np.array([r[1] for r in rows], dtype=np.uint64), len(buf)


def test_calls_check_their_arguments(lib):
    """LIBDEFLATE_AMD_BAD_ARG before any device work, with a reason: a format
    that is none, an unknown flag, an interlaced row, a NULL argument, an
    out_avail one byte short, and what png_decode_batch refuses besides"""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    dec = lib.libdeflate_amd_png_decode_pixels_batch
    siz = lib.libdeflate_amd_png_pixels_out_sizes

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
    rows, n = _good_rows()
    rp = rows.ctypes.data_as(ctypes.c_void_p)

    def sel(*s):
        a = np.array(s, dtype=np.uint64)
        return a, a.ctypes.data_as(ctypes.c_void_p)
    a, sp = sel(0, 1)
    for fmt in (0, 5, 0x20, 0x13 | 0x40, 0x10, 0x113):
        refused(dec(fake, d, n, rp, 2, 2, sp, fmt, d, 4096, 1, 0, None, d, None), "format")
        assert "png_decode_pixels_batch" in binding.last_error()
        refused(siz(rp, 2, 2, sp, fmt, 1, d, None), "format")
    for flags in (2, 3, 0x80000000):
        refused(dec(fake, d, n, rp, 2, 2, sp, 3, d, 4096, 1, flags, None, d, None), "flags")
    refused(dec(None, d, n, rp, 2, 2, sp, 3, d, 4096, 1, 0, None, d, None), "NULL")
    refused(dec(fake, None, n, rp, 2, 2, sp, 3, d, 4096, 1, 0, None, d, None), "NULL")
    refused(dec(fake, d, n, None, 2, 2, sp, 3, d, 4096, 1, 0, None, d, None), "NULL")
    refused(dec(fake, d, n, rp, 2, 2, None, 3, d, 4096, 1, 0, None, d, None), "NULL")
    refused(dec(fake, d, n, rp, 2, 2, sp, 3, None, 4096, 1, 0, None, d, None), "NULL")
    refused(dec(fake, d, n, rp, 2, 2, sp, 3, d, 4096, 1, 0, None, None, None), "NULL")
    refused(siz(None, 2, 2, sp, 3, 1, d, None), "NULL")
    refused(siz(rp, 2, 2, None, 3, 1, d, None), "NULL")
    refused(siz(rp, 2, 2, sp, 3, 1, None, None), "NULL")
    for align in (0, 3, 24, 512):
        refused(dec(fake, d, n, rp, 2, 2, sp, 3, d, 4096, align, 0, None, d, None), "out_align")
        refused(siz(rp, 2, 2, sp, 3, align, d, None), "out_align")
    refused(dec(fake, d, (1 << 36) + 1, rp, 2, 2, sp, 3, d, 4096, 1, 0, None, d, None), "in_nbytes")
    # one byte short, per format and with an alignment
    for fmt in px.FORMATS:
        need = (5 * 3 + 9 * 4) * px.fmt_channels(fmt) * (px.fmt_depth(fmt) // 8)
        refused(dec(fake, d, n, rp, 2, 2, sp, fmt, d, need - 1, 1, 0, None, d, None), "out_avail")
    refused(dec(fake, d, n, rp, 2, 2, sp, 3, d, 64 + 108 - 1, 64, 0, None, d, None), "out_avail")
    refused(dec(fake, d, n - 1, rp, 2, 2, sp, 3, d, 4096, 1, 0, None, d, None), "in_nbytes")
    assert "row 1" in binding.last_error()
    a, sp = sel(1, 2)
    refused(dec(fake, d, n, rp, 2, 2, sp, 3, d, 4096, 1, 0, None, d, None), "sel[1] = 2")
    refused(siz(rp, 2, 2, sp, 3, 1, d, None), "sel[1] = 2")
    a, sp = sel(1)
    r1 = [int(x) for x in rows[1]]
    end = r1[0] + r1[1]
    for col, value, word in ((0, n + 1, "file"), (2, 4 << 32, "width"),
                             (3, r1[3] & ~0xFF | 16, "bit depth"),
                             (3, r1[3] | 1 << 16, "interlaced"), (3, r1[3] ^ 3 << 24, "filter unit"),
                             (4, r1[0] + 32, "IDAT"), (5, end - 12 - r1[4] + 1, "IDAT"),
                             (6, 0, "PLTE"), (6, end - 3 | 1 << 48, "PLTE"),
                             (7, end - 4 | 1 << 48, "tRNS")):
        bad = rows.copy()
        bad[1, col] = value
        bp = bad.ctypes.data_as(ctypes.c_void_p)
        refused(dec(fake, d, n, bp, 2, 1, sp, 4, d, 1 << 40, 1, 0, None, d, None), word)
        assert "row 1" in binding.last_error()
        if col in (2, 3):
            refused(siz(bp, 2, 1, sp, 4, 1, d, None), word)
    # nothing selected: nothing to do, and the offsets say so
    offs = np.full(1, 77, dtype=np.uint64)
    assert dec(fake, d, n, rp, 2, 0, None, 3, d, 0, 1, 0, offs.ctypes.data_as(ctypes.c_void_p),
               None, None) == 0
    assert offs[0] == 0


def test_out_sizes_and_shapes_are_the_models(lib):
    """libdeflate_amd_png_pixels_out_sizes (no device) on the model's rows: all
    15 depth and colour pairs, the largest image below 2^32 raw bytes, a 1-bit
    image whose output passes 2^32 bytes, failed files among them, a selection
    out of order and with duplicates, for every format and alignment"""
    from libdeflate_amd import api, binding
    files = [pf.make(67, 65, d, c, seed=d, filters=0).data for d, c in pm.COMBOS]
    files += [pf.make(w, 3, 2, 0, seed=w, filters=0).data for w in (1, 4, 5, 17)]
    files += [data for data, _ in pf.defects().values()][:6]
    # (only the headers of the large ones are there: the index needs no more)
    for w, h, depth, colour in ((65535, 16384, 8, 6), (1 << 17, 1 << 17, 1, 0)):
        files.append(pm.SIGNATURE + pf.ihdr(w, h, depth, colour) + pf.chunk(b"IDAT", b"x") +
                     pf.chunk(b"IEND"))
    results = [pm.index(f) for f in files]
    rows = [r[1] for r in results]
    assert results[-1][0] == 0 and results[-2][0] == 0 and sum(r[0] != 0 for r in results) == 6
    rng = np.random.RandomState(5)
    sel = list(rng.permutation(len(rows))) + [0, 0, len(rows) - 1, 3]
    for fmt in px.FORMATS:
        shapes, dtype = api.png_pixels_shapes(rows, fmt)
        want_shapes, want_dtype = px.shapes(rows, fmt)
        assert shapes == want_shapes and dtype == np.dtype(want_dtype)
        for align in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            offs, total = api.png_pixels_out_sizes(rows, sel, fmt, align)
            want = px.out_sizes(rows, sel, fmt, align)
            assert offs.tolist() == want and total == want[-1]
    offs, total = api.png_pixels_out_sizes(rows, [len(rows) - 1], binding.PNG_RGBA | binding.PNG_OUT16)
    assert total == 1 << 37
    offs, total = api.png_pixels_out_sizes(rows, [], 3)
    assert offs.tolist() == [0] and total == 0
    with pytest.raises(ValueError):
        api.png_pixels_shapes(rows, 5)


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "png_pixels_kernels.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == KERNELS
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", rep)]
    sspills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", rep)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", rep)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", rep)]
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", rep)]
    assert spills == [0, 0], spills
    assert sspills == [0, 0], sspills
    assert scratch == [0, 0], scratch
    # the palette of 256 words and at most a few words more
    assert 1024 <= lds[0] <= 1024 + 64 and lds[1] == 0, lds
    # a memory-bound kernel wants several waves per SIMD in flight
    assert occ[0] >= 4, occ
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    src = open(os.path.join(CSRC, "png_pixels_kernels.hip")).read()
    for name in KERNELS:
        assert re.search(rf"^{name}\(", k, re.M) and re.search(rf"^{name}\(", src, re.M)
    # png_kernels.hip keeps its four kernels: the new ones live here
    old = open(os.path.join(CSRC, "png_kernels.hip")).read()
    assert "lda_pngx_" not in old
