"""CPU-side checks of the tar reader: the four calls declared, exported and
bound with the header's constants; arguments refused before any device is
touched; the CPU model of the whole rule (tools/models/tar_walk.py) against
Python's tarfile on every good file (tests/tar_files.py), and its verdicts on
the defect and limit files; and the new kernels' compile report."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import tar_files as tf
from tools.models import tar_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_tar_index_batch", "libdeflate_amd_tar_extract_batch",
           "libdeflate_amd_tar_read_batch", "libdeflate_amd_tar_ranges")
KERNELS = ["lda_tar_scan_kernel", "lda_tar_walk_kernel", "lda_tar_resolve_kernel",
           "lda_tar_desc_kernel", "lda_tar_copy_kernel", "lda_tar_final_kernel"]
BAD_ARG = -2
SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
MORE_RECORDS, MORE_CANDIDATES, UNSUPPORTED = 16, 17, 18


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
    assert len(lib.libdeflate_amd_tar_index_batch.argtypes) == 9
    assert len(lib.libdeflate_amd_tar_extract_batch.argtypes) == 11
    assert len(lib.libdeflate_amd_tar_read_batch.argtypes) == 13
    assert len(lib.libdeflate_amd_tar_ranges.argtypes) == 6
    assert not binding.MISSING
    for name in ("index_tar_batch", "extract_tar_batch", "read_tar_batch", "read_targz",
                 "read_targz_entries"):
        assert callable(getattr(api.Decompressor, name))
    assert callable(api.tar_entry_names) and callable(api.tar_ranges)


def test_constants_match_the_header():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name}\s+(\d+)", text).group(1))
    assert define("LIBDEFLATE_AMD_TAR_MORE_RECORDS") == binding.TAR_MORE_RECORDS == 16
    assert define("LIBDEFLATE_AMD_TAR_MORE_RECORDS") == define("LIBDEFLATE_AMD_ZIP_MORE_ENTRIES")
    assert define("LIBDEFLATE_AMD_TAR_MORE_CANDIDATES") == binding.TAR_MORE_CANDIDATES == 17
    assert define("LIBDEFLATE_AMD_TAR_UNSUPPORTED") == binding.TAR_UNSUPPORTED == 18
    assert define("LIBDEFLATE_AMD_TAR_RESULT_WORDS") == binding.TAR_RESULT_WORDS == 5
    assert define("LIBDEFLATE_AMD_TAR_WORDS") == binding.TAR_WORDS == 8
    assert define("LIBDEFLATE_AMD_TAR_SLACK") == binding.TAR_SLACK == 1024
    assert define("LIBDEFLATE_AMD_TAR_EOF") == binding.TAR_EOF == 1
    assert define("LIBDEFLATE_AMD_TAR_HAS_L") == binding.TAR_HAS_L == 2
    assert define("LIBDEFLATE_AMD_TAR_HAS_PAX") == binding.TAR_HAS_PAX == 4
    # the device side's copies (kernels.h), the plan's and the model's are the header's
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert define("LDA_TAR_MORE_RECORDS", k) == define("LDA_BR_MORE", k) == 16
    assert define("LDA_TAR_MORE_CANDIDATES", k) == 17
    assert define("LDA_TAR_UNSUPPORTED", k) == 18
    assert define("LDA_TAR_RESULT_WORDS", k) == 5
    assert define("LDA_TAR_WORDS", k) == 8
    assert (define("LDA_TAR_EOF", k), define("LDA_TAR_HAS_L", k), define("LDA_TAR_HAS_PAX", k)) == \
        (tar_walk.EOF, tar_walk.HAS_L, tar_walk.HAS_PAX) == (1, 2, 4)
    assert define("LDA_TAR_EXT_MAX", k) == tar_walk.EXT_MAX == 8
    assert define("LDA_TAR_EXT_BYTES", k) == tar_walk.EXT_BYTES == 1 << 20
    assert define("LDA_TAR_COPY_TILE", k) == tar_walk.COPY_TILE == tf.TILE == 65536
    assert define("LDA_TAR_SCAN_BLOCKS", k) * 512 == define("LDA_BR_SCAN_WG", k)
    assert (define("LDA_TAR_NAME_HEADER", k), define("LDA_TAR_NAME_L", k),
            define("LDA_TAR_NAME_PAX", k)) == \
        (tar_walk.NAME_HEADER, tar_walk.NAME_L, tar_walk.NAME_PAX)
    plan = open(os.path.join(CSRC, "tar_plan.h")).read()
    assert re.search(r"TAR_UNSUPPORTED = 18,", plan) and re.search(r"TAR_ROW_WORDS = 8,", plan)
    assert re.search(r"TAR_COPY_TILE = 65536,", plan)
    assert (tar_walk.MORE_RECORDS, tar_walk.MORE_CANDIDATES, tar_walk.UNSUPPORTED) == (16, 17, 18)
    assert (tar_walk.RESULT_WORDS, tar_walk.WORDS, tar_walk.SLACK) == (5, 8, 1024)
    assert (tf.MORE_RECORDS, tf.MORE_CANDIDATES, tf.UNSUPPORTED) == (16, 17, 18)


def test_calls_check_their_arguments(lib):
    """Refused before any device is touched, with a reason: a NULL object or
    pointer (d_out only with out_avail != 0, d_in only with in_nbytes != 0,
    d_index never), max_records == 0 or above 2^28, in_nbytes above 2^36, an
    out_align that is no power of two in 1 .. 256; and for a selection the
    rows, the entry numbers and the room."""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    ext = lib.libdeflate_amd_tar_extract_batch
    idx = lib.libdeflate_amd_tar_index_batch
    rd = lib.libdeflate_amd_tar_read_batch
    rg = lib.libdeflate_amd_tar_ranges

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
    refused(ext(None, d, 1024, 1, d, 64, 1, d, None, d, None), "NULL")
    refused(ext(fake, None, 1024, 1, d, 64, 1, d, None, d, None), "NULL")
    refused(ext(fake, d, 1024, 1, None, 64, 1, d, None, d, None), "NULL")
    refused(ext(fake, d, 1024, 1, d, 64, 1, None, None, d, None), "NULL")
    refused(ext(fake, d, 1024, 1, d, 64, 1, d, None, None, None), "NULL")
    refused(ext(fake, d, 1024, 0, d, 64, 1, d, None, d, None), "max_records")
    refused(ext(fake, d, 1024, (1 << 28) + 1, d, 64, 1, d, None, d, None), "max_records")
    refused(ext(fake, d, (1 << 36) + 1, 1, d, 64, 1, d, None, d, None), "in_nbytes")
    for align in (0, 3, 24, 512, 1 << 20):
        refused(ext(fake, d, 1024, 1, d, 64, align, d, None, d, None), "out_align")
        refused(idx(fake, d, 1024, 1, align, d, None, d, None), "out_align")
    assert "tar_index_batch" in binding.last_error()
    refused(idx(None, d, 1024, 1, 1, d, None, d, None), "NULL")
    refused(idx(fake, None, 1024, 1, 1, d, None, d, None), "NULL")
    refused(idx(fake, d, 1024, 1, 1, None, None, d, None), "NULL")
    refused(idx(fake, d, 1024, 1, 1, d, None, None, None), "NULL")
    refused(idx(fake, d, 1024, 0, 1, d, None, d, None), "max_records")
    refused(idx(fake, d, 1024, (1 << 28) + 1, 1, d, None, d, None), "max_records")
    refused(idx(fake, d, (1 << 36) + 1, 1, 1, d, None, d, None), "in_nbytes")
    # a selection: rows of a file of 4096 bytes
    rows = np.array([[0, 0, 5, 0x30, 512, 500, 7, 0],
                     [1024, 1024, 4 | 3 << 32, 0x30, 1536, 30, 7, 500]], dtype=np.uint64)
    rp = rows.ctypes.data_as(ctypes.c_void_p)

    def sel(*s):
        a = np.array(s, dtype=np.uint64)
        return a, a.ctypes.data_as(ctypes.c_void_p)
    a, sp = sel(0, 1)
    refused(rd(None, d, 4096, rp, 2, 2, sp, d, 4096, 1, None, d, None), "NULL")
    refused(rd(fake, None, 4096, rp, 2, 2, sp, d, 4096, 1, None, d, None), "NULL")
    refused(rd(fake, d, 4096, None, 2, 2, sp, d, 4096, 1, None, d, None), "NULL")
    refused(rd(fake, d, 4096, rp, 2, 2, None, d, 4096, 1, None, d, None), "NULL")
    refused(rd(fake, d, 4096, rp, 2, 2, sp, None, 4096, 1, None, d, None), "NULL")
    refused(rd(fake, d, 4096, rp, 2, 2, sp, d, 4096, 1, None, None, None), "NULL")
    refused(rd(fake, d, 4096, rp, 2, 2, sp, d, 4096, 48, None, d, None), "out_align")
    refused(rd(fake, d, (1 << 36) + 1, rp, 2, 2, sp, d, 4096, 1, None, d, None), "in_nbytes")
    refused(rd(fake, d, 4096, rp, 2, 2, sp, d, 529, 1, None, d, None), "out_avail")
    refused(rd(fake, d, 4096, rp, 2, 2, sp, d, 530 + 13, 16, None, d, None), "out_avail")
    refused(rd(fake, d, 1565, rp, 2, 2, sp, d, 4096, 1, None, d, None), "in_nbytes")
    refused(rd(fake, d, 1011, rp, 2, 1, sp, d, 4096, 1, None, d, None), "in_nbytes")
    a, sp = sel(1, 2)
    refused(rd(fake, d, 4096, rp, 2, 2, sp, d, 4096, 1, None, d, None), "sel[1] = 2")
    refused(rg(rp, 2, 2, sp, d, None), "sel[1] = 2")
    a, sp = sel(0)
    for col, value, word in ((5, 1 << 36, "2^36"), (0, 7, "header"), (4, 1024, "data"),
                             (3, 1 << 16, "typeflag"), (2, 5 | 156 << 32, "name")):
        bad = rows.copy()
        bad[0, col] = value
        bp = bad.ctypes.data_as(ctypes.c_void_p)
        refused(rd(fake, d, 1 << 36, bp, 2, 1, sp, d, 1 << 40, 1, None, d, None), word)
        refused(rg(bp, 2, 1, sp, d, None), word)
    refused(rg(None, 2, 1, sp, d, None), "NULL")
    refused(rg(rp, 2, 1, None, d, None), "NULL")
    refused(rg(rp, 2, 1, sp, None, None), "NULL")
    # nothing selected: nothing to do, and the offsets say so
    offs = np.full(1, 77, dtype=np.uint64)
    assert rd(fake, d, 4096, rp, 2, 0, None, d, 0, 1, offs.ctypes.data_as(ctypes.c_void_p), None,
              None) == 0
    assert offs[0] == 0


def test_ranges_are_the_models(lib):
    """libdeflate_amd_tar_ranges (no device) on the model's rows of a good
    file, a selection out of order and with duplicates; an S row gives 0"""
    from libdeflate_amd import api
    g = tf.good("unsupported")
    r = tar_walk.read(g.data, 64)
    sel = [3, 0, 8, 5, 5, 0]
    rng, total = api.tar_ranges(r.rows, sel)
    want, wtotal = tar_walk.ranges(r.rows, sel)
    assert rng.tolist() == [list(x) for x in want] and total == wtotal
    assert (r.rows[5][3] & 0xFF) == ord("S") and rng[3].tolist() == [r.rows[5][4], 0]


# ---- the CPU model against tarfile ----

@pytest.mark.parametrize("name", tf.GOOD_NAMES + tf.BIG_NAMES)
def test_model_reads_every_good_file_as_tarfile_does(name):
    """entry count, names (tarfile strips a directory's trailing '/': both
    sides are compared stripped), offset_data, sizes, mtimes and the bytes of
    every entry; out_off for out_align 1, 8 and 256"""
    g = tf.good(name)
    model = tar_walk.read(g.data, 4096)
    w = tar_walk.walk(g.data)
    assert w.ok and set(w.records) <= set(tar_walk.candidates(g.data))
    if not g.readable:
        return
    exp = tf.expected(g)
    assert model.words[0] == SUCCESS and model.words[1] == len(exp)
    at = 0
    for (ti, data), row, plain, res in zip(exp, model.rows, model.plain, model.results):
        got = tar_walk.name_of(g.data, row).decode("utf-8", "surrogateescape")
        assert got.rstrip("/") == ti.name.rstrip("/")
        # (tarfile's offset is that of the first extension record: the row
        # holds the entry's own header, the block in front of its data)
        assert (row[0], row[4], row[6]) == (ti.offset_data - 512, ti.offset_data, int(ti.mtime))
        assert ti.offset <= row[0]
        assert row[3] & 0xFF == ti.type[0] and res == SUCCESS
        assert row[5] == (ti.size if data is not None else 0) and row[7] == at
        assert plain == (data or b"")
        at += row[5]
    assert model.words[3] == at
    for align in (8, 256):
        ra = tar_walk.read(g.data, 4096, out_align=align, extract=False)
        at = 0
        for k, row in enumerate(ra.rows):
            assert row[7] == at and row[:7] == model.rows[k][:7]
            at += -(-row[5] // align) * align
        assert ra.words == model.words[:3] + [at, model.words[4]]


def test_model_lookalikes_and_endings():
    """the nested archive's headers are candidates and no records; the four
    endings give the same entries and differ in the flag and the end offset"""
    for fmt in tf.FORMATS:
        m = tf.mixed(fmt)
        w = tar_walk.walk(m.data)
        cands = tar_walk.candidates(m.data)
        assert len(cands) == len(w.records) + 4 and w.eof
        base = tar_walk.read(m.data, 64)
        end = base.words[2]
        for g, eof, n in ((tf.cut(fmt), 0, end), (tf.one_zero(fmt), 1, end + 512),
                          (tf.garbage(fmt), 1, None)):
            r = tar_walk.read(g.data, 64)
            assert r.rows == base.rows and r.words[:4] == base.words[:4]
            assert r.words[4] == (base.words[4] & ~1) | eof
            assert n is None or len(g.data) == n
    assert tar_walk.read(tf.empty().data, 1).words == [SUCCESS, 0, 0, 0, 1]
    nb = tf.nested_big()
    assert len(tar_walk.candidates(nb.data)) == 1102 and len(tar_walk.walk(nb.data).records) == 2


def test_model_limits_and_precedence():
    g = tf.mixed("gnu")
    r = tar_walk.read(g.data, 64)
    recs = len(tar_walk.walk(g.data).records)
    assert recs > r.words[1]                # extension records count as records
    assert tar_walk.read(g.data, recs - 1).words == [MORE_RECORDS, recs, 0, 0, 0]
    assert tar_walk.read(g.data, recs).words == r.words
    total = r.words[3]
    short = tar_walk.read(g.data, recs, out_avail=total - 1)
    assert short.words == [INSUFFICIENT_SPACE] + r.words[1:] and short.rows == r.rows
    assert short.plain is None
    assert tar_walk.read(g.data, recs, out_avail=total).words[0] == SUCCESS
    nb = tf.nested_big()
    k = len(tar_walk.candidates(nb.data))
    for mm in (2, k - 1024 - 1):
        assert tar_walk.read(nb.data, mm).words == [MORE_CANDIDATES, k, 0, 0, 0]
    assert tar_walk.read(nb.data, k - 1024).words[:2] == [SUCCESS, 2]
    for n in (0, 511):
        assert tar_walk.read(g.data[:n], 4).words == [BAD_DATA, 0, 0, 0, 0]
    for d in tf.defects():
        assert tar_walk.read(d.data, 64).words == [BAD_DATA, 0, 0, 0, 0], d.name
    u = tar_walk.read(tf.unsupported().data, 64)
    assert u.results == [0, 18, 0, 18, 0, 18, 0, 18, 0] and u.words[0] == UNSUPPORTED
    names = [tar_walk.name_of(tf.unsupported().data, row) for row in u.rows]
    assert names == [b"n0", b"nine", b"n1", b"sized", b"n2", b"sparse", b"pax/named", b"badpax",
                     b"n4"]
    assert [row[5] for row, res in zip(u.rows, u.results) if res] == [0, 0, 0, 0]


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "tar_kernels.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == KERNELS
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", rep)]
    sspills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", rep)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", rep)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", rep)]
    assert spills == [0] * len(KERNELS), spills
    assert sspills == [0] * len(KERNELS), sspills
    assert scratch == [0] * len(KERNELS), scratch
    # the scan's two words per block and four wave sums; the final kernel's
    # first-failure word
    assert lds == [32 * 4 + 32 * 4 + 16, 0, 0, 0, 0, 8], lds
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert [x for x in KERNELS if f"\n{x}(" not in k] == []
