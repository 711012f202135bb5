"""CPU-side checks of the ZIP reader: the three calls declared, exported and
bound with the header's constants; arguments refused before any device is
touched; the CPU model of the whole rule (tools/models/zip_walk.py) against
Python's zipfile on every good file (tests/zip_files.py), and its verdicts,
words and per-entry results on the defect and limit files; and the new
kernels' compile report."""
import ctypes
import io
import os
import re
import struct
import subprocess
import zipfile

import numpy as np
import pytest

from tests import zip_files as zf
from tools.models import zip_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_zip_index_batch", "libdeflate_amd_zip_decompress_batch",
           "libdeflate_amd_zip_read_batch")
KERNELS = ["lda_zip_end_kernel", "lda_zip_scan_kernel", "lda_zip_size_kernel",
           "lda_zip_resolve_kernel", "lda_zip_desc_kernel", "lda_zip_copy_kernel",
           "lda_zip_final_kernel", "lda_zip_rfinal_kernel"]
BAD_ARG = -2
SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
MORE_ENTRIES, MORE_CANDIDATES, UNSUPPORTED = 16, 17, 18


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
    assert len(lib.libdeflate_amd_zip_index_batch.argtypes) == 9
    assert len(lib.libdeflate_amd_zip_decompress_batch.argtypes) == 11
    assert len(lib.libdeflate_amd_zip_read_batch.argtypes) == 13
    assert not binding.MISSING
    for name in ("index_zip_batch", "decompress_zip_batch", "read_zip_batch"):
        assert callable(getattr(api.Decompressor, name))
    assert callable(api.zip_entry_names)


def test_constants_match_the_header():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name}\s+(\d+)", text).group(1))
    assert define("LIBDEFLATE_AMD_ZIP_MORE_ENTRIES") == binding.ZIP_MORE_ENTRIES == 16
    assert define("LIBDEFLATE_AMD_ZIP_MORE_ENTRIES") == define("LIBDEFLATE_AMD_BGZF_MORE_MEMBERS")
    assert define("LIBDEFLATE_AMD_ZIP_MORE_ENTRIES") == define("LIBDEFLATE_AMD_GZM_MORE_MEMBERS")
    assert define("LIBDEFLATE_AMD_ZIP_MORE_CANDIDATES") == binding.ZIP_MORE_CANDIDATES == 17
    assert define("LIBDEFLATE_AMD_ZIP_UNSUPPORTED") == binding.ZIP_UNSUPPORTED == 18
    assert define("LIBDEFLATE_AMD_ZIP_RESULT_WORDS") == binding.ZIP_RESULT_WORDS == 5
    assert define("LIBDEFLATE_AMD_ZIP_WORDS") == binding.ZIP_WORDS == 8
    assert define("LIBDEFLATE_AMD_ZIP_SLACK") == binding.ZIP_SLACK == 1024
    assert define("LIBDEFLATE_AMD_ZIP_ZIP64") == binding.ZIP_ZIP64 == 1
    # the device side's copies (kernels.h), the plan's and the model's are the header's
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert define("LDA_ZIP_MORE_ENTRIES", k) == define("LDA_BR_MORE", k) == 16
    assert define("LDA_ZIP_MORE_CANDIDATES", k) == 17
    assert define("LDA_ZIP_UNSUPPORTED", k) == 18
    assert define("LDA_ZIP_RESULT_WORDS", k) == 5
    assert define("LDA_ZIP_WORDS", k) == 8
    assert define("LDA_ZIP_ZIP64", k) == 1
    assert define("LDA_ZIP_WINDOW", k) == zip_walk.WINDOW == 65557
    plan = open(os.path.join(CSRC, "zip_plan.h")).read()
    assert re.search(r"ZIP_UNSUPPORTED = 18,", plan) and re.search(r"ZIP_ROW_WORDS = 8,", plan)
    assert (zip_walk.MORE_ENTRIES, zip_walk.MORE_CANDIDATES, zip_walk.UNSUPPORTED) == (16, 17, 18)
    assert (zip_walk.RESULT_WORDS, zip_walk.WORDS, zip_walk.SLACK, zip_walk.ZIP64) == (5, 8, 1024, 1)
    assert (zf.MORE_ENTRIES, zf.MORE_CANDIDATES, zf.UNSUPPORTED) == (16, 17, 18)


def test_calls_check_their_arguments(lib):
    """Refused before any device is touched, with a reason: a NULL object or
    pointer (d_out only with out_avail != 0, d_in only with in_nbytes != 0,
    d_index never), max_entries == 0 or above 2^28, in_nbytes above 2^36, an
    out_align that is no power of two in 1 .. 256; and for a selection the
    rows, the entry numbers and the room."""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    dec = lib.libdeflate_amd_zip_decompress_batch
    idx = lib.libdeflate_amd_zip_index_batch
    rd = lib.libdeflate_amd_zip_read_batch

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
    refused(dec(None, d, 28, 1, d, 64, 1, d, None, d, None), "NULL")
    refused(dec(fake, None, 28, 1, d, 64, 1, d, None, d, None), "NULL")
    refused(dec(fake, d, 28, 1, None, 64, 1, d, None, d, None), "NULL")
    refused(dec(fake, d, 28, 1, d, 64, 1, None, None, d, None), "NULL")
    refused(dec(fake, d, 28, 1, d, 64, 1, d, None, None, None), "NULL")
    refused(dec(fake, d, 28, 0, d, 64, 1, d, None, d, None), "max_entries")
    refused(dec(fake, d, 28, (1 << 28) + 1, d, 64, 1, d, None, d, None), "max_entries")
    refused(dec(fake, d, (1 << 36) + 1, 1, d, 64, 1, d, None, d, None), "in_nbytes")
    for align in (0, 3, 24, 512, 1 << 20):
        refused(dec(fake, d, 28, 1, d, 64, align, d, None, d, None), "out_align")
        refused(idx(fake, d, 28, 1, align, d, None, d, None), "out_align")
    assert "zip_index_batch" in binding.last_error()
    refused(idx(None, d, 28, 1, 1, d, None, d, None), "NULL")
    refused(idx(fake, None, 28, 1, 1, d, None, d, None), "NULL")
    refused(idx(fake, d, 28, 1, 1, None, None, d, None), "NULL")
    refused(idx(fake, d, 28, 1, 1, d, None, None, None), "NULL")
    refused(idx(fake, d, 28, 0, 1, d, None, d, None), "max_entries")
    refused(idx(fake, d, 28, (1 << 28) + 1, 1, d, None, d, None), "max_entries")
    refused(idx(fake, d, (1 << 36) + 1, 1, 1, d, None, d, None), "in_nbytes")
    # a selection: rows of a file of 1000 bytes
    rows = np.array([[900, 4, 8, 0x1234, 40, 100, 500, 0],
                     [950, 4, 0, 0x1234, 200, 30, 30, 500]], dtype=np.uint64)
    rp = rows.ctypes.data_as(ctypes.c_void_p)

    def sel(*s):
        a = np.array(s, dtype=np.uint64)
        return a, a.ctypes.data_as(ctypes.c_void_p)
    a, sp = sel(0, 1)
    refused(rd(None, d, 1000, rp, 2, 2, sp, d, 4096, 1, None, d, None), "NULL")
    refused(rd(fake, None, 1000, rp, 2, 2, sp, d, 4096, 1, None, d, None), "NULL")
    refused(rd(fake, d, 1000, None, 2, 2, sp, d, 4096, 1, None, d, None), "NULL")
    refused(rd(fake, d, 1000, rp, 2, 2, None, d, 4096, 1, None, d, None), "NULL")
    refused(rd(fake, d, 1000, rp, 2, 2, sp, None, 4096, 1, None, d, None), "NULL")
    refused(rd(fake, d, 1000, rp, 2, 2, sp, d, 4096, 1, None, None, None), "NULL")
    refused(rd(fake, d, 1000, rp, 2, 2, sp, d, 4096, 48, None, d, None), "out_align")
    refused(rd(fake, d, (1 << 36) + 1, rp, 2, 2, sp, d, 4096, 1, None, d, None), "in_nbytes")
    refused(rd(fake, d, 1000, rp, 2, 2, sp, d, 529, 1, None, d, None), "out_avail")
    refused(rd(fake, d, 1000, rp, 2, 2, sp, d, 530 + 13, 16, None, d, None), "out_avail")
    refused(rd(fake, d, 949, rp, 2, 2, sp, d, 4096, 1, None, d, None), "in_nbytes")
    refused(rd(fake, d, 139, rp, 2, 1, sp, d, 4096, 1, None, d, None), "in_nbytes")
    a, sp = sel(1, 2)
    refused(rd(fake, d, 1000, rp, 2, 2, sp, d, 4096, 1, None, d, None), "sel[1] = 2")
    big = rows.copy()
    big[0, 6] = 1 << 32
    a, sp = sel(0)
    refused(rd(fake, d, 1000, big.ctypes.data_as(ctypes.c_void_p), 2, 1, sp, d, 1 << 40, 1, None,
               d, None), "4 GiB")
    # nothing selected: nothing to do, and the offsets say so
    offs = np.full(1, 77, dtype=np.uint64)
    assert rd(fake, d, 1000, rp, 2, 0, None, d, 0, 1, offs.ctypes.data_as(ctypes.c_void_p), None,
              None) == 0
    assert offs[0] == 0


# ---- the CPU model against zipfile ----

def _name(data, row):
    raw = data[row[0] + 46:row[0] + 46 + row[1]]
    return raw.decode("utf-8" if (row[2] >> 16) & 0x800 else "cp437")


@pytest.mark.parametrize("name", zf.GOOD_NAMES)
def test_model_reads_every_good_file_as_zipfile_does(name):
    """entry count, names, methods, CRCs, sizes, header_offset, the data
    offset from the local header and the bytes of every entry; out_off for
    out_align 1, 16 and 256; max_entries exact and generous"""
    g = zf.good(name)
    assert g.name == name
    infos, datas = zf.expected(g)
    m = len(infos)
    r = zip_walk.read(g.data, max(m, 1))
    assert r.words[0] == SUCCESS and r.words[1] == m
    assert r.words[4] == (zip_walk.ZIP64 if g.zip64 else 0)
    assert r.results == [SUCCESS] * m and r.plain == datas
    assert zip_walk.read(g.data, 16 * max(m, 1), decode=False)[:3] == (r.words, r.rows, r.results)
    end = zip_walk.find_end(g.data)
    assert r.words[2] == end.cd_off
    at = 0
    for row, zi in zip(r.rows, infos):
        lho = zi.header_offset
        n, x = struct.unpack_from("<HH", g.twin, lho + 26)
        assert _name(g.data, row) == zi.filename or zi.filename.startswith(_name(g.data, row))
        assert row[1] == len(zi.orig_filename.encode("utf-8" if zi.flag_bits & 0x800 else "cp437"))
        assert row[2] == zi.compress_type | zi.flag_bits << 16
        assert row[3:7] == [zi.CRC, lho + 30 + n + x, zi.compress_size, zi.file_size]
        assert g.data[lho:lho + 4] == b"PK\3\4" and row[7] == at
        at += zi.file_size
    assert r.words[3] == at
    for align in (16, 256):
        ra = zip_walk.read(g.data, max(m, 1), out_align=align, decode=False)
        at = 0
        for k, (row, zi) in enumerate(zip(ra.rows, infos)):
            assert row[7] == at and row[:7] == r.rows[k][:7]
            at += -(-zi.file_size // align) * align
        assert ra.words == [SUCCESS, m, end.cd_off, at, r.words[4]]
    ri = zip_walk.read(g.data, max(m, 1), decode=False)
    assert ri.words == r.words and ri.rows == r.rows and ri.plain is None


def test_model_end_record_choice():
    """the window's far edge, bytes behind the end record, a look-alike in the
    comment, nothing at all"""
    g = zf.mixed(65535)
    p = zip_walk.end_offset(g.data)
    assert p == len(g.data) - zip_walk.WINDOW and g.data[p:p + 4] == b"PK\5\6"
    # one byte more behind it and the record is out of the window
    assert zip_walk.read(g.data + b"\0", 16).words == [BAD_DATA, 0, 0, 0, 0]
    f = zf.false()
    assert f.data.count(b"PK\5\6") == 3     # the archive's, the inner archive's, the look-alike
    assert zip_walk.end_offset(f.data) == zip_walk.end_offset(f.twin) == len(f.data) - 22 - 64
    for n in (0, 1, 21):
        assert zip_walk.read(b"\0" * n, 1).words == [BAD_DATA, 0, 0, 0, 0]
    assert zip_walk.read(b"\0" * 1000, 1).words == [BAD_DATA, 0, 0, 0, 0]
    # an end signature whose comment runs past the file is none
    e = zf.empty().data
    assert zip_walk.read(e, 1).words == [SUCCESS, 0, 0, 0, 0]
    assert zip_walk.read(e[:20] + b"\1\0", 1).words == [BAD_DATA, 0, 0, 0, 0]
    assert zip_walk.read(e[:20] + b"\1\0x", 1).words == [SUCCESS, 0, 0, 0, 0]


def test_model_false_candidates_are_there_and_do_not_matter():
    f = zf.false()
    end = zip_walk.find_end(f.data)
    cands = zip_walk.candidates(f.data, end)
    rels = zip_walk.chain(f.data, end, cands)
    assert len(rels) == 5 and len(cands) > 5 and set(rels) < set(cands)
    # the inner archive's directory lies outside the directory: no candidates
    assert f.data.count(b"PK\1\2") > len(cands)


def test_model_limits_and_precedence():
    g = zf.mixed(0)
    infos, datas = zf.expected(g)
    m, total = len(infos), sum(len(x) for x in datas)
    cd_off = zip_walk.find_end(g.data).cd_off
    r = zip_walk.read(g.data, m - 1)
    assert r.words == [MORE_ENTRIES, m, 0, 0, 0] and r.rows is None and r.results is None
    assert zip_walk.read(g.data, m - 1, out_avail=0).words[0] == MORE_ENTRIES
    r = zip_walk.read(g.data, m, out_avail=total - 1)
    assert r.words == [INSUFFICIENT_SPACE, m, cd_off, total, 0]
    assert r.plain is None and r.results == [SUCCESS] * m
    assert r.rows == zip_walk.read(g.data, m).rows
    assert zip_walk.read(g.data, m, out_avail=total).words[0] == SUCCESS
    assert zip_walk.read(g.data, m, out_avail=0, decode=False).words[0] == SUCCESS
    # candidates: room for max_entries + SLACK
    la = zf.lookalikes()
    k = len(zip_walk.candidates(la.data, zip_walk.find_end(la.data)))
    assert zf.LOOKALIKES - 12 <= k - 1 <= zf.LOOKALIKES
    for mm in (1, k - 1024 - 1):
        assert zip_walk.read(la.data, mm).words == [MORE_CANDIDATES, k, 0, 0, 0]
    assert zip_walk.read(la.data, k - 1024).words[:2] == [SUCCESS, 1]
    # the end record comes before the count, the count before the candidates
    bad = {d.name: d for d in zf.defects()}
    assert zip_walk.read(bad["cd_off+1"].data, 1).words == [BAD_DATA, 0, 0, 0, 0]
    assert zip_walk.read(bad["count+1"].data, 6).words == [MORE_ENTRIES, 7, 0, 0, 0]
    assert zip_walk.read(bad["cen_sig"].data, 6, out_avail=0).words == [BAD_DATA, 0, 0, 0, 0]


@pytest.mark.parametrize("d", zf.defects(), ids=lambda d: d.name)
def test_model_on_the_defect_files(d):
    """one defect per file: the verdict, the words and the per-entry results
    the issue states; every neighbour's bytes are zipfile's"""
    infos, datas = zf.expected(d.base)
    m = len(infos)
    r = zip_walk.read(d.data, m + 1)
    if d.entry is None:
        assert r.words == [BAD_DATA, 0, 0, 0, 0] and r.rows is None and r.results is None
        assert zip_walk.read(d.data, m + 1, decode=False).words == r.words
        if not d.name.startswith("count"):      # zipfile does not look at the count
            with pytest.raises((zipfile.BadZipFile, ValueError)):
                zipfile.ZipFile(io.BytesIO(d.data)).testzip()
        return
    want = [SUCCESS] * m
    want[d.entry] = d.result
    assert r.results == want and r.words[0] == d.result and r.words[1] == m
    assert [p for k, p in enumerate(r.plain) if k != d.entry] == \
        [p for k, p in enumerate(datas) if k != d.entry]
    assert r.plain[d.entry] is None
    pre = d.name in ("zip64_extra_short", "local_sig", "data_past_cd", "stored_sizes",
                     "flag_bit0", "method12")
    ri = zip_walk.read(d.data, m + 1, decode=False)
    assert ri.results == (want if pre else [SUCCESS] * m)
    # an entry refused before the decode takes no room, any other keeps its slot
    base = zip_walk.read(d.base.data, m)
    usize = r.rows[d.entry][6]
    assert r.words[3] == base.words[3] - base.rows[d.entry][6] + (0 if pre else usize)
    if d.name == "local_sig":
        assert r.rows[d.entry][4] == 0
    if d.name == "crc":
        assert [row[:3] + row[4:] for row in r.rows] == [row[:3] + row[4:] for row in base.rows]
    # a selection of it fails alone too
    offs, res, plain = zip_walk.read_selection(d.data, r.rows, list(range(m)))
    assert res == r.results or d.name in ("zip64_extra_short", "local_sig", "data_past_cd")
    assert [p for k, p in enumerate(plain) if k != d.entry] == \
        [p for k, p in enumerate(datas) if k != d.entry]


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "zip_kernels.hip", "-o", os.devnull],
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
    # the end search's 16 wave maxima; the scan's tile and four wave sums; the
    # final kernel's first-failure word
    assert lds == [64, 4096 + 16 + 16, 0, 0, 0, 0, 8, 0], lds
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert [x for x in KERNELS if f"\n{x}(" not in k] == []
