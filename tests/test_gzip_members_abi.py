"""CPU-side checks of the reader of concatenated gzip members: the two calls
declared, exported and bound with the header's constants; arguments refused
before any device is touched; the CPU model of the finder
(tools/models/gzip_chain.py) against the member lists recorded while the
files were built (tests/gzip_members_files.py), adversarial and defect files
included; and the new kernels' compile report."""
import ctypes
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gzip_members_files as gf
from tools.models import gzip_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
SYMBOLS = ("libdeflate_amd_gzip_members_decompress_batch",
           "libdeflate_amd_gzip_members_index_batch")
KERNELS = ["lda_gzm_scan_kernel", "lda_gzm_slots_kernel", "lda_gzm_size32_kernel",
           "lda_gzm_break_kernel", "lda_gzm_msize_kernel", "lda_gzm_desc_kernel",
           "lda_gzm_final_kernel"]
BAD_ARG = -2
SUCCESS, BAD_DATA, INSUFFICIENT_SPACE, MORE_MEMBERS, MORE_CANDIDATES = 0, 1, 3, 16, 17


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from libdeflate_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    return binding.load()


@pytest.fixture(scope="module")
def files():
    return gf.good_files()


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
    assert len(lib.libdeflate_amd_gzip_members_decompress_batch.argtypes) == 9
    assert len(lib.libdeflate_amd_gzip_members_index_batch.argtypes) == 7
    assert not binding.MISSING
    assert callable(api.Decompressor.decompress_gzip_members_batch)
    assert callable(api.Decompressor.index_gzip_members_batch)


def test_constants_match_the_header():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name, text=hdr):
        return int(re.search(rf"#define {name}\s+(\d+)", text).group(1))
    assert define("LIBDEFLATE_AMD_GZM_MORE_MEMBERS") == binding.GZM_MORE_MEMBERS == 16
    assert define("LIBDEFLATE_AMD_GZM_MORE_MEMBERS") == define("LIBDEFLATE_AMD_BGZF_MORE_MEMBERS")
    assert define("LIBDEFLATE_AMD_GZM_MORE_CANDIDATES") == binding.GZM_MORE_CANDIDATES == 17
    assert define("LIBDEFLATE_AMD_GZM_RESULT_WORDS") == binding.GZM_RESULT_WORDS == 5
    assert define("LIBDEFLATE_AMD_GZM_SLACK") == binding.GZM_SLACK == 1024
    assert define("LIBDEFLATE_AMD_GZM_NAME_MAX") == binding.GZM_NAME_MAX == 65536
    assert gzip_chain.NAME_MAX == gf.NAME_MAX == 65536
    # the device side's copies (kernels.h) and the model's are the header's
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert define("LDA_GZM_MORE_CANDIDATES", k) == 17
    assert define("LDA_GZM_RESULT_WORDS", k) == 5
    assert define("LDA_GZM_NAME_MAX", k) == 65536
    assert define("LDA_BR_MORE", k) == 16
    assert define("LDA_BR_JUMP", k) == gzip_chain.BLOCK
    assert (gzip_chain.MORE_MEMBERS, gzip_chain.MORE_CANDIDATES, gzip_chain.SLACK) == (16, 17, 1024)
    assert binding.SIZE_LIMIT_MAX == gzip_chain.SIZE_LIMIT


def test_calls_check_their_arguments(lib):
    """Refused before any device is touched, with a reason: a NULL object or
    pointer (d_out only with out_avail != 0), max_members == 0 or above 2^28,
    in_nbytes above 2^36."""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    dec = lib.libdeflate_amd_gzip_members_decompress_batch
    idx = lib.libdeflate_amd_gzip_members_index_batch

    def refused(rc, word):
        assert rc == BAD_ARG
        assert word in binding.last_error(), binding.last_error()
    refused(dec(None, d, 28, 1, d, 64, d, None, None), "NULL")
    refused(dec(fake, None, 28, 1, d, 64, d, None, None), "NULL")
    refused(dec(fake, d, 28, 1, None, 64, d, None, None), "NULL")
    refused(dec(fake, d, 28, 1, d, 64, None, None, None), "NULL")
    refused(dec(fake, d, 28, 0, d, 64, d, None, None), "max_members")
    refused(dec(fake, d, 28, (1 << 28) + 1, d, 64, d, None, None), "max_members")
    refused(dec(fake, d, (1 << 36) + 1, 1, d, 64, d, None, None), "in_nbytes")
    refused(dec(fake, d, 0, 0, d, 64, d, None, None), "max_members")
    refused(idx(None, d, 28, 1, d, None, None), "NULL")
    refused(idx(fake, None, 28, 1, d, None, None), "NULL")
    refused(idx(fake, d, 28, 1, None, None, None), "NULL")
    refused(idx(fake, d, 28, 0, d, None, None), "max_members")
    refused(idx(fake, d, 28, (1 << 28) + 1, d, None, None), "max_members")
    refused(idx(fake, d, (1 << 36) + 1, 1, d, None, None), "in_nbytes")
    assert "gzip_members_index_batch" in binding.last_error()


# ---- the CPU model of the finder ----

def _rows(r):
    return np.array(r.rows, dtype=np.uint64).reshape(-1, 2)


def test_model_reads_every_good_file(files):
    """words, index and bytes of every good file, with max_members exact and
    generous, and with blocks of 4 candidates and of 1, which put every chain
    across many blocks"""
    for f in files:
        mm = 477 if f.name == "overflow" else f.m
        plain = gzip.decompress(f.data)
        assert plain == f.plain
        for kw in ({}, {"block": 4}, {"block": 1}):
            for m in (mm, 16 * mm):
                r = gzip_chain.read(f.data, m, **kw)
                assert r.words == [SUCCESS, f.m, len(f.data), len(plain), 0], (f.name, m, kw)
                assert np.array_equal(_rows(r), f.rows()), f.name
                assert r.plain == plain, f.name
        r = gzip_chain.read(f.data, mm, decode=False)
        assert r.words == [SUCCESS, f.m, len(f.data), len(plain), 0] and r.plain is None
        assert np.array_equal(_rows(r), f.rows()), f.name


def test_model_false_candidates_are_there_and_are_no_members():
    for kind in gf.FALSE_KINDS:
        f = gf.false_candidates(kind)
        cands = gzip_chain.candidates(f.data)
        starts = {o for o, _, _ in f.members}
        extra = [p for p in cands if p not in starts]
        assert starts <= set(cands) and len(cands) == gf.n_candidates(f.data)
        counts = [gzip_chain.count(f.data, p) for p in extra]
        if kind == "member":    # counts, and ends where nothing starts
            assert len(extra) == 1 and counts[0][0] == SUCCESS
            assert extra[0] + counts[0][1] not in cands
        if kind == "pair":      # the first false candidate's successor is the second
            assert len(extra) == 2 and [c[0] for c in counts] == [SUCCESS, SUCCESS]
            assert extra[0] + counts[0][1] == extra[1]
            assert extra[1] + counts[1][1] not in cands
        if kind == "junk":
            assert len(extra) == 1 and counts[0][0] == BAD_DATA
        if kind == "stride3":   # six candidates within 16 bytes
            assert len(extra) == 199
            assert all(b - a == 3 for a, b in zip(extra, extra[1:]))


def test_model_name_limit():
    """FNAME + FCOMMENT of NAME_MAX bytes are a member's, one more is not: the
    reader's own rule, which bounds what a false candidate with FNAME set can
    make the count walk.  zlib's and the host loop's readers have no such rule"""
    f = gf.long_names(gf.NAME_MAX)
    assert gzip_chain.read(f.data, f.m).words == [SUCCESS, f.m, len(f.data), len(f.plain), 0]
    g = gf.long_names(gf.NAME_MAX + 1)
    assert gzip.decompress(g.data) == g.plain
    assert gzip_chain.read(g.data, g.m).words == [BAD_DATA, 0, 0, 0, 0]
    # a header with FNAME set looks NAME_MAX bytes far for the name's end, no further
    head = gf.SIG + b"\x08" + b"\1" * 6
    assert gzip_chain.header_len(head + b"n" * (gf.NAME_MAX - 1) + b"\0" * 20, 0) == 10 + gf.NAME_MAX
    assert gzip_chain.header_len(head + b"n" * gf.NAME_MAX + b"\0" * 20, 0) == 0
    assert gzip_chain.header_len(head + b"n" * 300, 0) == 0      # no end at all


def test_model_limits_and_precedence():
    f = gf.overflow()
    assert gzip_chain.read(f.data, 1).words == [MORE_CANDIDATES, 1501, 0, 0, 0]
    assert gzip_chain.read(f.data, 476).words == [MORE_CANDIDATES, 1501, 0, 0, 0]
    assert gzip_chain.read(f.data, 477).words[0] == SUCCESS
    f = gf.tiny()
    n, total = len(f.data), len(f.plain)
    r = gzip_chain.read(f.data, f.m - 1)
    assert r.words == [MORE_MEMBERS, f.m, 0, 0, 0] and r.rows is None and r.plain is None
    # MORE_MEMBERS comes before the space
    assert gzip_chain.read(f.data, f.m - 1, out_avail=0).words[0] == MORE_MEMBERS
    r = gzip_chain.read(f.data, f.m, out_avail=total - 1)
    assert r.words == [INSUFFICIENT_SPACE, f.m, n, total, 0] and r.plain is None
    assert np.array_equal(_rows(r), f.rows())
    assert gzip_chain.read(f.data, f.m, out_avail=total).words[0] == SUCCESS
    assert gzip_chain.read(f.data, f.m, out_avail=total - 1, decode=False).words[0] == SUCCESS
    # a broken chain comes before both
    bad = dict(gf.defects())["zero1"]
    assert gzip_chain.read(bad, 1, out_avail=0).words == [BAD_DATA, 0, 0, 0, 0]


def test_model_on_the_defect_files():
    base = gf.defect_base()
    n, total = len(base.data), len(base.plain)
    for name, b in gf.defects():
        for kw in ({}, {"block": 2}):
            r = gzip_chain.read(b, base.m, **kw)
            if name == "crc":   # the decode's verdict; the neighbours' bytes are right
                assert r.words == [BAD_DATA, base.m, n, total, 0]
                assert r.plain == base.plain and np.array_equal(_rows(r), base.rows())
                assert gzip_chain.read(b, base.m, decode=False).words[0] == SUCCESS
            else:
                assert r.words == [BAD_DATA, 0, 0, 0, 0], name
                assert r.rows is None and r.plain is None
                assert gzip_chain.read(b, base.m, decode=False).words == r.words


# ---- the kernels as the compiler reports them ----

def test_kernels_compile_without_spills_or_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        "gzip_members_kernels.hip", "-o", os.devnull],
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
    # the scan's tile and four wave sums; nothing else but the final kernel's word
    assert lds == [4096 + 16 + 16, 0, 0, 0, 0, 0, 4], lds
    # the declarations the host side launches through are the definitions'
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert [x for x in KERNELS if f"\n{x}(" not in k] == []
