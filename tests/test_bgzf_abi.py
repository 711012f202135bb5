"""CPU-side checks of the BGZF calls: declared in the header, exported by the
library, described by the binding with the header's constants, the bound's
arithmetic, arguments refused before any device work, and the pure-Python
BGZF walker (tests/bgzf_walk.py) the GPU tests rest on, against files built
by hand with zlib."""
import ctypes
import gzip
import os
import random
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import bgzf_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGZF_SYMBOLS = ("libdeflate_amd_bgzf_compress_bound", "libdeflate_amd_bgzf_compress_batch",
                "libdeflate_amd_bgzf_compress")
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


def test_bgzf_symbols_declared_exported_and_bound(lib):
    from libdeflate_amd import binding
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", _header(), re.M))
    assert set(BGZF_SYMBOLS) <= declared
    assert set(BGZF_SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(BGZF_SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    for s in BGZF_SYMBOLS:
        assert getattr(lib, s).argtypes, s
    assert not binding.MISSING


def test_bgzf_constants_match_the_header():
    from libdeflate_amd import binding
    hdr = _header()

    def define(name):
        return int(re.search(rf"#define {name}\s+(\d+)", hdr).group(1))
    assert int(re.search(r"LIBDEFLATE_AMD_BGZF = (\d+),", hdr).group(1)) == binding.FMT_BGZF == 3
    assert binding.FORMATS["bgzf"] == 3
    assert define("LIBDEFLATE_AMD_BGZF_BLOCK") == binding.BGZF_BLOCK == bgzf_walk.BLOCK == 65280
    assert define("LIBDEFLATE_AMD_BGZF_MEMBER_MAX") == binding.BGZF_MEMBER_MAX == 65536
    assert define("LIBDEFLATE_AMD_BGZF_EOF_BYTES") == binding.BGZF_EOF_BYTES == \
        len(bgzf_walk.EOF_MEMBER) == 28
    assert define("LIBDEFLATE_AMD_BGZF_NO_EOF") == binding.BGZF_NO_EOF == 1
    # the fixed bytes the header documents are the walker's
    assert "1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00" in hdr
    assert bgzf_walk.PREFIX == bytes.fromhex("1f8b08040000000000ff060042430200")


def test_bgzf_bound_arithmetic(lib):
    """m members of at most 64 KiB, m = ceil(n / 65280), and the EOF member;
    a NULL compressor is allowed"""
    for n in (0, 1, 65279, 65280, 65281, 2 * 65280, 2 * 65280 + 1, 1 << 30, 1 << 34):
        m = -(-n // 65280)
        assert lib.libdeflate_amd_bgzf_compress_bound(None, n) == m * 65536 + 28
    # every member's worst case - stored blocks of one 4 KiB tile each, a
    # byte of padding, header and trailer - stays under the 64 KiB of BSIZE
    assert 18 + 8 + 65280 + 5 * (65280 // 4096 + 1) + 1 < 65536


def test_bgzf_calls_check_their_arguments(lib):
    """Refused before any device is touched: a NULL object or buffer, unknown
    flags, output space below 27 bytes per member and the EOF member, index
    space below 2 (m + 1); format 3 in the dictionary calls."""
    from libdeflate_amd import binding
    buf = (ctypes.c_uint8 * 4096)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    # a stand-in object: every check below comes before the object is used
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    dev = lib.libdeflate_amd_bgzf_compress_batch
    host = lib.libdeflate_amd_bgzf_compress
    assert dev(None, d, 16, d, 4096, d, None, 0, None) == BAD_ARG
    assert "NULL" in binding.last_error()
    assert host(None, d, 16, d, 4096, None, 0, 0) == 0
    assert dev(fake, None, 16, d, 4096, d, None, 0, None) == BAD_ARG
    assert dev(fake, d, 16, None, 4096, d, None, 0, None) == BAD_ARG
    assert dev(fake, d, 16, d, 4096, None, None, 0, None) == BAD_ARG
    assert dev(fake, d, 16, d, 4096, d, None, 2, None) == BAD_ARG
    assert "flags" in binding.last_error()
    assert host(fake, d, 16, d, 4096, None, 0, 6) == 0
    assert "flags" in binding.last_error()
    # output space: one member of 16 bytes needs 27 + 28 at the very least
    assert dev(fake, d, 16, d, 54, d, None, 0, None) == BAD_ARG
    assert "out_avail" in binding.last_error()
    assert host(fake, d, 16, d, 54, None, 0, 0) == 0
    assert "out_avail" in binding.last_error()
    assert host(fake, d, 16, d, 26, None, 0, 1) == 0    # NO_EOF: 27
    assert dev(fake, d, 0, d, 27, d, None, 0, None) == BAD_ARG   # EOF alone: 28
    # index space: 2 (m + 1) u64 entries
    assert host(fake, d, 65281, d, 1 << 20, d, 5, 0) == 0
    assert "index_avail" in binding.last_error()
    # format 3 takes no dictionary
    for fn in (lib.libdeflate_amd_compress_batch_dict, lib.libdeflate_amd_decompress_batch_dict):
        nargs = len(fn.argtypes)
        assert fn(*([None, binding.FMT_BGZF, 1, d, 16] + [d] * (nargs - 5))) == BAD_ARG
        assert "dictionary" in binding.last_error()
    assert lib.libdeflate_amd_compress_dict(None, binding.FMT_BGZF, d, 16, d, 16, d, 64) == 0
    assert lib.libdeflate_amd_decompress_dict_ex(None, binding.FMT_BGZF, d, 16, d, 16, d, 64,
                                                 None, None) == binding.BAD_DATA


def _data(n, seed):
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"acgtn") for _ in range(rng.randrange(3, 12))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
        if rng.random() < 0.05:
            out += bytes(rng.randrange(256) for _ in range(20))
    return bytes(out[:n])


@pytest.mark.parametrize("n", [0, 1, 65279, 65280, 65281, 3 * 65280, 200000])
def test_walker_reads_files_built_with_zlib(n):
    data = _data(n, n)
    f = bgzf_walk.build(data, level=6)
    members, eof = bgzf_walk.walk(f)
    assert eof and len(members) == -(-n // 65280)
    assert b"".join(m.data for m in members) == data == gzip.decompress(f)
    assert all(m.isize == 65280 for m in members[:-1])
    pos = 0
    for m in members:
        assert m.offset == pos and f[pos + 16] | f[pos + 17] << 8 == m.size - 1
        pos += m.size
    assert pos == len(f) - 28
    # without the EOF member the walker says so, or refuses
    assert bgzf_walk.walk(f[:-28], require_eof=False) [1] is False
    with pytest.raises(bgzf_walk.BgzfError):
        bgzf_walk.walk(f[:-28])


def test_walker_rejects_what_the_spec_forbids():
    data = _data(150000, 7)
    f = bytearray(bgzf_walk.build(data))
    bad = [bytearray(f) for _ in range(6)]
    bad[0][16] ^= 1                                # BSIZE off by one
    bad[1][9] = 3                                  # OS
    bad[2][12] = ord("X")                          # subfield id
    m0 = struct.unpack_from("<H", f, 16)[0] + 1
    bad[3][m0 - 8] ^= 0xFF                         # CRC
    bad[4][m0 - 4] ^= 1                            # ISIZE
    bad[5] = f[:-28] + f[-28:] + bgzf_walk.member(b"x")   # data after EOF
    for b in bad:
        with pytest.raises(bgzf_walk.BgzfError):
            bgzf_walk.walk(bytes(b))
    # a member of more than 65280 input bytes is not BGZF
    big = bgzf_walk.member(bytes(65281), level=1)
    with pytest.raises(bgzf_walk.BgzfError):
        bgzf_walk.walk(big + bgzf_walk.EOF_MEMBER)


def test_gzi_helper_round_trips():
    from libdeflate_amd import api
    idx = np.array([[0, 0], [1000, 65280], [2500, 130560], [2600, 140000]], dtype=np.uint64)
    blob = api.bgzf_gzi(idx)
    assert len(blob) == 8 + 16 * 2
    assert struct.unpack("<Q", blob[:8])[0] == 2
    assert np.array_equal(api.bgzf_gzi_parse(blob), idx[1:-1])
    assert api.bgzf_gzi(idx[[0, -1]]) == bytes(8)   # one member: no entries
