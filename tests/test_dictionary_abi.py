"""CPU-side checks of the preset-dictionary calls: declared in the header,
exported by the library, described by the binding, and their arguments
checked before any device work."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICT_SYMBOLS = ("libdeflate_amd_compress_batch_dict", "libdeflate_amd_decompress_batch_dict",
                "libdeflate_amd_compress_dict", "libdeflate_amd_decompress_dict_ex")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from libdeflate_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    return binding.load()


def test_dictionary_symbols_declared_and_exported(lib):
    from libdeflate_amd import binding
    hdr = open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", hdr, re.M))
    assert set(DICT_SYMBOLS) <= declared
    assert set(DICT_SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(DICT_SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    for s in DICT_SYMBOLS:
        assert getattr(lib, s).argtypes, s


def test_dictionary_window_is_what_the_header_states():
    """W = 32 KiB minus two 4 KiB tiles and the 272-byte lookahead, in whole
    tiles (host_compress.hip, dict_window())"""
    hdr = open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()
    w = int(re.search(r"#define LIBDEFLATE_AMD_DICT_WINDOW (\d+)", hdr).group(1))
    assert w == (32768 - 2 * 4096 - 272) // 4096 * 4096 == 20480


def test_dictionary_calls_check_their_arguments(lib):
    """Bad arguments come back before any device is touched: a gzip format,
    a NULL object, a NULL dictionary with a length."""
    from libdeflate_amd import binding
    buf = (ctypes.c_uint8 * 64)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.libdeflate_amd_compress_batch_dict, lib.libdeflate_amd_decompress_batch_dict):
        nargs = len(fn.argtypes)
        # gzip: zlib refuses a dictionary there
        args = [None, binding.FMT_GZIP, 1, d, 16] + [d] * (nargs - 5)
        assert fn(*args) == -2
        assert "dictionary" in binding.last_error()
        # a length without a dictionary
        args = [None, binding.FMT_ZLIB, 1, None, 16] + [d] * (nargs - 5)
        assert fn(*args) == -2
        # a NULL object
        args = [None, binding.FMT_DEFLATE, 1, d, 16] + [d] * (nargs - 5)
        assert fn(*args) == -2
    # single buffer: compress returns 0, decompress BAD_DATA
    assert lib.libdeflate_amd_compress_dict(None, binding.FMT_GZIP, d, 16, d, 16, d, 64) == 0
    assert "dictionary" in binding.last_error()
    assert lib.libdeflate_amd_compress_dict(None, binding.FMT_ZLIB, d, 16, d, 16, d, 64) == 0
    assert lib.libdeflate_amd_decompress_dict_ex(None, binding.FMT_GZIP, d, 16, d, 16, d, 64,
                                                 None, None) == binding.BAD_DATA
    assert lib.libdeflate_amd_decompress_dict_ex(None, binding.FMT_DEFLATE, d, 16, d, 16, d,
                                                 64, None, None) == binding.BAD_DATA
