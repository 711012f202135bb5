"""CPU-side checks of libdeflate_amd_decompress_large (one raw DEFLATE / zlib /
gzip stream from device memory to device memory on many waves): declared in the
header, exported by the library, described by the binding, its arguments
refused before any device work, and present in the Python interface."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "libdeflate_amd_decompress_large"
BAD_DATA = 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from libdeflate_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    return binding.load()


def test_symbol_declared_exported_and_bound(lib):
    from libdeflate_amd import binding
    hdr = open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()
    assert SYMBOL in re.findall(r"^(libdeflate_[a-z0-9_]+)\(", hdr, re.M)
    assert SYMBOL in binding.BATCH_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert SYMBOL in re.findall(r" T (libdeflate_\w+)", out)
    fn = getattr(lib, SYMBOL)
    assert len(fn.argtypes) == 9 and fn.restype is ctypes.c_int
    assert not binding.MISSING


def test_arguments_are_checked_before_any_device_work(lib):
    """A NULL object, a NULL input of a non-zero size, a NULL output of a
    non-zero size, a format that is not DEFLATE / zlib / gzip:
    LIBDEFLATE_BAD_DATA with a reason that names what was wrong.  The object is
    a stand-in: every check comes before it is used."""
    from libdeflate_amd import binding
    buf = (ctypes.c_uint8 * 4096)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    fn = getattr(lib, SYMBOL)
    gz = binding.FMT_GZIP
    ai, ao = ctypes.c_size_t(7), ctypes.c_size_t(7)

    def refused(*args):
        rc = fn(*args)
        return rc == BAD_DATA and binding.last_error() != ""
    for rets in ((ctypes.byref(ai), ctypes.byref(ao)), (None, None)):
        assert refused(None, gz, d, 16, d, 4096, *rets, None)
        assert "NULL" in binding.last_error()
        assert refused(fake, gz, None, 16, d, 4096, *rets, None)
        assert "NULL" in binding.last_error() and "d_in" in binding.last_error()
        assert refused(fake, gz, d, 16, None, 4096, *rets, None)
        assert "NULL" in binding.last_error() and "d_out" in binding.last_error()
        for fmt in (binding.FMT_BGZF, -1, 4, 99):
            assert refused(fake, fmt, d, 16, d, 4096, *rets, None), fmt
            assert "format" in binding.last_error()
    assert (ai.value, ao.value) == (7, 7)       # nothing written on a refusal


def test_python_interface_has_the_call():
    from libdeflate_amd import api
    assert callable(api.Decompressor.decompress_large)
