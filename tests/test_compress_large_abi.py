"""CPU-side checks of libdeflate_amd_compress_large_batch (one raw DEFLATE /
zlib / gzip stream from one device buffer): declared in the header, exported by
the library, described by the binding, its arguments refused before any device
work, and present in the Python interface."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "libdeflate_amd_compress_large_batch"
BAD_ARG = -2


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
    assert len(fn.argtypes) == 8 and fn.restype is ctypes.c_int
    assert not binding.MISSING


def test_arguments_are_checked_before_any_device_work(lib):
    """A NULL object, a NULL input of a non-zero size, a NULL output or size
    pointer, a format that is not DEFLATE / zlib / gzip, output space that
    cannot hold header, footer and one byte: BAD_ARG with a reason.  The object
    is a stand-in: every check comes before it is used."""
    from libdeflate_amd import binding
    buf = (ctypes.c_uint8 * 4096)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    fn = getattr(lib, SYMBOL)
    gz = binding.FMT_GZIP

    def refused(*args):
        rc = fn(*args)
        return rc == BAD_ARG and binding.last_error() != ""
    assert refused(None, gz, d, 16, d, 4096, d, None)
    assert "NULL" in binding.last_error()
    assert refused(fake, gz, None, 16, d, 4096, d, None)
    assert refused(fake, gz, d, 16, None, 4096, d, None)
    assert refused(fake, gz, d, 16, d, 4096, None, None)
    for fmt in (binding.FMT_BGZF, -1, 4, 99):
        assert refused(fake, fmt, d, 16, d, 4096, d, None), fmt
        assert "format" in binding.last_error()
    # header + footer + one byte: 1, 7 and 19 bytes at the least
    for fmt, least in ((binding.FMT_DEFLATE, 1), (binding.FMT_ZLIB, 7), (binding.FMT_GZIP, 19)):
        assert refused(fake, fmt, d, 16, d, least - 1, d, None), fmt
        assert "out_avail" in binding.last_error()
        assert refused(fake, fmt, None, 0, d, least - 1, d, None), fmt


def test_python_interface_has_the_call():
    from libdeflate_amd import api
    assert callable(api.Compressor.compress_large_batch)
