"""CPU-side checks of the seek index: libdeflate_amd_decompress_large_index
(decompress_large that also leaves an index of restart points) and
libdeflate_amd_seek_read_batch (ranged reads through it) are declared in the
header, exported by the library, described by the binding, refuse their
arguments before any device work, and exist in the Python interface."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX, READ = "libdeflate_amd_decompress_large_index", "libdeflate_amd_seek_read_batch"
BAD_DATA, BAD_ARG = 1, -2
MAGIC, END = 0x314B45455341444C, 0x21444E454B454553


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from libdeflate_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        g.build()
    return binding.load()


def test_symbols_declared_exported_and_bound(lib):
    from libdeflate_amd import binding
    hdr = open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for sym, nargs in ((INDEX, 15), (READ, 12)):
        assert sym in re.findall(r"^(libdeflate_[a-z0-9_]+)\(", hdr, re.M)
        assert sym in binding.BATCH_SYMBOLS
        assert sym in re.findall(r" T (libdeflate_\w+)", out)
        fn = getattr(lib, sym)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
    assert re.search(r"#define LIBDEFLATE_AMD_SEEK_WINDOW 32768\b", hdr)
    assert re.search(r"#define LIBDEFLATE_AMD_SEEK_WORDS 4\b", hdr)
    assert (binding.SEEK_WINDOW, binding.SEEK_WORDS) == (32768, 4)
    assert not binding.MISSING


def test_index_call_checks_its_arguments_before_any_device_work(lib):
    """What decompress_large refuses, and a capacity below 1, spacing 0, a NULL
    index / points_ret / d_windows: LIBDEFLATE_BAD_DATA with a reason that
    names what was wrong, nothing written through the result pointers.  The
    object is a stand-in: every check comes before it is used."""
    from libdeflate_amd import binding
    buf = (ctypes.c_uint8 * 4096)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    fn = getattr(lib, INDEX)
    gz = binding.FMT_GZIP
    ai, ao, npts = ctypes.c_size_t(7), ctypes.c_size_t(7), ctypes.c_size_t(7)
    index = np.full(64, 0x55, dtype=np.uint64)
    ip = index.ctypes.data_as(ctypes.c_void_p)
    pp = ctypes.byref(npts)

    def refused(word, *args):
        rc = fn(*args)
        err = binding.last_error()
        assert rc == BAD_DATA and word in err, (rc, word, err)
        assert INDEX in err
    for rets in ((ctypes.byref(ai), ctypes.byref(ao)), (None, None)):
        refused("NULL", None, gz, d, 16, d, 4096, *rets, 65536, ip, 64, pp, d, 1 << 20, None)
        refused("d_in", fake, gz, None, 16, d, 4096, *rets, 65536, ip, 64, pp, d, 1 << 20, None)
        refused("d_out", fake, gz, d, 16, None, 4096, *rets, 65536, ip, 64, pp, d, 1 << 20, None)
        for fmt in (binding.FMT_BGZF, -1, 4, 99):
            refused("format", fake, fmt, d, 16, d, 4096, *rets, 65536, ip, 64, pp, d, 1 << 20, None)
        refused("spacing", fake, gz, d, 16, d, 4096, *rets, 0, ip, 64, pp, d, 1 << 20, None)
        refused("NULL index", fake, gz, d, 16, d, 4096, *rets, 65536, None, 64, pp, d, 1 << 20, None)
        refused("NULL points_ret", fake, gz, d, 16, d, 4096, *rets, 65536, ip, 64, None, d, 1 << 20,
                None)
        refused("NULL d_windows", fake, gz, d, 16, d, 4096, *rets, 65536, ip, 64, pp, None, 1 << 20,
                None)
        # room for no point: under three rows of index, under one window
        for index_avail, windows_avail in ((11, 1 << 20), (0, 1 << 20), (64, 32767), (64, 0)):
            refused("capacity", fake, gz, d, 16, d, 4096, *rets, 65536, ip, index_avail, pp, d,
                    windows_avail, None)
    assert (ai.value, ao.value, npts.value) == (7, 7, 7)    # nothing written on a refusal
    assert (index == 0x55).all()


def _index(points, total, raw_off=10, raw_n=500, ftr=8, fmt=2):
    rows = [[MAGIC, fmt, raw_off, len(points)]]
    for k, off in enumerate(points):
        bit = 0 if k == 0 else 3 + 2 * off
        rows.append([off, bit, bit if k % 2 == 0 else bit - 1, 0 if k % 2 == 0 else 2])
    rows.append([total, raw_n, ftr, END])
    return np.array(rows, dtype=np.uint64)


def test_read_call_checks_its_arguments_before_any_device_work(lib):
    """A NULL pointer, a bad magic or format, rows that do not rise strictly,
    a closing row that needs more input than in_nbytes, a range past the total,
    ranges that need more than out_avail: LIBDEFLATE_AMD_BAD_ARG with the
    reason, on a stand-in object."""
    from libdeflate_amd import binding
    d = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_uint8 * 4096)(), ctypes.c_void_p)
    fn = getattr(lib, READ)
    good = _index([0, 100, 250, 900], 1000)
    in_n = 10 + 500 + 8
    ranges = np.array([[0, 10], [990, 10]], dtype=np.uint64)

    def call(idx=good, n=in_n, rng=ranges, avail=4096, obj=fake, din=d, win=d, dout=d, res=d,
             words=None, null_index=False, null_ranges=False):
        idx = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        rng = np.ascontiguousarray(rng, dtype=np.uint64).reshape(-1, 2)
        rc = fn(obj, din, n, None if null_index else idx.ctypes.data_as(ctypes.c_void_p),
                idx.size if words is None else words, win, len(rng),
                None if null_ranges else rng.ctypes.data_as(ctypes.c_void_p), dout, avail, res, None)
        return rc, binding.last_error()

    def refused(word, **kw):
        rc, err = call(**kw)
        assert rc == BAD_ARG and word in err and "seek_read_batch" in err, (rc, word, err)

    def edit(row, col, val):
        idx = good.copy()
        idx[row, col] = val
        return idx
    refused("decompressor", obj=None)
    refused("d_in", din=None)
    refused("index", null_index=True)
    refused("d_windows", win=None)
    refused("ranges", null_ranges=True)
    refused("d_results", res=None)
    refused("d_out", dout=None)
    refused("magic", idx=edit(0, 0, MAGIC ^ 1))
    refused("format", idx=edit(0, 1, 3))
    refused("points", idx=edit(0, 3, 0))
    refused("points", words=good.size - 1)
    refused("index_words", words=8)
    refused("end marker", idx=edit(5, 3, 0))
    refused("row 2", idx=edit(2, 0, 0))                 # out_off does not rise
    refused("row 3", idx=edit(3, 0, 100))
    refused("row 3", idx=edit(3, 1, int(good[2, 1])))   # start_bit does not rise
    refused("point 0", idx=edit(1, 1, 1))
    refused("in_nbytes", n=in_n - 1)                    # the closing row needs more input
    refused("in_nbytes", idx=edit(5, 1, 501))
    refused("past the end", rng=[[1000, 1]])
    refused("past the end", rng=[[1001, 0]])
    refused("past the end", rng=[[5, 2 ** 64 - 1]])
    refused("out_avail", avail=19)
    # no ranges: nothing to do, and nothing is touched
    rc, _err = call(rng=np.zeros((0, 2), dtype=np.uint64), dout=None, res=None)
    assert rc == 0


def test_python_interface_has_the_calls():
    from libdeflate_amd import api
    assert callable(api.Decompressor.decompress_large_index)
    assert callable(api.Decompressor.seek_read_batch)
