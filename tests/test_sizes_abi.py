"""CPU-side checks of the size query and the packed decompress: declared,
exported, bound; their arguments checked before any device work; and the
count-only kernel as the compiler reports it - no scratch, fewer registers and
less LDS than the decode kernel, and no store but those to the three result
arrays.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("libdeflate_amd_decompress_sizes_batch", "libdeflate_amd_decompress_sizes_batch_dict",
           "libdeflate_amd_decompress_sizes_batch_host", "libdeflate_amd_decompress_batch_packed")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
         "-ffp-contract=off", "-mllvm", "-disable-machine-licm", "--cuda-device-only"]
BAD_ARG, OK = -2, 0


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
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", hdr, re.M))
    assert set(SYMBOLS) <= declared
    assert set(SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    assert binding.MISSING == []
    nargs = dict(zip(SYMBOLS, (11, 13, 9, 14)))
    for s in SYMBOLS:
        assert len(getattr(lib, s).argtypes) == nargs[s], s
    from libdeflate_amd import api
    for m in ("decompress_sizes_batch", "decompress_sizes_batch_dict",
              "decompress_sizes_batch_host", "decompress_batch_packed"):
        assert callable(getattr(api.Decompressor, m))


def test_size_limit_max_is_the_same_in_header_and_binding():
    from libdeflate_amd import binding
    hdr = open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()
    v = re.search(r"#define LIBDEFLATE_AMD_SIZE_LIMIT_MAX (0x[0-9A-Fa-f]+)ull", hdr).group(1)
    assert int(v, 16) == binding.SIZE_LIMIT_MAX == 0xFFFFFFFF
    # the kernel's own constant (the limit a NULL array stands for)
    src = open(os.path.join(CSRC, "inflate_kernel.hip")).read()
    k = re.search(r"#define LDA_SIZE_LIMIT_MAX (0x[0-9A-Fa-f]+)ull", src).group(1)
    assert int(k, 16) == binding.SIZE_LIMIT_MAX


def test_bad_arguments_are_refused_without_a_device(lib):
    """Every argument is looked at before the object or a device is: the
    `object` below is 64 bytes of host memory that no call may touch."""
    from libdeflate_amd import binding
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    F = binding.FMT_DEFLATE
    sizes = lib.libdeflate_amd_decompress_sizes_batch
    sizes_dict = lib.libdeflate_amd_decompress_sizes_batch_dict
    host = lib.libdeflate_amd_decompress_sizes_batch_host
    packed = lib.libdeflate_amd_decompress_batch_packed

    def a_sizes(d=p, fmt=F, n=1, d_in=p, off=p, inn=p, lim=None, res=p, ain=None, size=p):
        return sizes(d, fmt, n, d_in, off, inn, lim, res, ain, size, None)

    def a_dict(d=p, fmt=F, n=1, dic=p, dn=16, d_in=p, off=p, inn=p, lim=None, res=p, ain=None,
               size=p):
        return sizes_dict(d, fmt, n, dic, dn, d_in, off, inn, lim, res, ain, size, None)

    def a_host(d=p, fmt=F, n=1, ins=p, inn=p, lim=None, res=p, ain=None, size=p):
        return host(d, fmt, n, ins, inn, lim, res, ain, size)

    def a_packed(d=p, fmt=F, n=1, d_in=p, off=p, inn=p, out=p, cap=64, align=16, ooff=p, res=p,
                 ain=None, aout=p):
        return packed(d, fmt, n, d_in, off, inn, out, cap, align, ooff, res, ain, aout, None)

    for call in (a_sizes, a_dict, a_host, a_packed):
        assert call(d=None) == BAD_ARG                               # NULL object
        assert "bad argument" in binding.last_error()
        for fmt in (binding.FMT_BGZF, -1, 4, 99):                    # BGZF / unknown format
            assert call(fmt=fmt) == BAD_ARG, (call.__name__, fmt)
        assert call(res=None) == BAD_ARG
        assert call(inn=None) == BAD_ARG
        assert call(d=None, n=0) == BAD_ARG
    for call in (a_sizes, a_dict):
        for k in ("d_in", "off", "size"):
            assert call(**{k: None}) == BAD_ARG, (call.__name__, k)
        assert call(n=0) == OK                                       # nothing to do
    assert a_host(ins=None) == BAD_ARG and a_host(size=None) == BAD_ARG
    assert a_host(n=0) == OK
    for k in ("d_in", "off", "out", "ooff", "aout"):
        assert a_packed(**{k: None}) == BAD_ARG, k
    for align in (0, 3, 512, 24, 1 << 20):
        assert a_packed(align=align) == BAD_ARG, align
        assert a_packed(align=align, n=0) == BAD_ARG, align
    # a dictionary: gzip takes none; a length without a pointer
    assert a_dict(fmt=binding.FMT_GZIP) == BAD_ARG
    assert "dictionary" in binding.last_error()
    assert a_dict(dic=None, dn=16) == BAD_ARG
    assert bytes(buf) == bytes(64)


def _compile(src, *extra):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC, *FLAGS, *extra, src], cwd=CSRC, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _report(rep, kernel):
    m = re.search(r"Function Name: %s\b(.*?)(?:Function Name:|\Z)" % kernel, rep, re.S)
    assert m, kernel
    return {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", m.group(1))}


def test_count_kernel_resources(lib):
    """no scratch (no spilled VGPR), at most the decode kernel's VGPRs, less
    LDS per wave (the kernels' LDS is dynamic: the library reports it)"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    nolicm = re.search(r"^NOLICM \?= (.*)$", mk, re.M).group(1).split()
    assert "inflate_sizes" in nolicm and "inflate_kernel" in nolicm
    assert re.search(r"^\$\(OBJDIR\)inflate_sizes\.o: inflate_kernel\.hip$", mk, re.M)
    opts = ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull]
    sizes = _report(_compile("inflate_sizes.hip", *opts).stderr, "lda_inflate_sizes_kernel")
    wave = _report(_compile("inflate_kernel.hip", *opts).stderr, "lda_inflate_wave_kernel")
    assert sizes["VGPRs Spill"] == 0 and sizes["ScratchSize"] == 0, sizes
    assert sizes["VGPRs"] <= wave["VGPRs"], (sizes, wave)
    assert sizes["Occupancy"] >= wave["Occupancy"] == 4, (sizes, wave)
    lds = (ctypes.c_size_t * 2)()
    lib.lda_sizes_lds_report.argtypes = [ctypes.POINTER(ctypes.c_size_t)]
    lib.lda_sizes_lds_report.restype = None
    lib.lda_sizes_lds_report(lds)
    assert 0 < lds[0] < lds[1], list(lds)
    assert 163840 // lds[0] >= 20 > 163840 // lds[1] >= 16, list(lds)


def test_count_kernel_stores_nothing_but_its_results():
    """The kernel takes no output buffer and no token scratch, and its ISA
    holds five stores to memory: actual_in (set, + footer, cleared on failure),
    results, out_nbytes - and the atomic that hands the streams out."""
    src = open(os.path.join(CSRC, "inflate_sizes.hip")).read()
    sig = re.search(r"lda_inflate_sizes_kernel\((.*?)\)\s*\{", src, re.S).group(1)
    params = [re.sub(r"/\*.*?\*/", "", x, flags=re.S).split()[-1].lstrip("*")
              for x in sig.split(",")]
    assert params == ["n_chunks", "format", "par", "next_stream", "order", "in_base", "in_offsets",
                      "in_nbytes", "limits", "results", "actual_in", "out_nbytes", "dict_len",
                      "dict_id"], params
    ptrs = re.findall(r"(const\s+)?u(?:8|32|64)\s*\*__restrict__\s+(\w+)", sig)
    assert sorted(n for c, n in ptrs if not c) == ["actual_in", "next_stream", "out_nbytes"]
    asm = _compile("inflate_sizes.hip", "-S", "-o", "-").stdout
    m = re.search(r"^lda_inflate_sizes_kernel:[^\n]*\n(.*?)\n\s*s_endpgm", asm, re.M | re.S)
    ops = [l.split()[0] for l in m.group(1).splitlines()
           if re.match(r"\s*(global|flat|buffer|scratch)_", l)]
    stores = sorted(o for o in ops if "store" in o)
    assert stores == ["global_store_dword"] + ["global_store_dwordx2"] * 4, stores
    assert [o for o in ops if "atomic" in o] == ["global_atomic_add"]
    assert not [o for o in ops if o.startswith(("scratch_", "buffer_"))]
