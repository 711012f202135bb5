"""CPU-side checks of the prefix decompress: the four calls and the result
constant declared, exported and bound; their arguments checked before any
device work; the kernel's build rules and compile report; and the expectation
helper of the GPU tests (tests/prefix_expect.py) checked against zlib's
inflate() with a small avail_out.  No GPU needed."""
import collections
import ctypes
import os
import re
import subprocess

import pytest

from tests import prefix_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libdeflate_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("libdeflate_amd_decompress_prefix_batch", "libdeflate_amd_decompress_prefix_batch_dict",
           "libdeflate_amd_decompress_prefix", "libdeflate_amd_gzip_members_peek_batch")
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


def test_symbols_and_constant_declared_exported_and_bound(lib):
    from libdeflate_amd import api, binding
    hdr = open(os.path.join(ROOT, "include", "libdeflate_amd.h")).read()
    declared = set(re.findall(r"^(libdeflate_[a-z0-9_]+)\(", hdr, re.M))
    assert set(SYMBOLS) <= declared
    assert set(SYMBOLS) <= set(binding.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r" T (libdeflate_\w+)", out))
    assert binding.MISSING == []
    nargs = dict(zip(SYMBOLS, (13, 15, 7, 11)))
    for s in SYMBOLS:
        assert len(getattr(lib, s).argtypes) == nargs[s], s
    for m in ("decompress_prefix_batch", "decompress_prefix_batch_dict", "decompress_prefix",
              "peek_gzip_members_batch"):
        assert callable(getattr(api.Decompressor, m))
    # the constant: header, binding, api and the kernel's own copy; 16 to 18 are taken
    v = int(re.search(r"#define LIBDEFLATE_AMD_PREFIX\s+(\d+)", hdr).group(1))
    src = open(os.path.join(CSRC, "inflate_kernel.hip")).read()
    k = int(re.search(r"#define LDA_PREFIX (\d+)", src).group(1))
    assert v == k == binding.PREFIX == api.PREFIX == E.PREFIX == 19
    taken = {int(x) for x in re.findall(r"#define LIBDEFLATE_AMD_(?:BGZF|GZM|ZIP)_(?:MORE|UNSUP)\w+\s+(\d+)", hdr)}
    assert taken == {16, 17, 18}


def test_bad_arguments_are_refused_without_a_device(lib):
    """Every argument is looked at before the object or a device is: the
    `object` below is 64 bytes of host memory that no call may touch."""
    from libdeflate_amd import binding
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    F = binding.FMT_DEFLATE
    batch = lib.libdeflate_amd_decompress_prefix_batch
    batch_dict = lib.libdeflate_amd_decompress_prefix_batch_dict
    one = lib.libdeflate_amd_decompress_prefix
    peek = lib.libdeflate_amd_gzip_members_peek_batch

    def a_batch(d=p, fmt=F, n=1, d_in=p, off=p, inn=p, out=p, ooff=p, lim=p, res=p, ain=None,
                aout=p):
        return batch(d, fmt, n, d_in, off, inn, out, ooff, lim, res, ain, aout, None)

    def a_dict(d=p, fmt=F, n=1, dic=p, dn=16, d_in=p, off=p, inn=p, out=p, ooff=p, lim=p, res=p,
               ain=None, aout=p):
        return batch_dict(d, fmt, n, dic, dn, d_in, off, inn, out, ooff, lim, res, ain, aout, None)

    for call in (a_batch, a_dict):
        assert call(d=None) == BAD_ARG
        assert "bad argument" in binding.last_error()
        for fmt in (binding.FMT_BGZF, -1, 4, 99):
            assert call(fmt=fmt) == BAD_ARG, (call.__name__, fmt)
        for k in ("d_in", "off", "inn", "out", "ooff", "lim", "res", "aout"):
            assert call(**{k: None}) == BAD_ARG, (call.__name__, k)
        assert call(d=None, n=0) == BAD_ARG
        assert call(n=0) == OK                                       # nothing to do
    # a dictionary: gzip takes none; a length without a pointer
    assert a_dict(fmt=binding.FMT_GZIP) == BAD_ARG
    assert "dictionary" in binding.last_error()
    assert a_dict(fmt=binding.FMT_GZIP, n=0) == BAD_ARG
    assert a_dict(dic=None, dn=16) == BAD_ARG

    # the host call: a bad argument is BAD_DATA with the reason in last_error()
    ao = ctypes.c_size_t(77)
    for args in ((None, F, p, 8, p, 8, ctypes.byref(ao)), (p, 7, p, 8, p, 8, ctypes.byref(ao)),
                 (p, binding.FMT_BGZF, p, 8, p, 8, ctypes.byref(ao)),
                 (p, F, None, 8, p, 8, ctypes.byref(ao)), (p, F, p, 8, None, 8, ctypes.byref(ao)),
                 (p, F, p, 8, p, 8, None)):
        assert one(*args) == E.BAD_DATA, args
        assert "bad argument" in binding.last_error()
    # ... and so is a limit that is no size of a buffer (the staging holds it)
    for big in (ctypes.c_size_t(-1).value, ctypes.c_size_t(-1).value // 2):
        assert one(p, F, p, 8, p, big, ctypes.byref(ao)) == E.BAD_DATA
        assert "bad argument" in binding.last_error()
    assert ao.value == 77

    def a_peek(d=p, d_in=p, n=64, result=p, index=p, M=4, head=8, heads=p, sizes=p, res=p):
        return peek(d, d_in, n, result, index, M, head, heads, sizes, res, None)

    assert a_peek(d=None) == BAD_ARG
    assert "bad argument" in binding.last_error()
    for k in ("d_in", "result", "index", "heads", "sizes", "res"):
        assert a_peek(**{k: None}) == BAD_ARG, k
    for M in (0, (1 << 28) + 1):
        assert a_peek(M=M) == BAD_ARG, M
    assert a_peek(head=1 << 32) == BAD_ARG
    assert a_peek(d_in=None, n=64) == BAD_ARG       # (NULL with n == 0 is an empty file)
    assert bytes(buf) == bytes(64)


def _report(rep, kernel):
    m = re.search(r"Function Name: %s\b(.*?)(?:Function Name:|\Z)" % kernel, rep, re.S)
    assert m, kernel
    return {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", m.group(1))}


def test_prefix_kernel_build_rules_and_resources():
    """The kernel is a translation unit of its own on the NOLICM list, its
    mode a constant of that unit that the other units do not define; it has
    the wave kernel's geometry (at most 128 VGPRs, four waves per SIMD, no
    static LDS) and it does not spill: no VGPR goes to memory, no scratch
    (DESIGN 3.16 has the report)."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    nolicm = re.search(r"^NOLICM \?= (.*)$", mk, re.M).group(1).split()
    assert "inflate_prefix" in nolicm
    assert re.search(r"^\$\(OBJDIR\)inflate_prefix\.o: inflate_kernel\.hip$", mk, re.M)
    src = open(os.path.join(CSRC, "inflate_prefix.hip")).read()
    assert re.search(r"^#define LDA_INFLATE_DEVICE_ONLY$", src, re.M)
    assert re.search(r"^#define LDA_INFLATE_PREFIX 1$", src, re.M)
    for other in ("inflate_sizes.hip", "inflate_stream.hip"):
        assert "LDA_INFLATE_PREFIX" not in open(os.path.join(CSRC, other)).read()
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    opts = ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull]
    rep = {}
    for f in ("inflate_prefix.hip", "inflate_kernel.hip"):
        r = subprocess.run([HIPCC, *FLAGS, *opts, f], cwd=CSRC, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        rep[f] = r.stderr
    pre = _report(rep["inflate_prefix.hip"], "lda_inflate_prefix_kernel")
    wave = _report(rep["inflate_kernel.hip"], "lda_inflate_wave_kernel")
    print("prefix:", pre, "wave:", wave)
    assert pre["VGPRs"] <= 128 and pre["Occupancy"] == wave["Occupancy"] == 4, (pre, wave)
    assert pre["LDS Size"] == 0, pre
    assert pre["VGPRs Spill"] == 0 and pre["ScratchSize"] == 0, pre


def test_expectation_helper_agrees_with_zlib_max_length(ref):
    """Wherever the reference says INSUFFICIENT_SPACE for a sound stream,
    zlib.decompressobj(wbits).decompress(s, max_length=limit) returns exactly
    plain[:limit]: what the helper expects of the device is what zlib's
    callers get.  A few hundred (stream, limit) pairs from every group."""
    dictionary, dcases = E.dict_cases()
    cases = E.site_cases()[::3] + E.edge_cases() + E.handover_cases(ref)[::5] + dcases + \
        [c for c in E.fuzz_cases() if c.plain is not None][::2]
    seen = collections.Counter()
    for c in cases:
        E.expect(ref, c)
        assert c.want in (E.SUCCESS, E.PREFIX, E.BAD_DATA), c
        if c.want == E.PREFIX:
            assert c.aout == c.limit and c.data == c.plain[:c.limit], c
            if c.limit:
                z = E.zlib_prefix(c.fmt, c.s, c.limit, c.dictionary)
                assert z == c.plain[:c.limit], c
            seen[c.fmt] += 1
        elif c.want == E.SUCCESS:
            assert c.data == c.plain and c.aout == len(c.plain) <= c.limit, c
    assert min(seen[f] for f in ("deflate", "zlib", "gzip")) >= 100, seen


def test_hand_set_expectations_are_where_the_reference_has_no_verdict(ref):
    """The cut match with a bad offset and the cut stored block that runs past
    the input: the reference says INSUFFICIENT_SPACE for every one of them (it
    looks at the room first), which is why their BAD_DATA is set by hand."""
    hand = [c for c in E.bad_offset_cases() + E.stored_past_input_cases() if c.by_hand]
    assert len(hand) >= 15
    for c in hand:
        assert (c.want, c.aout) == (E.BAD_DATA, 0), c
        assert ref.decompress_ex(c.fmt, c.s, c.limit)[0] == E.INSUFFICIENT_SPACE, c
    # the empty offset code: the reference decodes the match as distance 1
    s = E.empty_offset_code_stream(["A", "M", "A"])
    assert ref.decompress_ex("deflate", s, 5)[::3] == (0, b"AAAAA")


def test_fuzz_seed_skips_few_cases(ref):
    """the committed seed: the damaged cases nothing can be said about stay
    under 5 % of the batch"""
    cases = [E.expect(ref, c) for c in E.fuzz_cases()]
    assert len(cases) == 512 and sum("damaged" in c.tag for c in cases) == 128
    skipped = sum(c.want is None for c in cases)
    assert skipped * 20 <= len(cases), skipped
    kinds = collections.Counter(c.want for c in cases)
    assert kinds[E.PREFIX] >= 100 and kinds[E.SUCCESS] >= 20 and kinds[E.BAD_DATA] >= 10, kinds
