"""The step catalogue of tests/object_steps.py, checked without the library:
every step's `expected` is held against a second CPU source (zlib, gzip,
zipfile, tarfile, the oracle, the models), so that the GPU sequence tests
never hold the code under test against itself.  Runs without a GPU."""
import pytest

from tests import object_steps as O

# the call families the issue names; a catalogue that lost one would hide it
D_FAMILIES = {"batch", "batch-dict", "prefix", "sizes", "packed", "zip", "zip-large", "tar", "bgzf",
              "gzip-members", "stream", "seek", "host", "refused"}
C_FAMILIES = {"compress", "compress-dict", "zip-write", "gzm-write", "png-write", "tar-write",
              "compress-large", "bgzf-write", "host"}


@pytest.fixture(scope="module")
def dsteps(oracle):
    return O.decompressor_steps(oracle)


def test_every_family_is_in_the_catalogue(dsteps):
    assert {s.family for s in dsteps.values()} == D_FAMILIES
    assert {s.family for s in O.compressor_steps().values()} == C_FAMILIES
    for name, s in list(dsteps.items()) + list(O.compressor_steps().items()):
        assert s.name == name and s.fields and s.expected is not None, name
        assert s.family in O.__doc__ and s.fields in O.__doc__, name     # the docstring's table
    blocking = {n for n, s in dsteps.items() if s.blocking}
    assert blocking == {"zip-large", "large", "large-damaged", "large-index", "seek-read",
                        "batch-host", "ex-host"}


def test_decompressor_steps_expect_what_the_cpu_references_say(dsteps):
    for s in dsteps.values():
        s.validate()


def test_compressor_steps_expect_what_the_cpu_references_say():
    for s in O.compressor_steps().values():
        s.validate()


def test_the_shapes_reach_the_paths_they_are_there_for(dsteps):
    """both sides of what a call decides on, so that a catalogue edited later
    cannot quietly lose a path"""
    b = dsteps["batch-synth"]
    results = {e[0] for e in b.expected}
    assert {O.SUCCESS, O.BAD_DATA, O.INSUFFICIENT_SPACE} <= results, results
    assert all(c.avail < 70000 for c in b.cases) and len(b.cases) > 100
    assert len(dsteps["batch300"].cases) == 300
    assert {e[0] for e in dsteps["batch-short"].expected} == {O.SUCCESS, O.INSUFFICIENT_SPACE}
    assert len(dsteps["prefix"].cases) == 7 and len(dsteps["sizes"].streams) == 40
    assert {e[0] for e in dsteps["dict-zlib"].expected} == {O.SUCCESS, O.BAD_DATA}
    z = dsteps["zip"]
    methods = {row[2] & 0xFFFF for row in z.expected.rows}
    assert methods == {0, 8} and b"PK\6\6" in z.data
    assert dsteps["zip-defect"].expected.results.count(O.BAD_DATA) == 1
    assert dsteps["zip-overflow"].expected.words[0] == 17       # MORE_CANDIDATES
    assert dsteps["tar-overflow"].expected.words[0] == 17
    assert dsteps["zip-space"].expected.words[0] == O.INSUFFICIENT_SPACE
    assert dsteps["large-damaged"].expected[0] != O.SUCCESS
    assert any(len(n.encode()) > 100 for n in O.compressor_steps()["c-tar"].names)


class _Bounds:
    """a stand-in for the Compressor in prepare(): room enough, no device"""
    level = 6

    def bound(self, fmt, n):
        return n + 64

    def bgzf_bound(self, n):
        return n + 1000

    def zip_bound(self, names, sizes, flags=0):
        return sum(sizes) + 10000

    def gzip_members_compress_bound(self, sizes, names=None):
        return sum(sizes) + 10000

    def png_encode_bound(self, images):
        return O.pw.bound(images)

    def tar_write_size(self, names, sizes):
        return len(O.tw.tarfile_bytes(names, [bytes(n) for n in sizes]))


def test_every_device_output_check_fails_on_outputs_that_nothing_wrote(dsteps, monkeypatch):
    """the checks themselves, on host tensors: a call that wrote nothing (or a
    refusal that did not come) is found by the check of every step that has
    device outputs - every decompressor step but large-index and seek-read
    (whose index comes back through the host), large-damaged (nothing of its
    output is defined) and the two host-pointer steps, and every compressor
    step but the three host-pointer ones.  What a call returns to the host is
    set to the right answer, so that it is the untouched tensors that fail."""
    import numpy as np
    import torch
    monkeypatch.setattr(O, "DEVICE", "cpu")
    seen = 0
    for name, s in dsteps.items():
        if s.family == "host" or isinstance(s, O.LargeIndex) or name == "large-damaged":
            continue
        h = s.prepare(torch)
        h.error = None                                      # (Refused: no exception came)
        if hasattr(s, "offs") and hasattr(s, "sel"):        # (a selection: the offsets are right)
            h.offs = np.array(s.offs, dtype=np.uint64)
        if isinstance(s, O.Large):
            h.got, h.stats = s.expected[:3], {"parallel": s.parallel}
        with pytest.raises(AssertionError):
            s.check(h)
        seen += 1
    assert seen == len(dsteps) - 5
    for name, s in O.compressor_steps().items():
        if s.family == "host":
            continue
        h = s.prepare(torch, _Bounds())
        if isinstance(s, O.CTar):
            h.rows = np.array(O.tar_walk.read(s.archive, 64, extract=False).rows, dtype=np.uint64)
        with pytest.raises(AssertionError):
            s.check(h)
        seen += 1
    assert seen == len(dsteps) - 5 + len(O.compressor_steps()) - 3


# ------------------------------------------- the PNG decodes, the shuffle read

R_FAMILIES = {"png", "png-pixels", "png-adam7", "shuffle", "refused"}


@pytest.fixture(scope="module")
def rsteps():
    return O.reader_steps()


def test_the_reader_steps_are_a_catalogue_of_their_own(dsteps, rsteps):
    assert {s.family for s in rsteps.values()} == R_FAMILIES
    assert not set(rsteps) & set(dsteps)    # (the seeded shuffles draw from dsteps alone)
    for name, s in rsteps.items():
        assert s.name == name and s.fields and s.expected is not None and not s.blocking, name
        assert s.family in O.__doc__ and s.fields in O.__doc__, name
    calls = {s.call for s in rsteps.values() if isinstance(s, O.PngDecode)}
    assert calls == {"decode_png_batch", "decode_png_pixels_batch", "decode_png_batch_ex"}


def test_reader_steps_expect_what_the_cpu_models_say(rsteps):
    for s in rsteps.values():
        s.validate()


def test_the_reader_inputs_reach_every_stage(rsteps):
    files = O.png_files()
    assert len(files) == 7 and all(f.width <= 64 and f.height <= 64 for f in files)
    rows = rsteps["png-ex"].rows
    assert any(f.colour == 3 and r[6] and r[7] for f, r in zip(files, rows)), "no palette with tRNS"
    assert any(f.depth == 16 for f in files) and any(f.width == 1 for f in files)
    narrow = [f for f, r in zip(files, rows) if O.p7m.is_interlaced(r) and f.width < 8]
    assert narrow and any((0, 0) in O.p7m.pass_sizes(f.width, f.height) for f in narrow)
    # the plain calls: a zero row among the images; the pixel format: rooms the
    # unfilter writes and rooms the convert writes; the _ex calls: interlaced
    # and plain selections, with and without the convert behind them
    assert {O.SUCCESS, O.UNSUPPORTED} == set(rsteps["png"].results)
    assert set(rsteps["png-zero"].results) == {O.UNSUPPORTED} and rsteps["png-zero"].offs == [0, 0, 0]
    for name in ("png-pixels", "png-ex"):
        s = rsteps[name]
        direct = {O.px.is_direct(files[k].depth, files[k].colour, s.fmt) for k in s.sel
                  if not O.pm.is_zero(s.rows[k])}
        assert direct == {True, False}, name
    for name in ("png-ex", "png-ex-raw"):
        s = rsteps[name]
        assert {O.p7m.is_interlaced(s.rows[k]) for k in s.sel} == {True, False}, name
        assert set(s.results) == {O.SUCCESS}, name
    sh = rsteps["shuffle"]
    assert 8 <= len(sh.rows) <= 10 and max(r[3] for r in sh.rows) <= 5 << 12
    classes = {O.sm.classify(r) for r in sh.rows}
    assert classes >= {O.sm.DECODE_DIRECT, O.sm.DECODE_UNSHUFFLE, O.sm.STORED_UNSHUFFLE,
                       O.sm.STORED_COPY}, classes
    assert any(r[5] == O.sm.NO_DEFLATE for r in sh.rows) and any(r[5] == O.sm.NO_SHUFFLE for r in sh.rows)
    assert any(O.sm.GEN_BYTES % r[4] and not O.sm.identity(r[3], r[4], r[5]) for r in sh.rows)
    assert any(O.sm.tiles(r[3], r[4]) > 1 for r in sh.rows)


def test_every_reader_check_fails_on_outputs_that_nothing_wrote(rsteps, monkeypatch):
    """as for the older catalogue: the right offsets, no exception from a
    refused call, and tensors nothing wrote"""
    import numpy as np
    import torch
    monkeypatch.setattr(O, "DEVICE", "cpu")
    for name, s in rsteps.items():
        h = s.prepare(torch)
        h.error = None
        if hasattr(s, "offs"):
            h.offs = np.array(s.offs, dtype=np.uint64)
        with pytest.raises(AssertionError):
            s.check(h)
