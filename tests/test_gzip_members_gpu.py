"""Files of concatenated gzip members read on the GPU
(libdeflate_amd_gzip_members_decompress_batch / _index_batch).  No tolerance
anywhere: decoded bytes equal gzip.decompress(file), index rows equal the
offsets recorded while the file was built (tests/gzip_members_files.py),
result words equal what the CPU model (tools/models/gzip_chain.py) states, and
for every file the verdict - for every good file the counts too, wherever it
is read (_check_good) - equals the host loop's,
libdeflate_amd_gzip_decompress_members on the same bytes."""
import gzip

import numpy as np
import pytest

from tests import gzip_members_files as gf
from tools.models import gzip_chain

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, INSUFFICIENT_SPACE, MORE_MEMBERS, MORE_CANDIDATES = 0, 1, 3, 16, 17
CANARY = 0xA5
# what lies behind in_nbytes in the device buffer: signatures that are no
# candidates, because nothing at or past in_nbytes is part of the file
BEHIND = b"\x1f\x8b\x08\x00" * 8

SHAPES = ("one", "two", "tiny", "empties", "flagged", "stored", "mixed")
_files = {}


def _file(name):
    if name not in _files:
        if name.startswith("boundary"):
            _files[name] = gf.boundary(int(name[8:]))
        elif name.startswith("false-"):
            _files[name] = gf.false_candidates(name[6:])
        else:
            _files[name] = getattr(gf, name)()
    return _files[name]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec():
    from libdeflate_amd import api
    d = api.Decompressor()
    yield d
    d.close()


def _up(torch, data):
    return torch.frombuffer(bytearray(data) + bytearray(BEHIND), dtype=torch.uint8).cuda()


def _read(torch, dec, data, max_members, out_avail, decode=True, canary=64):
    """-> (result words, output as numpy (out_avail + canary bytes, 0xA5 where
    nothing was written), index rows (-1 where nothing was written))"""
    d_in = _up(torch, data)
    out = torch.full((out_avail + canary,), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((2 * (max_members + 1),), -1, dtype=torch.int64, device="cuda")
    if decode:
        dec.decompress_gzip_members_batch(d_in, max_members, out, res, index=idx,
                                          in_nbytes=len(data), out_avail=out_avail)
    else:
        dec.index_gzip_members_batch(d_in, max_members, res, index=idx, in_nbytes=len(data))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert not (host[out_avail:] != CANARY).any(), "bytes written past out_avail"
    words = [int(x) for x in res.cpu().tolist()]
    return words, host, idx.cpu().numpy().reshape(-1, 2)


def _untouched(host, rows=None):
    assert not (host != CANARY).any(), "d_out was written"
    if rows is not None:
        assert (rows == -1).all(), "d_index was written"


_host_loop = {}


def _host(dec, f):
    """(result, members, actual_in, actual_out) of the host loop on the same
    bytes, once per file"""
    if f.name not in _host_loop:
        r, ain, aout, members, got = dec.gzip_decompress_members(f.data, len(f.plain))
        assert got == f.plain, f.name
        _host_loop[f.name] = (r, members, ain, aout)
    return _host_loop[f.name]


def _check_good(torch, dec, f, max_members):
    """bytes, words, index, the model's words and the host loop's figures"""
    plain = gzip.decompress(f.data)
    n, total = len(f.data), len(plain)
    words, host, rows = _read(torch, dec, f.data, max_members, total)
    assert words == [SUCCESS, f.m, n, total, 0], f.name
    assert words == gzip_chain.read(f.data, max_members).words, f.name
    assert tuple(words[:4]) == _host(dec, f), f.name
    assert host[:total].tobytes() == plain, f.name
    assert np.array_equal(rows[:f.m + 1].astype(np.uint64), f.rows()), f.name
    assert (rows[f.m + 1:] == -1).all(), f.name
    return words, host, rows


@pytest.mark.parametrize("name", SHAPES)
def test_shapes(torch, dec, name):
    """one member, two, 2100 tiny ones (the 1024-candidate block of the chain
    crossed twice), empty members at the front, in the middle and at the end,
    every optional header field, stored members, 300 members of 1 byte to 200
    KiB at levels 1, 6 and 9 - and for each the host loop's (members,
    actual_in, actual_out)"""
    _check_good(torch, dec, _file(name), _file(name).m)


@pytest.mark.parametrize("at", gf.BOUNDARIES)
def test_signature_across_a_scan_step_and_a_scan_workgroup(torch, dec, at):
    f = _file(f"boundary{at}")
    assert f.members[1][0] == at
    _check_good(torch, dec, f, f.m)


@pytest.mark.parametrize("kind", gf.FALSE_KINDS)
def test_false_candidates_are_no_members(torch, dec, kind):
    """a whole member in a stored payload, two of them back to back, a
    signature in front of junk, signatures at a 3-byte stride, 300 headers
    with FNAME set in front of text without a zero byte"""
    f = _file(f"false-{kind}")
    assert len(gzip_chain.candidates(f.data)) > f.m
    _check_good(torch, dec, f, f.m)


def test_candidate_overflow(torch, dec):
    f = _file("overflow")
    total = len(f.plain)
    for mm in (1, 476):
        words, host, rows = _read(torch, dec, f.data, mm, total)
        assert words == [MORE_CANDIDATES, 1501, 0, 0, 0] == gzip_chain.read(f.data, mm).words
        _untouched(host, rows)
        assert _read(torch, dec, f.data, mm, 0, decode=False)[0] == words
    _check_good(torch, dec, f, 477)


@pytest.mark.parametrize("name", ("two", "tiny", "empties", "mixed"))
def test_more_members(torch, dec, name):
    f = _file(name)
    total = len(f.plain)
    words, host, rows = _read(torch, dec, f.data, f.m - 1, total)
    assert words == [MORE_MEMBERS, f.m, 0, 0, 0] == gzip_chain.read(f.data, f.m - 1).words
    _untouched(host, rows)
    assert _read(torch, dec, f.data, f.m - 1, 0, decode=False)[0] == words
    a = _check_good(torch, dec, f, f.m)
    b = _check_good(torch, dec, f, 16 * f.m)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ("one", "tiny", "mixed"))
def test_insufficient_space(torch, dec, name):
    f = _file(name)
    n, total = len(f.data), len(f.plain)
    words, host, rows = _read(torch, dec, f.data, f.m, total - 1)
    assert words == [INSUFFICIENT_SPACE, f.m, n, total, 0]
    assert words == gzip_chain.read(f.data, f.m, out_avail=total - 1).words
    _untouched(host)
    assert np.array_equal(rows.astype(np.uint64), f.rows())     # the index is there
    # out_avail = total: _check_good reads into exactly that, canary behind it
    _check_good(torch, dec, f, f.m)
    # the index call has no output to run out of
    assert _read(torch, dec, f.data, f.m, 0, decode=False)[0] == [SUCCESS, f.m, n, total, 0]


@pytest.mark.parametrize("name", [d[0] for d in gf.defects()])
def test_defects(torch, dec, name):
    """one defect per file: the words are the model's, the verdict the host
    loop's"""
    base, b = gf.defect_base(), dict(gf.defects())[name]
    n, total = len(base.data), len(base.plain)
    model = gzip_chain.read(b, base.m)
    words, host, rows = _read(torch, dec, b, base.m, total)
    assert words == model.words, name
    assert words[0] == dec.gzip_decompress_members(b, total)[0] == BAD_DATA
    iwords, _, irows = _read(torch, dec, b, base.m, 0, decode=False)
    assert iwords == gzip_chain.read(b, base.m, decode=False).words, name
    if name == "crc":   # the decode's verdict: everything is in place, the index too
        assert words == [BAD_DATA, base.m, n, total, 0] and iwords[0] == SUCCESS
        lo = int(base.rows()[2][1])
        hi = int(base.rows()[3][1])
        assert host[:lo].tobytes() == base.plain[:lo]
        assert host[hi:total].tobytes() == base.plain[hi:]
        assert np.array_equal(rows.astype(np.uint64), base.rows())
        assert np.array_equal(irows.astype(np.uint64), base.rows())
    else:               # refused before the decode
        assert words == [BAD_DATA, 0, 0, 0, 0] == iwords
        _untouched(host, rows)
        assert (irows == -1).all()


def test_name_limit(torch, dec):
    """FNAME + FCOMMENT of LIBDEFLATE_AMD_GZM_NAME_MAX bytes are a member's;
    one byte more is no member to this reader (the host loop has no such
    limit: the one stated difference between the two)"""
    _check_good(torch, dec, gf.long_names(gf.NAME_MAX), 3)
    g = gf.long_names(gf.NAME_MAX + 1)
    total = len(g.plain)
    words, host, rows = _read(torch, dec, g.data, g.m, total)
    assert words == [BAD_DATA, 0, 0, 0, 0] == gzip_chain.read(g.data, g.m).words
    _untouched(host, rows)
    assert dec.gzip_decompress_members(g.data, total)[:4] == (SUCCESS, len(g.data), total, g.m)


@pytest.mark.parametrize("name", ("flagged", "tiny", "false-pair"))
def test_index_call_and_packed_decode_through_the_index(torch, dec, name):
    """_index_batch rows = _decompress_batch rows = the builder's; the index's
    member offsets and lengths through decompress_batch_packed give the
    file's bytes"""
    f = _file(name)
    total = len(f.plain)
    _, _, rows = _check_good(torch, dec, f, f.m)
    words, host, irows = _read(torch, dec, f.data, f.m, 0, decode=False)
    assert words == [SUCCESS, f.m, len(f.data), total, 0]
    _untouched(host)
    assert np.array_equal(irows, rows)
    offs = torch.from_numpy(irows[:f.m, 0].copy()).cuda()
    lens = torch.from_numpy((irows[1:, 0] - irows[:-1, 0]).copy()).cuda()
    out = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
    out_offs = torch.zeros(f.m + 1, dtype=torch.int64, device="cuda")
    res = torch.full((f.m,), -1, dtype=torch.int32, device="cuda")
    aout = torch.zeros(f.m, dtype=torch.int64, device="cuda")
    dec.decompress_batch_packed("gzip", _up(torch, f.data), offs, lens, out, out_offs, res,
                                aout, out_align=1, out_capacity=total)
    torch.cuda.synchronize()
    assert not res.cpu().numpy().any()
    assert np.array_equal(out_offs.cpu().numpy(), irows[:, 1])
    assert out.cpu().numpy()[:total].tobytes() == f.plain


def test_stream_contract(torch, dec):
    """enqueued on a non-default stream behind the copy that produces the
    input; read after a synchronize of that stream only"""
    f = _file("mixed")
    n, total = len(f.data), len(f.plain)
    pinned = torch.frombuffer(bytearray(f.data) + bytearray(BEHIND), dtype=torch.uint8).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
        res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        idx = torch.full((2 * (f.m + 1),), -1, dtype=torch.int64, device="cuda")
        d_in = pinned.to("cuda", non_blocking=True)
        dec.decompress_gzip_members_batch(d_in, f.m, out, res, index=idx, stream=s,
                                          in_nbytes=n, out_avail=total)
        h_out = torch.empty(total + 64, dtype=torch.uint8).pin_memory()
        h_res = torch.empty(5, dtype=torch.int64).pin_memory()
        h_idx = torch.empty(2 * (f.m + 1), dtype=torch.int64).pin_memory()
        h_out.copy_(out, non_blocking=True)
        h_res.copy_(res, non_blocking=True)
        h_idx.copy_(idx, non_blocking=True)
    s.synchronize()
    assert h_res.tolist() == [SUCCESS, f.m, n, total, 0]
    assert h_out.numpy()[:total].tobytes() == f.plain
    assert (h_out.numpy()[total:] == CANARY).all()
    assert np.array_equal(h_idx.numpy().reshape(-1, 2).astype(np.uint64), f.rows())
