"""BGZF files on the GPU (libdeflate_amd_bgzf_compress[_batch] and the
LIBDEFLATE_AMD_BGZF format of the compress batch).  Python's gzip / zlib and
the spec walker of tests/bgzf_walk.py are the oracles: structure, decoding,
the index, the output-space rule, caller-cut blocks, and byte identity with
the per-block GZIP streams (the deflate body must not change) and between
the host and the device calls."""
import gzip
import random
import zlib

import numpy as np
import pytest

from libdeflate_amd import binding
from tests import bgzf_walk, datagen

pytestmark = pytest.mark.gpu

B = 65280


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


_comps = {}


def _comp(level):
    from libdeflate_amd import api
    if level not in _comps:
        _comps[level] = api.Compressor(level)
    return _comps[level]


_base = {}


def _file(n, seed):
    """n bytes: a cycle of 64 datagen chunks of 64 KiB (text, binary, runs,
    random), so neighbouring BGZF blocks differ"""
    if seed not in _base:
        _base[seed] = b"".join(datagen.chunk(i, 65536, seed) for i in range(64))
    b = _base[seed]
    return (b * (n // len(b) + 1))[:n]


def _num_cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev_file(torch, c, data, eof=True, index=True, out_avail=None, canary=64):
    """the device call -> (file bytes or None, index rows, raw out tensor)"""
    n = len(data)
    m = -(-n // B)
    d_in = torch.frombuffer(bytearray(data) + bytearray(16), dtype=torch.uint8).cuda()
    avail = c.bgzf_bound(n) if out_avail is None else out_avail
    out = torch.full((avail + canary,), 0xA5, dtype=torch.uint8, device="cuda")
    nb = torch.zeros(1, dtype=torch.int64, device="cuda")
    idx = torch.zeros(2 * (m + 1), dtype=torch.int64, device="cuda") if index else None
    c.compress_bgzf_batch(d_in, out, nb, index=idx, eof=eof, in_nbytes=n, out_avail=avail)
    torch.cuda.synchronize()
    size = int(nb.item())
    host = out.cpu().numpy()
    assert not (host[avail:] != 0xA5).any(), "bytes written past out_avail"
    rows = idx.cpu().numpy().astype(np.uint64).reshape(m + 1, 2) if index else None
    return (host[:size].tobytes() if size else None), rows, host


def _batch(torch, c, fmt, chunks, avail=None):
    """per-chunk streams of compress_batch (no bound: the fused kernel)"""
    offs, blob = [], bytearray()
    for x in chunks:
        offs.append(len(blob))
        blob += x + bytes(-len(x) % 16 + 16)
    n = len(chunks)
    av = [65536] * n if avail is None else avail
    oo = [sum(a + 32 for a in av[:i]) for i in range(n)]
    data = torch.frombuffer(blob + bytearray(64), dtype=torch.uint8).cuda()
    out = torch.zeros(sum(a + 32 for a in av) + 64, dtype=torch.uint8, device="cuda")
    t = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    nb = t([0] * n)
    c.compress_batch(fmt, data, t(offs), t([len(x) for x in chunks]), out, t(oo), t(av), nb)
    torch.cuda.synchronize()
    h, sz = out.cpu().numpy(), nb.cpu().tolist()
    return [h[o:o + s].tobytes() if s else None for o, s in zip(oo, sz)]


def _check_file(f, data, rows=None, eof=True):
    members, has_eof = bgzf_walk.walk(f, require_eof=eof)
    m = -(-len(data) // B)
    assert has_eof == eof and len(members) == m
    assert all(x.isize == B for x in members[:-1])
    assert all(x.size <= 65536 for x in members)
    assert b"".join(x.data for x in members) == data
    if eof:
        assert f[-28:] == bgzf_walk.EOF_MEMBER
        assert gzip.decompress(f) == data
    if rows is not None:
        for k, x in enumerate(members):
            assert (int(rows[k][0]), int(rows[k][1])) == (x.offset, k * B)
            d = zlib.decompressobj(31)
            one = d.decompress(f[x.offset:x.offset + x.size])
            assert one == data[k * B:k * B + x.isize] and d.eof
        assert (int(rows[m][0]), int(rows[m][1])) == (len(f) - (28 if eof else 0), len(data))
    return members


@pytest.mark.parametrize("n", [0, 1, 65279, 65280, 65281, 4 * 65280, 5 * 65280 + 7])
def test_bgzf_file_structure_index_and_decoding(torch, dec, n):
    c = _comp(6)
    data = _file(n, 0xB62F0001)
    f, rows, _ = _dev_file(torch, c, data)
    assert f is not None
    members = _check_file(f, data, rows)
    if n == 0:
        assert f == bgzf_walk.EOF_MEMBER
    # one indexed device batch through the members decoder
    r, ain, aout, nm, out = dec.gzip_decompress_members(f, max(n, 1))
    assert (r, ain, aout, out) == (0, len(f), n, data)
    assert nm in (len(members), len(members) + 1)   # (+ the EOF member)
    # the member bytes are what the compress batch gives every block
    if n:
        assert _batch(torch, c, "bgzf", [data[k:k + B] for k in range(0, n, B)]) == \
            [f[x.offset:x.offset + x.size] for x in members]


@pytest.mark.parametrize("level", [1, 6, 9])
def test_bgzf_split_and_fused_paths_match_per_block_batches(torch, level):
    """>= 4 blocks per CU: the split (LZ77 + entropy) path; a few blocks: the
    fused kernel.  Both files hold exactly the members of per-block calls"""
    c = _comp(level)
    big = _file(4 * _num_cus(torch) * B - 1000, 0xB62F0002)
    for data in (big, big[:3 * B + 99]):
        f, rows, _ = _dev_file(torch, c, data)
        members = _check_file(f, data, rows if len(data) < len(big) else None)
        want = _batch(torch, c, "bgzf", [data[k:k + B] for k in range(0, len(data), B)])
        assert [f[x.offset:x.offset + x.size] for x in members] == want


def test_bgzf_body_is_the_gzip_body_at_every_level(torch):
    data = _file(6 * B + 4321, 0xB62F0003)
    blocks = [data[k:k + B] for k in range(0, len(data), B)]
    for level in range(13):
        c = _comp(level)
        f, _, _ = _dev_file(torch, c, data, index=False)
        members = _check_file(f, data)
        gz = _batch(torch, c, "gzip", blocks)
        for x, g in zip(members, gz):
            assert f[x.offset + 18:x.offset + x.size] == g[10:], (level, x.offset)


def test_bgzf_incompressible_input_fits_at_every_level(torch):
    data = np.random.default_rng(0xB62F).integers(0, 256, 3 * B + 5, dtype=np.uint8).tobytes()
    for level in range(13):
        f, _, _ = _dev_file(torch, _comp(level), data, index=False)
        assert f is not None, level
        members = _check_file(f, data)
        assert max(x.size for x in members) <= 65536


def test_bgzf_no_eof_appends_and_gzi(torch):
    c = _comp(6)
    a, b = _file(2 * B + 17, 0xB62F0004), _file(B - 3, 0xB62F0005)
    fa, ra, _ = _dev_file(torch, c, a, eof=False)
    fb, _, _ = _dev_file(torch, c, b, eof=False)
    assert int(ra[-1][0]) == len(fa) and not fa.endswith(bgzf_walk.EOF_MEMBER)
    whole = fa + fb + bgzf_walk.EOF_MEMBER
    members, has_eof = bgzf_walk.walk(whole)
    assert has_eof and [x.isize for x in members] == [B, B, 17, B - 3]
    assert b"".join(x.data for x in members) == a + b == gzip.decompress(whole)
    # nothing to write: an empty input without the EOF member
    assert _dev_file(torch, c, b"", eof=False)[0] is None
    # the .gzi helper round-trips the index of a real file
    from libdeflate_amd import api
    data = _file(3 * B + 1, 0xB62F0006)
    f, rows = c.compress_bgzf(data, index=True)
    assert np.array_equal(api.bgzf_gzi_parse(api.bgzf_gzi(rows)), rows[1:-1])
    _check_file(f, data, rows)


def test_bgzf_output_space_and_canaries(torch):
    c = _comp(6)
    data = _file(3 * B + 500, 0xB62F0007)
    f, _, _ = _dev_file(torch, c, data)
    size = len(f)
    got, _, raw = _dev_file(torch, c, data, out_avail=size)
    assert got == f
    got, _, raw = _dev_file(torch, c, data, out_avail=size - 1)
    assert got is None      # (the canaries past out_avail are checked in _dev_file)
    got, _, raw = _dev_file(torch, c, data, out_avail=size - 28, eof=False)
    assert got == f[:-28]
    assert _dev_file(torch, c, data, out_avail=size - 29, eof=False)[0] is None
    # the host call: the same rule
    assert c.compress_bgzf(data, out_avail=size) == f
    assert c.compress_bgzf(data, out_avail=size - 1) is None


def test_bgzf_caller_cut_blocks(torch):
    """htslib cuts blocks at record boundaries: compress_batch(BGZF) on chunks
    of any size up to 65280 gives one member each; 65281 bytes report 0"""
    c = _comp(6)
    rng = random.Random(0xB62F)
    recs = [datagen.text_chunk(rng.randrange(1, B + 1), 0xB62F0100 + i) for i in range(40)]
    recs += [bytes(B), _file(B, 0xB62F0008)]
    got = _batch(torch, c, "bgzf", recs + [bytes(B + 1)])
    assert got[-1] is None
    whole = b"".join(got[:-1]) + bgzf_walk.EOF_MEMBER
    members = bgzf_walk.walk(whole)[0]
    assert [x.data for x in members] == recs
    # an empty chunk is an empty member (at level 6 byte for byte the EOF member)
    empty = _batch(torch, c, "bgzf", [b""])[0]
    assert empty[:16] == bgzf_walk.PREFIX and gzip.decompress(empty) == b""
    assert empty[16] | empty[17] << 8 == len(empty) - 1
    # a slot below the member's size reports 0 like any other format
    small = _batch(torch, c, "bgzf", recs[:3], avail=[len(g) - 1 for g in got[:3]])
    assert small == [None] * 3
    # the host-pointer batch takes the format too
    assert c.compress_batch_host("bgzf", recs[:8]) == got[:8]


def test_bgzf_host_call_matches_the_device_call(torch):
    """the host form (slices of 8 blocks per CU) gives the device call's bytes
    and index, also for an input of more than one slice"""
    c = _comp(6)
    for n in (0, 5 * B + 3, 8 * _num_cus(torch) * B + 3 * B + 11):
        data = _file(n, 0xB62F0009)
        fd, rd, _ = _dev_file(torch, c, data)
        fh, rh = c.compress_bgzf(data, index=True)
        assert fh == fd and np.array_equal(rh, rd), n
        if n > 10 * B:
            _check_file(fh, data)
            # no room for the EOF member: found by the last slice's drain
            assert c.compress_bgzf(data, out_avail=len(fh) - 1) is None


def test_bgzf_format_is_refused_where_it_has_no_meaning(torch):
    from libdeflate_amd import api
    d = api.Decompressor()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    rc = d._lib.libdeflate_amd_decompress_batch(
        d._h, binding.FMT_BGZF, 1, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
        t.data_ptr(), t.data_ptr(), t.data_ptr(), None, None, None)
    assert rc == -2
