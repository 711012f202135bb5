"""Files of concatenated gzip members written on the GPU
(libdeflate_amd_gzip_members_compress_batch).  No tolerance anywhere: every
unnamed member equals, byte for byte, what libdeflate_gzip_compress of the same
compressor object returns for the record alone, every named member equals it
but for FLG, the name field and MTIME (the CPU model,
tools/models/gzip_members_write.py, builds the whole file from those streams);
result words and index pairs equal the model's; Python's gzip, a zlib member
walk and the project's own reader read the file back; and nothing is written
where nothing may be."""
import gzip

import numpy as np
import pytest

from tests import datagen
from tools.models import gzip_members_write as gzmw

pytestmark = pytest.mark.gpu

SUCCESS, INSUFFICIENT_SPACE = 0, 3
CANARY = 0xA5
MIB = 1 << 20
# the empty record, the smallest, both sides of the pass-through size of level
# 6 (31 bytes) and of the small-buffer kernel's 4 KiB, the segment rule's edge
# (128 KiB: 16 KiB segments), one record of 32 KiB segments
SIZES = (0, 1, 31, 32, 4096, 4097, 131071, 131072, 131073, 4 * MIB + 1)
RANDOM = 70000          # one incompressible record: stored blocks inside the stream
NAMES = (None, b"a", b"\xe9", b"n" * 65534, b"", "w/漢字.warc".encode("utf-8"), None, b"b",
         None, b"big.bin", b"noise")
# both sides of the pass-through size of levels 12, 6 and 1 (7, 31, 51 bytes),
# of 4 KiB, a whole record above it and a segmented one
SHORT = (0, 1, 7, 8, 31, 32, 51, 52, 4096, 4097, 70001, 131072 + 5)
SHORT_NAMES = (b"zero", None, b"x", None, None, b"\x80\xff", None, None, b"four-k", None, None,
               b"cut")


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


_COMPRESSORS, _MEMBERS = {}, {}


def _comp(level):
    from libdeflate_amd import api
    if level not in _COMPRESSORS:
        _COMPRESSORS[level] = api.Compressor(level)
    return _COMPRESSORS[level]


def _place(torch, records):
    """one device buffer that holds the records at offsets of their own, with
    gaps of every length mod 16 between them"""
    buf, offs = bytearray(b"\xEE" * 5), []
    for k, r in enumerate(records):
        offs.append(len(buf))
        buf += r + b"\xEE" * (1 + 3 * k % 16)
    return offs, torch.frombuffer(buf, dtype=torch.uint8).cuda()


def _cut(text, sizes):
    out, at = [], 0
    for n in sizes:
        out.append(text[at:at + n])
        at += n
    return out


@pytest.fixture(scope="module")
def case(torch):
    records = _cut(datagen.text_chunk(sum(SIZES), 0x2B1), SIZES) + [datagen.random_chunk(RANDOM, 7)]
    assert len(records) == len(NAMES)
    offs, d_in = _place(torch, records)
    return records, list(NAMES), offs, d_in


@pytest.fixture(scope="module")
def short(torch):
    records = _cut(datagen.text_chunk(sum(SHORT), 0x2B2), SHORT)
    records[3] = datagen.random_chunk(8, 9)
    offs, d_in = _place(torch, records)
    return records, list(SHORT_NAMES), offs, d_in


def _members(key, level, records):
    """what the object's single-buffer call returns for every record alone:
    computed once per file and level, shared by the tests"""
    if (key, level) not in _MEMBERS:
        c = _comp(level)
        _MEMBERS[key, level] = [c.compress("gzip", r) for r in records]
    return _MEMBERS[key, level]


def _model(key, level, records, names, mtime=0, out_avail=None):
    streams = [m[10:-8] for m in _members(key, level, records)]
    return gzmw.build(records, streams, names, mtime, level, out_avail)


def _write(torch, comp, case, out_avail, names=True, mtime=0, stream=None):
    """-> (result words, d_out as numpy (out_avail + 64 bytes, 0xA5 where
    nothing was written), index pairs (-1 where nothing was written))"""
    records, nm, offs, d_in = case
    n = len(records)
    out = torch.full((out_avail + 64,), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((n + 1, 2), -1, dtype=torch.int64, device="cuda")
    comp.gzip_members_compress((d_in, offs, [len(r) for r in records]), nm if names else None,
                               mtime, out=out, result=res, index=idx, out_avail=out_avail,
                               stream=stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert not (host[out_avail:] != CANARY).any(), "bytes written past out_avail"
    return [int(x) for x in res.cpu().tolist()], host, idx.cpu().numpy()


def _check(words, host, rows, model):
    size = model.words[1]
    assert words == model.words
    assert bytes(host[:size]) == model.data
    assert not (host[size:] != CANARY).any(), "bytes written behind the file"
    assert rows.tolist() == model.index


@pytest.fixture(scope="module")
def written(torch, case):
    """the one file the first checks share: level 6, mtime 0, room to spare"""
    records, names, offs, d_in = case
    comp = _comp(6)
    bound = comp.gzip_members_compress_bound([len(r) for r in records], names)
    assert bound == gzmw.bound([len(r) for r in records], [len(x or b"") for x in names])
    words, host, rows = _write(torch, comp, case, bound)
    assert words[0] == SUCCESS and 0 < words[1] <= bound
    return words, host, rows, bytes(host[:words[1]])


def test_gzip_reads_the_records_back(case, written):
    words, _, _, data = written
    records = case[0]
    assert gzip.decompress(data) == b"".join(records)
    assert words == [SUCCESS, len(data), sum(len(r) for r in records), len(records)]


def test_member_walk_is_the_index(case, written):
    _, _, rows, data = written
    index, plain = gzmw.walk(data)
    assert rows.tolist() == index and plain == case[0]


def test_members_are_the_single_buffer_calls(case, written):
    """an unnamed member is libdeflate_gzip_compress's bytes; a named one
    differs in FLG, the name field and - were it not 0 - MTIME"""
    words, host, rows, data = written
    records, names = case[0], case[1]
    alone = _members("case", 6, records)
    for k, (gz, name) in enumerate(zip(alone, names)):
        m = data[rows[k][0]:rows[k + 1][0]]
        if not name:
            assert m == gz, k
        else:
            assert m[:3] == gz[:3] and m[3] == 8 and gz[3] == 0, k
            assert m[4:10] == gz[4:10] and m[4:8] == b"\0\0\0\0", k
            assert m[10:10 + len(name) + 1] == name + b"\0", k
            assert m[10 + len(name) + 1:] == gz[10:], k
    # the segmented records are segmented: their streams hold the sync markers
    assert alone[7][10:-8].count(b"\x00\x00\xff\xff") >= 7
    # ... and the whole of it, with the words and the index, is the model's
    _check(words, host, rows, _model("case", 6, records, names))
    # the empty record's member
    assert data[:rows[1][0]] == b"\x1f\x8b\x08\0\0\0\0\0\0\xff\x01\0\0\xff\xff" + b"\0" * 8


def test_the_reader_reads_the_file(torch, dec, case, written):
    words, _, rows, data = written
    records = case[0]
    n, total = len(records), sum(len(r) for r in records)
    d_file = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((n + 1, 2), -1, dtype=torch.int64, device="cuda")
    dec.index_gzip_members_batch(d_file, n, res, index=idx)
    torch.cuda.synchronize()
    assert [int(x) for x in res.cpu().tolist()] == [SUCCESS, n, len(data), total, 0]
    assert np.array_equal(idx.cpu().numpy(), rows)
    out = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
    idx.fill_(-1)
    dec.decompress_gzip_members_batch(d_file, n, out, res, index=idx, out_avail=total)
    torch.cuda.synchronize()
    assert [int(x) for x in res.cpu().tolist()] == [SUCCESS, n, len(data), total, 0]
    assert np.array_equal(idx.cpu().numpy(), rows)
    got = out.cpu().numpy()
    assert bytes(got[:total]) == b"".join(records) and not (got[total:] != CANARY).any()


def test_the_reference_decodes_every_member(case, written):
    from tests import oracle_util
    ref = oracle_util.load_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    _, _, rows, data = written
    at = 0
    for k, raw in enumerate(case[0]):
        r, ain, aout, got = ref.decompress_ex("gzip", data[at:], len(raw))
        assert (r, aout, got) == (SUCCESS, len(raw), raw), k
        at += ain
        assert at == rows[k + 1][0], k
    assert at == len(data)


def test_no_records_is_a_file_of_size_0(torch):
    comp = _comp(6)
    assert comp.gzip_members_compress_bound([]) == 0
    empty = ([], [], [], torch.zeros(16, dtype=torch.uint8, device="cuda"))
    for names in (True, False):
        words, host, rows = _write(torch, comp, empty, 100, names=names)
        assert words == [SUCCESS, 0, 0, 0]
        assert not (host != CANARY).any() and rows.tolist() == [[0, 0]]
    # d_in NULL with in_avail 0, and no room at all
    none = ([b"", b""], [b"a", None], [0, 0], torch.zeros(0, dtype=torch.uint8, device="cuda"))
    words, host, rows = _write(torch, comp, none, 48)
    _check(words, host, rows, gzmw.build([b"", b""], [None, None], [b"a", None]))
    assert words[1] == (10 + 2 + 5 + 8) + (10 + 5 + 8) == 48


def test_one_byte_short_writes_nothing(torch, case, written):
    words, _, _, data = written
    got, host, rows = _write(torch, _comp(6), case, len(data) - 1)
    assert got == [INSUFFICIENT_SPACE] + words[1:]
    assert not (host != CANARY).any(), "d_out was written"
    assert (rows == -1).all(), "d_index was written"


def test_exactly_enough_room(torch, case, written):
    words, _, rows, data = written
    got, host, rows2 = _write(torch, _comp(6), case, len(data))     # (64 guard bytes behind)
    assert got == words and bytes(host[:len(data)]) == data and np.array_equal(rows2, rows)


@pytest.mark.parametrize("level", (0, 1, 6, 12))
def test_levels_on_a_short_mix(torch, short, level):
    """both sides of every level's pass-through size, of the small-buffer
    kernel's 4 KiB and of the segment rule, with names and an MTIME, and the
    same records without names: the single-buffer call's bytes"""
    records, names = short[0], short[1]
    comp = _comp(level)
    alone = _members("short", level, records)
    assert [gzip.decompress(m) for m in alone] == records
    mtime = 0x65D4A1B2
    model = _model("short", level, records, names, mtime)
    sizes = [len(r) for r in records]
    words, host, rows = _write(torch, comp, short, comp.gzip_members_compress_bound(sizes, names),
                               mtime=mtime)
    _check(words, host, rows, model)
    assert gzip.decompress(model.data) == b"".join(records)
    for k in range(len(records)):
        assert model.data[rows[k][0] + 4:rows[k][0] + 8] == mtime.to_bytes(4, "little")
    words, host, rows = _write(torch, comp, short, comp.gzip_members_compress_bound(sizes),
                               names=False)
    assert bytes(host[:words[1]]) == b"".join(alone)
    assert words == [SUCCESS, sum(len(m) for m in alone), sum(sizes), len(records)]


def test_two_calls_back_to_back_on_a_stream(torch, short, case):
    """a fresh object, a small file and then a larger one queued behind it on
    a non-default stream without a wait between them: the scratch grows for
    the second while the first may still run"""
    from libdeflate_amd import api
    comp = api.Compressor(6)
    s = torch.cuda.Stream()
    outs = []
    for key, c in (("short", short), ("case", case)):
        records, names, offs, d_in = c
        sizes = [len(r) for r in records]
        avail = comp.gzip_members_compress_bound(sizes, names)
        out = torch.full((avail + 64,), CANARY, dtype=torch.uint8, device="cuda")
        res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        idx = torch.full((len(records) + 1, 2), -1, dtype=torch.int64, device="cuda")
        outs.append((key, c, avail, out, res, idx))
    torch.cuda.synchronize()
    for key, c, avail, out, res, idx in outs:
        records, names, offs, d_in = c
        comp.gzip_members_compress((d_in, offs, [len(r) for r in records]), names, 0, out=out,
                                   result=res, index=idx, out_avail=avail, stream=s)
    s.synchronize()
    for key, c, avail, out, res, idx in outs:
        host = out.cpu().numpy()
        assert not (host[avail:] != CANARY).any()
        _check([int(x) for x in res.cpu().tolist()], host[:avail], idx.cpu().numpy(),
               _model(key, 6, c[0], c[1]))
    comp.close()
