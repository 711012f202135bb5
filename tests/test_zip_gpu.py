"""ZIP archives read on the GPU (libdeflate_amd_zip_index_batch /
_decompress_batch / _read_batch).  No tolerance anywhere: every entry's bytes
equal zipfile's, index rows, result words and per-entry results equal what the
CPU model (tools/models/zip_walk.py) states, and nothing is written where
nothing may be."""
import numpy as np
import pytest

from tests import zip_files as zf
from tools.models import zip_walk

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
MORE_ENTRIES, MORE_CANDIDATES, UNSUPPORTED = 16, 17, 18
CANARY = 0xA5
UNSET = -7      # d_results where nothing was written
# what lies behind in_nbytes in the device buffer: an end record that is not
# seen, because nothing at or past in_nbytes is part of the file
BEHIND = b"PK\5\6" + b"\0" * 18
DEFECTS = {d.name: d for d in zf.defects()}


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


def _read(torch, dec, data, max_entries, out_avail, align=1, decode=True):
    """-> (result words, output as numpy (out_avail + 64 bytes, 0xA5 where
    nothing was written), index rows (-1 where nothing was written), per-entry
    results (UNSET where nothing was written))"""
    d_in = _up(torch, data)
    out = torch.full((out_avail + 64,), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * max_entries,), -1, dtype=torch.int64, device="cuda")
    per = torch.full((max_entries,), UNSET, dtype=torch.int32, device="cuda")
    if decode:
        dec.decompress_zip_batch(d_in, max_entries, out, res, per, index=idx, out_align=align,
                                 in_nbytes=len(data), out_avail=out_avail)
    else:
        dec.index_zip_batch(d_in, max_entries, res, per, index=idx, out_align=align,
                            in_nbytes=len(data))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert not (host[out_avail:] != CANARY).any(), "bytes written past out_avail"
    words = [int(x) for x in res.cpu().tolist()]
    return words, host, idx.cpu().numpy().reshape(-1, 8), per.cpu().numpy()


def _untouched(host, rows=None, per=None):
    assert not (host != CANARY).any(), "d_out was written"
    if rows is not None:
        assert (rows == -1).all(), "d_index was written"
    if per is not None:
        assert (per == UNSET).all(), "d_results was written"


def _image(rows, datas, size):
    """the output as it has to be: every entry at its out_off, 0xA5 elsewhere"""
    want = np.full(size, CANARY, dtype=np.uint8)
    for row, b in zip(rows, datas):
        if b:
            want[row[7]:row[7] + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return want


def _check_good(torch, dec, g, max_entries, align):
    infos, datas = zf.expected(g)
    m = len(infos)
    model = zip_walk.read(g.data, max_entries, out_align=align)
    total = model.words[3]
    assert model.words[:2] == [SUCCESS, m] and model.plain == datas
    words, host, rows, per = _read(torch, dec, g.data, max_entries, total, align)
    assert words == model.words, g.name
    assert rows[:m].tolist() == model.rows and (rows[m:] == -1).all(), g.name
    assert not per[:m].any() and (per[m:] == UNSET).all(), g.name
    assert np.array_equal(host, _image(model.rows, datas, total + 64)), g.name
    for row, zi in zip(rows[:m].tolist(), infos):
        assert row[3] == zi.CRC and row[6] == zi.file_size and row[7] % align == 0
    # the index call: the same rows and words, nothing decoded
    iwords, _, irows, iper = _read(torch, dec, g.data, max_entries, 0, align, decode=False)
    assert iwords == words and np.array_equal(irows, rows) and np.array_equal(iper, per)
    return words, rows


@pytest.mark.parametrize("align", (1, 16, 256))
@pytest.mark.parametrize("name", zf.GOOD_NAMES)
def test_good_files(torch, dec, name, align):
    """entries of 0 bytes to 300 000 at levels 1 / 6 / 9 and stored, archive
    comments up to the search window's far edge, data descriptors, ZIP64,
    65 600 entries, bytes behind the end record, false candidates, no entry at
    all; max_entries exact and 16 times that"""
    g = zf.good(name)
    m = max(len(zf.expected(g)[0]), 1)
    a = _check_good(torch, dec, g, m, align)
    b = _check_good(torch, dec, g, 16 * m, align)
    assert a[0] == b[0] and np.array_equal(a[1][:m], b[1][:m])


def test_false_candidates_were_there(torch, dec):
    f = zf.good("false")
    end = zip_walk.find_end(f.data)
    assert len(zip_walk.candidates(f.data, end)) > end.entries


@pytest.mark.parametrize("n", (0, 1, 21, 22, 5000))
def test_no_archive(torch, dec, n):
    words, host, rows, per = _read(torch, dec, b"\0" * n, 4, 100)
    assert words == [BAD_DATA, 0, 0, 0, 0] == zip_walk.read(b"\0" * n, 4).words
    _untouched(host, rows, per)
    assert _read(torch, dec, b"\0" * n, 4, 0, decode=False)[0] == words


@pytest.mark.parametrize("name", list(DEFECTS))
def test_defects(torch, dec, name):
    """one defect per file: the verdict, the failing entry's own result, every
    neighbour's bytes; nothing written under a pre-decode verdict"""
    d = DEFECTS[name]
    infos, datas = zf.expected(d.base)
    m = len(infos)
    model = zip_walk.read(d.data, m + 1)
    total = zip_walk.read(d.base.data, m).words[3] + 8
    words, host, rows, per = _read(torch, dec, d.data, m + 1, total)
    assert words == model.words and words[0] == d.result, name
    iwords, _, irows, iper = _read(torch, dec, d.data, m + 1, 0, decode=False)
    imodel = zip_walk.read(d.data, m + 1, decode=False)
    assert iwords == imodel.words, name
    if d.entry is None:
        assert words == [BAD_DATA, 0, 0, 0, 0] == iwords
        _untouched(host, rows, per)
        assert (irows == -1).all() and (iper == UNSET).all()
        return
    assert per[:m].tolist() == model.results and per[m] == UNSET, name
    assert iper[:m].tolist() == imodel.results, name
    assert rows[:m].tolist() == model.rows == irows[:m].tolist(), name
    assert per[d.entry] == d.result and not np.delete(per[:m], d.entry).any()
    for k, row in enumerate(model.rows):
        if k != d.entry or name == "crc":   # a CRC failure keeps its slot, bytes and all
            assert host[row[7]:row[7] + row[6]].tobytes() == datas[k], (name, k)
    # nothing outside the slots
    mask = np.ones(len(host), dtype=bool)
    for k, row in enumerate(model.rows):
        if imodel.results[k] == SUCCESS:    # refused before the decode: no slot
            mask[row[7]:row[7] + row[6]] = False
    assert (host[mask] == CANARY).all(), name


def test_limits(torch, dec):
    g = zf.good("mixed1")
    infos, datas = zf.expected(g)
    m = len(infos)
    good = zip_walk.read(g.data, m)
    total = good.words[3]
    words, host, rows, per = _read(torch, dec, g.data, m - 1, total)
    assert words == [MORE_ENTRIES, m, 0, 0, 0] == zip_walk.read(g.data, m - 1).words
    _untouched(host, rows, per)
    assert _read(torch, dec, g.data, m - 1, 0, decode=False)[0] == words
    for align in (1, 256):
        ga = zip_walk.read(g.data, m, out_align=align)
        need = ga.words[3]
        words, host, rows, per = _read(torch, dec, g.data, m, need - 1, align)
        assert words == [INSUFFICIENT_SPACE, m, good.words[2], need, 0]
        assert words == zip_walk.read(g.data, m, out_avail=need - 1, out_align=align).words
        _untouched(host)
        assert rows.tolist() == ga.rows and not per.any()   # the index is there
        # exactly enough room: _check_good reads into exactly that, canary behind it
        _check_good(torch, dec, g, m, align)
    # MORE_ENTRIES comes before the space, the end record before both
    assert _read(torch, dec, g.data, m - 1, 0)[0][0] == MORE_ENTRIES
    assert _read(torch, dec, DEFECTS["cd_off+1"].data, 1, 0)[0] == [BAD_DATA, 0, 0, 0, 0]
    assert _read(torch, dec, DEFECTS["count+1"].data, 6, 0)[0] == [MORE_ENTRIES, 7, 0, 0, 0]


def test_candidate_overflow(torch, dec):
    la = zf.lookalikes()
    k = len(zip_walk.candidates(la.data, zip_walk.find_end(la.data)))
    for mm in (1, k - 1024 - 1):
        words, host, rows, per = _read(torch, dec, la.data, mm, 100)
        assert words == [MORE_CANDIDATES, k, 0, 0, 0] == zip_walk.read(la.data, mm).words
        _untouched(host, rows, per)
        assert _read(torch, dec, la.data, mm, 0, decode=False)[0] == words
    _check_good(torch, dec, la, k - 1024, 1)


def _select(torch, dec, data, rows, sel, align, out_avail=None):
    sel = list(sel)
    offs_m, res_m, plain_m = zip_walk.read_selection(data, rows, sel, out_align=align)
    avail = offs_m[-1] if out_avail is None else out_avail
    out = torch.full((avail + 64,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((max(len(sel), 1),), UNSET, dtype=torch.int32, device="cuda")
    offs = dec.read_zip_batch(_up(torch, data), rows, sel, out, per, out_align=align,
                              in_nbytes=len(data), out_avail=avail)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert not (host[avail:] != CANARY).any(), "bytes written past out_avail"
    assert offs.tolist() == offs_m
    assert per.cpu().numpy()[:len(sel)].tolist() == res_m
    return host, offs_m, res_m, plain_m


@pytest.mark.parametrize("align", (1, 16))
def test_read_selections(torch, dec, align):
    """one entry, all entries reversed, duplicates, none, an empty entry, a
    stored entry: bytes and offsets are exact"""
    g = zf.good("mixed0")
    infos, datas = zf.expected(g)
    m = len(infos)
    _, _, rows, _ = _read(torch, dec, g.data, m, 0, decode=False)
    names = [zi.filename for zi in infos]
    empty, stored = names.index("dir/e0.bin"), names.index("dir/e4096.bin")
    assert infos[stored].compress_type == 0 and infos[empty].file_size == 0
    for sel in ([12], list(range(m))[::-1], [3, 3, 12, 3, 0, 12], [], [empty], [stored],
                [empty, stored, empty]):
        host, offs, res, plain = _select(torch, dec, g.data, rows, sel, align)
        assert res == [SUCCESS] * len(sel)
        want = np.full(len(host), CANARY, dtype=np.uint8)
        for r, k in enumerate(sel):
            assert plain[r] == datas[k]
            want[offs[r]:offs[r] + len(datas[k])] = np.frombuffer(datas[k], dtype=np.uint8)
        assert np.array_equal(host, want), sel


@pytest.mark.parametrize("name", ("crc", "deflate_byte", "usize+1", "flag_bit0", "stored_sizes"))
def test_read_a_defect_entry_fails_alone(torch, dec, name):
    d = DEFECTS[name]
    infos, datas = zf.expected(d.base)
    m = len(infos)
    _, _, rows, _ = _read(torch, dec, d.data, m, 0, decode=False)
    sel = [0, d.entry, m - 1, d.entry, 1]
    host, offs, res, plain = _select(torch, dec, d.data, rows, sel, 1)
    assert res == [d.result if k == d.entry else SUCCESS for k in sel]
    for r, k in enumerate(sel):
        if k != d.entry:
            assert host[offs[r]:offs[r] + len(datas[k])].tobytes() == datas[k]


def test_read_refuses_before_any_device_work(torch, dec):
    g = zf.good("zip64")
    m = len(zf.expected(g)[0])
    _, _, rows, _ = _read(torch, dec, g.data, m, 0, decode=False)
    out = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((4,), UNSET, dtype=torch.int32, device="cuda")
    need = int(rows[1][6])
    for kw, sel in ((dict(out_avail=need - 1), [1]), (dict(in_nbytes=int(rows[1][4])), [1]),
                    (dict(), [m])):
        with pytest.raises(RuntimeError, match="zip_read_batch"):
            dec.read_zip_batch(_up(torch, g.data), rows, sel, out, per,
                               **{"in_nbytes": len(g.data), **kw})
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all() and (per.cpu().numpy() == UNSET).all()


@pytest.mark.parametrize("name", zf.GOOD_NAMES)
def test_entry_names(torch, dec, name):
    from libdeflate_amd import api
    g = zf.good(name)
    infos, _ = zf.expected(g)
    m = max(len(infos), 1)
    d_in = _up(torch, g.data)
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * m,), -1, dtype=torch.int64, device="cuda")
    per = torch.full((m,), UNSET, dtype=torch.int32, device="cuda")
    dec.index_zip_batch(d_in, m, res, per, index=idx, in_nbytes=len(g.data))
    torch.cuda.synchronize()
    assert api.zip_entry_names(d_in, res, idx) == [zi.orig_filename for zi in infos]


def test_stream_contract(torch, dec):
    """enqueued on a non-default stream behind the copy that produces the
    input; read after a synchronize of that stream only"""
    g = zf.good("mixed0")
    infos, datas = zf.expected(g)
    m = len(infos)
    model = zip_walk.read(g.data, m, out_align=16)
    total = model.words[3]
    pinned = torch.frombuffer(bytearray(g.data) + bytearray(BEHIND), dtype=torch.uint8).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
        res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        per = torch.full((m,), UNSET, dtype=torch.int32, device="cuda")
        d_in = pinned.to("cuda", non_blocking=True)
        dec.decompress_zip_batch(d_in, m, out, res, per, out_align=16, stream=s,
                                 in_nbytes=len(g.data), out_avail=total)
        h_out = torch.empty(total + 64, dtype=torch.uint8).pin_memory()
        h_res = torch.empty(5, dtype=torch.int64).pin_memory()
        h_per = torch.empty(m, dtype=torch.int32).pin_memory()
        h_out.copy_(out, non_blocking=True)
        h_res.copy_(res, non_blocking=True)
        h_per.copy_(per, non_blocking=True)
    s.synchronize()
    assert h_res.tolist() == model.words and not h_per.numpy().any()
    assert np.array_equal(h_out.numpy(), _image(model.rows, datas, total + 64))
