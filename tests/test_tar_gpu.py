"""tar archives read on the GPU (libdeflate_amd_tar_index_batch /
_extract_batch / _read_batch, and a .tar.gz through the seek index).  No
tolerance anywhere: the verdict, the five words, every index row, every
per-entry result and every extracted byte equal what the CPU model
(tools/models/tar_walk.py) states, the bytes equal tarfile's where it reads
the file, and nothing is written where nothing may be."""
import contextlib
import io
import os
import tarfile

import numpy as np
import pytest

from tests import tar_files as tf
from tools.models import tar_walk

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
MORE_RECORDS, MORE_CANDIDATES, UNSUPPORTED = 16, 17, 18
CANARY = 0xA5
UNSET = -7      # d_results where nothing was written
GUARD = 64
# what lies behind in_nbytes in the device buffer: a header that is not seen,
# because nothing at or past in_nbytes is part of the file
BEHIND = tf.member(b"behind", b"never read")


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


def _up(torch, data, shift=0):
    """the file on the device, `shift` bytes into its allocation"""
    buf = bytearray(shift) + bytearray(data) + bytearray(BEHIND)
    return torch.frombuffer(buf, dtype=torch.uint8).cuda()[shift:]


def _read(torch, dec, data, max_records, out_avail, align=1, extract=True, shift=0,
          out_shift=0):
    """-> (result words, output as numpy (out_avail + 64 bytes, 0xA5 where
    nothing was written), index rows (-1 where nothing was written), per-entry
    results (UNSET where nothing was written))"""
    d_in = _up(torch, data, shift)
    whole = torch.full((out_shift + out_avail + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    out = whole[out_shift:]
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * max_records,), -1, dtype=torch.int64, device="cuda")
    per = torch.full((max_records,), UNSET, dtype=torch.int32, device="cuda")
    if extract:
        dec.extract_tar_batch(d_in, max_records, out, res, per, index=idx, out_align=align,
                              in_nbytes=len(data), out_avail=out_avail)
    else:
        dec.index_tar_batch(d_in, max_records, res, per, index=idx, out_align=align,
                            in_nbytes=len(data))
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert not (host[:out_shift] != CANARY).any(), "bytes written in front of d_out"
    host = host[out_shift:]
    assert not (host[out_avail:] != CANARY).any(), "bytes written past out_avail"
    words = [int(x) for x in res.cpu().tolist()]
    return words, host, idx.cpu().numpy().reshape(-1, 8), per.cpu().numpy()


def _untouched(host, rows=None, per=None):
    assert not (host != CANARY).any(), "d_out was written"
    if rows is not None:
        assert (rows == -1).all(), "d_index was written"
    if per is not None:
        assert (per == UNSET).all(), "d_results was written"


def _image(rows, plain, size):
    """the output as it has to be: every entry at its out_off, 0xA5 elsewhere
    (the alignment's padding included)"""
    want = np.full(size, CANARY, dtype=np.uint8)
    for row, b in zip(rows, plain):
        if b:
            want[row[7]:row[7] + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return want


def _check(torch, dec, g, max_records, align, shift=0, out_shift=0):
    """the extract into exactly the room it needs with guard bytes behind it,
    and the index call, against the model (and tarfile)"""
    model = tar_walk.read(g.data, max_records, out_align=align)
    total, m = model.words[3], model.words[1]
    words, host, rows, per = _read(torch, dec, g.data, max_records, total, align, shift=shift,
                                   out_shift=out_shift)
    assert words == model.words, g.name
    assert rows[:m].tolist() == model.rows and (rows[m:] == -1).all(), g.name
    assert per[:m].tolist() == model.results and (per[m:] == UNSET).all(), g.name
    assert np.array_equal(host, _image(model.rows, model.plain, total + GUARD)), g.name
    if g.readable:
        exp = tf.expected(g)
        assert len(exp) == m
        for (ti, data), row in zip(exp, rows[:m].tolist()):
            assert row[4] == ti.offset_data and row[7] % align == 0
            if data is not None:
                assert host[row[7]:row[7] + row[5]].tobytes() == data, (g.name, ti.name)
    iwords, _, irows, iper = _read(torch, dec, g.data, max_records, 0, align, extract=False,
                                   shift=shift)
    assert iwords == words and np.array_equal(irows, rows) and np.array_equal(iper, per)
    return words, rows


@contextlib.contextmanager
def _serial_walk():
    """the one-lane walk instead of the scan and the chain (the switch is read
    through reload_env)"""
    from libdeflate_amd import binding
    os.environ["LDA_TAR_SERIAL"] = "1"
    binding.reload_env()
    try:
        yield
    finally:
        os.environ.pop("LDA_TAR_SERIAL", None)
        binding.reload_env()


def _records(g):
    return max(len(tar_walk.walk(g.data).records), 1)


@pytest.mark.parametrize("align", (1, 8, 256))
@pytest.mark.parametrize("name", tf.GOOD_NAMES)
def test_good_files(torch, dec, name, align):
    """the three formats with short, prefix-split, 300-character and non-ASCII
    names, empty files, sizes 1 / 511 / 512 / 513, links and directories, a
    nested archive, zero blocks inside data; the archive cut at the last
    entry's end, with one zero block, with garbage behind the marker; hand
    packed headers (base-256 size, signed checksum, V7, a hard link with a
    size); entries refused alone; max_records exact and 16 times that"""
    g = tf.good(name)
    m = _records(g)
    a = _check(torch, dec, g, m, align)
    b = _check(torch, dec, g, 16 * m, align)
    assert a[0] == b[0] and np.array_equal(a[1][:a[0][1]], b[1][:a[0][1]])


@pytest.mark.parametrize("name", ("mixed_pax", "cut_gnu", "one_zero_ustar", "empty", "unsupported",
                                  "tiles"))
def test_serial_walk_gives_the_same(torch, dec, name):
    """LDA_TAR_SERIAL: the walk kernel in place of the finder, same results"""
    g = tf.good(name)
    with _serial_walk():
        _check(torch, dec, g, _records(g), 8)
        for d in tf.defects():
            assert _read(torch, dec, d.data, 64, 0)[0] == [BAD_DATA, 0, 0, 0, 0]


def test_lookalikes_were_there():
    for fmt in tf.FORMATS:
        g = tf.mixed(fmt)
        assert len(tar_walk.candidates(g.data)) > len(tar_walk.walk(g.data).records)
    assert len(tar_walk.candidates(tf.garbage("gnu").data)) > \
        len(tar_walk.candidates(tf.mixed("gnu").data))


@pytest.mark.parametrize("at", (0, 1, 5, 31, 32, 33))
def test_nested_archive_at_several_block_offsets(torch, dec, at):
    """the inner archive's headers land in the first, the last and the middle
    blocks of a scan workgroup's range: candidates, never records"""
    d = b"".join(tf.member(b"p%02d" % i) for i in range(at))
    d += tf.member(b"nested.tar", tf.inner_tar()) + tf.member(b"z", tf.payload(3, at))
    for tail in (tf.END, b""):
        g = tf.Good("nested@%d" % at, d + tail, True)
        assert len(tar_walk.candidates(g.data)) == at + 2 + 4
        _check(torch, dec, g, at + 2, 1)


def test_unsupported_entries_fail_alone(torch, dec):
    g = tf.good("unsupported")
    words, rows = _check(torch, dec, g, 32, 1)
    assert words[0] == UNSUPPORTED and words[1] == 9
    assert words[4] == tar_walk.EOF | tar_walk.HAS_L | tar_walk.HAS_PAX


@pytest.mark.parametrize("name", tf.BIG_NAMES[:3])
def test_chain_across_a_jump_block(torch, dec, name):
    """1100 one-block files, and an L + entry and an x + entry pair whose
    extension record is record 1023 and whose entry is record 1024"""
    g = tf.good(name)
    recs = tar_walk.walk(g.data).records
    assert len(recs) > 1024
    if name != "many":
        assert g.data[512 * recs[1023] + 156] in b"Lx" and \
            g.data[512 * recs[1024] + 156] == ord("0")
    _check(torch, dec, g, len(recs), 8)


@pytest.mark.parametrize("n", (0, 511, 512, 1023))
def test_short_files(torch, dec, n):
    """no block at all is BAD_DATA; one block is what the block is"""
    for data in (bytes(n), tf.member(b"lone")[:n], tf.mixed("ustar").data[:n]):
        model = tar_walk.read(data, 4, out_avail=100)
        words, host, rows, per = _read(torch, dec, data, 4, 100)
        assert words == model.words
        if n < 512:
            assert words == [BAD_DATA, 0, 0, 0, 0]
        if model.rows is None:
            _untouched(host, rows, per)
        else:
            assert rows[:words[1]].tolist() == model.rows
        assert _read(torch, dec, data, 4, 0, extract=False)[0] == \
            tar_walk.read(data, 4, extract=False).words


@pytest.mark.parametrize("d", tf.defects(), ids=lambda d: d.name)
def test_defects(torch, dec, d):
    """a flipped checksum byte in the middle of the chain, a size that runs
    past the file, an invalid size field, a file cut inside an entry's data:
    a broken chain, and nothing is written"""
    assert tar_walk.read(d.data, 64).words == [BAD_DATA, 0, 0, 0, 0]
    words, host, rows, per = _read(torch, dec, d.data, 64, 1 << 16)
    assert words == [BAD_DATA, 0, 0, 0, 0]
    _untouched(host, rows, per)
    assert _read(torch, dec, d.data, 64, 0, extract=False)[0] == words


def test_limits(torch, dec):
    g = tf.mixed("gnu")
    recs = _records(g)
    good = tar_walk.read(g.data, recs)
    total = good.words[3]
    words, host, rows, per = _read(torch, dec, g.data, recs - 1, total)
    assert words == [MORE_RECORDS, recs, 0, 0, 0] == tar_walk.read(g.data, recs - 1).words
    _untouched(host, rows, per)
    assert _read(torch, dec, g.data, recs - 1, 0, extract=False)[0] == words
    for align in (1, 256):
        ga = tar_walk.read(g.data, recs, out_align=align)
        need = ga.words[3]
        words, host, rows, per = _read(torch, dec, g.data, recs, need - 1, align)
        assert words == [INSUFFICIENT_SPACE] + ga.words[1:]
        assert words == tar_walk.read(g.data, recs, out_avail=need - 1, out_align=align).words
        _untouched(host)
        m = words[1]
        assert rows[:m].tolist() == ga.rows and not per[:m].any()   # the index is there
        # exactly enough room: _check reads into exactly that, guard bytes behind it
        _check(torch, dec, g, recs, align)
    # MORE_RECORDS comes before the space, a broken chain before both
    assert _read(torch, dec, g.data, recs - 1, 0)[0][0] == MORE_RECORDS
    assert _read(torch, dec, tf.defects()[0].data, 1, 0)[0] == [BAD_DATA, 0, 0, 0, 0]


def test_candidate_overflow(torch, dec):
    """the nested archive of 1100 records: two records, 1102 candidates"""
    g = tf.nested_big()
    k = len(tar_walk.candidates(g.data))
    assert k == 1102
    for mm in (2, k - 1024 - 1):
        words, host, rows, per = _read(torch, dec, g.data, mm, 100)
        assert words == [MORE_CANDIDATES, k, 0, 0, 0] == tar_walk.read(g.data, mm).words
        _untouched(host, rows, per)
        assert _read(torch, dec, g.data, mm, 0, extract=False)[0] == words
    _check(torch, dec, g, k - 1024, 1)


@pytest.mark.parametrize("shift,out_shift", ((0, 0), (1, 0), (0, 3), (1, 7)))
def test_copy_tiles_and_odd_addresses(torch, dec, shift, out_shift):
    """entries of exactly one tile, one tile + 1 and three tiles - 1 bytes next
    to empty and 1-byte entries, out_align 1 so that destinations are odd,
    d_in and d_out themselves off their allocations' alignment"""
    g = tf.tiles()
    words, rows = _check(torch, dec, g, _records(g), 1, shift=shift, out_shift=out_shift)
    assert [r[5] for r in rows[:8].tolist()] == [1, tf.TILE, 0, tf.TILE + 1, 1, 3 * tf.TILE - 1,
                                                0, 17]
    assert any(r[7] % 2 for r in rows[:8].tolist())
    if not shift and not out_shift:
        _check(torch, dec, g, _records(g), 256)


def _select(torch, dec, data, rows, sel, align):
    sel = list(sel)
    offs_m, res_m, plain_m = tar_walk.read_selection(data, np.asarray(rows).tolist(), sel,
                                                     out_align=align)
    avail = offs_m[-1]
    out = torch.full((avail + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((max(len(sel), 1),), UNSET, dtype=torch.int32, device="cuda")
    offs = dec.read_tar_batch(_up(torch, data), rows, sel, out, per, out_align=align,
                              in_nbytes=len(data), out_avail=avail)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert offs.tolist() == offs_m
    assert per.cpu().numpy()[:len(sel)].tolist() == res_m
    want = np.full(len(host), CANARY, dtype=np.uint8)
    for r, b in enumerate(plain_m):
        if b:
            want[offs_m[r]:offs_m[r] + len(b)] = np.frombuffer(b, dtype=np.uint8)
    assert np.array_equal(host, want), sel
    return res_m


@pytest.mark.parametrize("align", (1, 16))
def test_read_selections(torch, dec, align):
    """out of order, with duplicates, none, empty entries, entries of several
    tiles, a refused row: bytes, offsets and results are the model's"""
    g = tf.tiles()
    _, _, rows, _ = _read(torch, dec, g.data, 8, 0, extract=False)
    for sel in ([5], list(range(8))[::-1], [3, 3, 1, 3, 0, 1], [], [2], [2, 5, 6, 7]):
        assert _select(torch, dec, g.data, rows, sel, align) == [SUCCESS] * len(sel)
    u = tf.unsupported()
    _, _, rows, _ = _read(torch, dec, u.data, 32, 0, extract=False)
    res = _select(torch, dec, u.data, rows[:9], [8, 5, 0, 6], align)
    assert res == [SUCCESS, UNSUPPORTED, SUCCESS, SUCCESS]


def test_read_refuses_before_any_device_work(torch, dec):
    g = tf.tiles()
    _, _, rows, _ = _read(torch, dec, g.data, 8, 0, extract=False)
    out = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((4,), UNSET, dtype=torch.int32, device="cuda")
    for kw, sel in ((dict(out_avail=16), [7]), (dict(in_nbytes=int(rows[7][4]) + 16), [7]),
                    (dict(), [8])):
        with pytest.raises(RuntimeError, match="tar_read_batch"):
            dec.read_tar_batch(_up(torch, g.data), rows, sel, out, per,
                               **{"in_nbytes": len(g.data), **kw})
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all() and (per.cpu().numpy() == UNSET).all()


@pytest.mark.parametrize("name", ("mixed_ustar", "mixed_gnu", "mixed_pax", "hand"))
def test_entry_names(torch, dec, name):
    from libdeflate_amd import api
    g = tf.good(name)
    m = _records(g)
    d_in = _up(torch, g.data)
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * m,), -1, dtype=torch.int64, device="cuda")
    per = torch.full((m,), UNSET, dtype=torch.int32, device="cuda")
    dec.index_tar_batch(d_in, m, res, per, index=idx, in_nbytes=len(g.data))
    torch.cuda.synchronize()
    got = api.tar_entry_names(d_in, res, idx)
    assert [x.rstrip("/") for x in got] == [ti.name.rstrip("/") for ti, _ in tf.expected(g)]


def test_targz_through_the_seek_index(torch, dec):
    """a .tar.gz of about 1 MiB of text, gzip level 6 (far above the 16 384
    input bytes from which the many-wave decoder answers): decoded and indexed
    once, then the first, a middle and the last entry out of the compressed
    bytes, and the same entries from the decoded buffer"""
    from libdeflate_amd import api
    tar, gz = tf.targz()
    assert len(gz) > 16384 and 900_000 < len(tar) < 1_300_000
    with tarfile.open(fileobj=io.BytesIO(gz), mode="r:gz") as t:
        want = [(ti.name, t.extractfile(ti).read()) for ti in t.getmembers()]
    d_gz = torch.frombuffer(bytearray(gz), dtype=torch.uint8).cuda()
    d_tar = torch.full((len(tar) + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    tz = dec.read_targz(d_gz, d_tar, 256, spacing=65536, max_points=64, out_avail=len(tar))
    assert tz.result == 0 and tz.nbytes == len(tar)
    assert d_tar.cpu().numpy().tobytes() == tar + bytes([CANARY]) * GUARD
    model = tar_walk.read(tar, 256, extract=False)
    assert tz.words == model.words and tz.rows.tolist() == model.rows
    assert tz.results.tolist() == model.results and len(tz.seek_index) > 4
    assert api.tar_entry_names(d_tar, tz.words, tz.rows) == [n for n, _ in want]
    m = len(want)
    sel = [0, m // 2, m - 1]
    need = sum(len(want[k][1]) for k in sel)
    for how in ("gz", "tar"):
        out = torch.full((need + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        per = torch.full((3,), UNSET, dtype=torch.int32, device="cuda")
        if how == "gz":
            offs = dec.read_targz_entries(d_gz, tz, sel, out, per, out_avail=need)
        else:
            offs = dec.read_tar_batch(d_tar, tz.rows, sel, out, per, in_nbytes=len(tar),
                                      out_avail=need)
        torch.cuda.synchronize()
        host = out.cpu().numpy().tobytes()
        assert per.cpu().tolist() == [0, 0, 0] and int(offs[-1]) == need, how
        assert host == b"".join(want[k][1] for k in sel) + bytes([CANARY]) * GUARD, how
        assert [int(x) for x in offs[:3]] == [0, len(want[0][1]),
                                             len(want[0][1]) + len(want[m // 2][1])]


def test_calls_only_enqueue(torch, dec):
    """after a call with the same shapes has grown the scratch, the extract
    and the selection return while the stream is still busy with a kernel
    queued in front of them: they do not synchronise"""
    g = tf.tiles()
    m = _records(g)
    model = tar_walk.read(g.data, m, out_align=16)
    total = model.words[3]
    d_in = _up(torch, g.data)
    st = torch.cuda.current_stream()

    def run(pre):
        out = torch.full((total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        sub = torch.full((total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        idx = torch.full((8 * m,), -1, dtype=torch.int64, device="cuda")
        per = torch.full((m,), UNSET, dtype=torch.int32, device="cuda")
        per2 = torch.full((m,), UNSET, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        if pre:
            torch.cuda._sleep(200_000_000)
        dec.extract_tar_batch(d_in, m, out, res, per, index=idx, out_align=16, stream=st,
                              in_nbytes=len(g.data), out_avail=total)
        dec.read_tar_batch(d_in, model.rows, list(range(m)), sub, per2, out_align=16, stream=st,
                           in_nbytes=len(g.data), out_avail=total)
        busy = not st.query()
        torch.cuda.synchronize()
        assert [int(x) for x in res.cpu().tolist()] == model.words
        want = _image(model.rows, model.plain, total + GUARD)
        assert np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(sub.cpu().numpy(), want)
        return busy
    run(False)                  # the scratch and the pinned block exist now
    assert run(True), "the stream had drained when the calls returned"
