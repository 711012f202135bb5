"""ZIP archives with huge entries read on the GPU
(libdeflate_amd_zip_read_large).  No tolerance anywhere: on every existing
archive and defect file the call equals libdeflate_amd_zip_read_batch - offsets,
results, every output byte - and the CPU model (tools/models/zip_walk.py); on
an archive with entries of 1 to 4 MiB every entry's bytes equal zipfile's;
damage in a large entry fails that entry alone; and nothing is written where
nothing may be (canary bytes behind out_avail and in the alignment gaps)."""
import numpy as np
import pytest

from tests import zip_files as zf
from tests import zip_large_files as zl
from tools.models import zip_walk

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE = 0, 1, 2, 3
UNSUPPORTED = 18
CANARY = 0xA5
UNSET = -7      # d_results where nothing was written
BEHIND = b"PK\5\6" + b"\0" * 18     # behind in_nbytes: not part of the file
NEVER = 1 << 40     # a large_min no entry reaches
CAP = 64        # entries per selection (tests/test_zip_large_abi.py: why that loses nothing)
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


def _index(torch, dec, d_in, n, max_entries):
    """-> (entries, index rows as the device states them)"""
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * max_entries,), -1, dtype=torch.int64, device="cuda")
    per = torch.full((max_entries,), UNSET, dtype=torch.int32, device="cuda")
    dec.index_zip_batch(d_in, max_entries, res, per, index=idx, in_nbytes=n)
    torch.cuda.synchronize()
    words = res.cpu().tolist()
    m = int(words[1]) if words[0] == SUCCESS or per.cpu()[0] != UNSET else 0
    return m, idx.cpu().numpy().reshape(-1, 8)[:m].astype(np.uint64)


def _offsets(rows, sel, align):
    """where the selections lie: the prefix sum of the sizes rounded up to the
    alignment, a row refused before the decode taking no room"""
    offs, at = [], 0
    for k in sel:
        row = [int(x) for x in rows[k]]
        method, flags = row[2] & 0xFFFF, row[2] >> 16
        offs.append(at)
        if not (flags & 0x2061) and method in (0, 8) and (method == 8 or row[5] == row[6]):
            at += -(-row[6] // align) * align
    return offs + [at]


def _read(torch, dec, call, d_in, n, rows, sel, align, **kw):
    """one call into exactly the room the selection needs -> (offsets,
    results, the output and 64 bytes behind it as numpy: 0xA5 where nothing
    was written)"""
    avail = _offsets(rows, sel, align)[-1]
    out = torch.full((avail + 64,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((max(len(sel), 1),), UNSET, dtype=torch.int32, device="cuda")
    offs = getattr(dec, call)(d_in, rows, sel, out, per, out_align=align, in_nbytes=n,
                              out_avail=avail, **kw)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert not (host[avail:] != CANARY).any(), "bytes written at or past out_avail"
    assert offs.tolist() == _offsets(rows, sel, align)
    return offs.tolist(), per.cpu().numpy()[:len(sel)].tolist(), host


def _same_as_the_batch_call(torch, dec, data, rows, sel, large_min, refused=None):
    d_in = _up(torch, data)
    for align in (1, 256):
        if refused is not None and refused in sel:
            # a row that cannot be one of this file: refused alike, before any
            # work, and the other entries read alike without it
            with pytest.raises(RuntimeError, match=f"status -2.*row {refused}:") as e1:
                _read(torch, dec, "read_zip_batch", d_in, len(data), rows, sel, align)
            with pytest.raises(RuntimeError) as e2:
                _read(torch, dec, "read_zip_large", d_in, len(data), rows, sel, align,
                      large_min=large_min)
            assert str(e2.value) == str(e1.value).replace("zip_read_batch", "zip_read_large")
            sel = [k for k in sel if k != refused]
        ref = _read(torch, dec, "read_zip_batch", d_in, len(data), rows, sel, align)
        got = _read(torch, dec, "read_zip_large", d_in, len(data), rows, sel, align,
                    large_min=large_min)
        assert got[0] == ref[0] and got[1] == ref[1], (align, got[1], ref[1])
        assert np.array_equal(got[2], ref[2]), align
        # ... and both as the CPU model has them
        offs, res, plain = zip_walk.read_selection(data, rows, sel, out_align=align)
        assert got[0] == offs and got[1] == res
        for r, b in enumerate(plain):
            if res[r] == SUCCESS:
                assert got[2][offs[r]:offs[r] + len(b)].tobytes() == b, (align, r)


@pytest.mark.parametrize("large_min", (1, NEVER))
@pytest.mark.parametrize("name", zf.GOOD_NAMES)
def test_good_files_read_as_the_batch_call_reads_them(torch, dec, name, large_min):
    """every existing archive, its first 64 entries: with large_min 1 every
    deflated entry with a byte of data goes through
    libdeflate_amd_decompress_large, with 2^40 none does"""
    g = zf.good(name)
    want = len(zf.expected(g)[0])
    m, rows = _index(torch, dec, _up(torch, g.data), len(g.data), max(want, 1))
    assert m == want
    _same_as_the_batch_call(torch, dec, g.data, rows, list(range(min(m, CAP))), large_min)


@pytest.mark.parametrize("large_min", (1, NEVER))
@pytest.mark.parametrize("name", list(DEFECTS))
def test_defect_files_read_as_the_batch_call_reads_them(torch, dec, name, large_min):
    """one defect per file, through the rows the index call states for it; an
    archive that is refused as a whole has no rows, so its base file's are
    used on its bytes"""
    d = DEFECTS[name]
    want = len(zf.expected(d.base)[0])
    m, rows = _index(torch, dec, _up(torch, d.data), len(d.data), want + 1)
    if d.entry is None:
        assert m == 0
        m, rows = _index(torch, dec, _up(torch, d.base.data), len(d.base.data), want)
    assert m == want and (d.entry is None or d.entry < CAP)
    # (its ZIP64 extra is too short to tell csize: the row keeps 0xFFFFFFFF)
    refused = d.entry if name == "zip64_extra_short" else None
    _same_as_the_batch_call(torch, dec, d.data, rows, list(range(min(m, CAP))), large_min,
                            refused)


# ---- the archive with large entries ----

@pytest.fixture(scope="module")
def big(torch, dec):
    a = zl.archive()
    d_in = _up(torch, a.data)
    m, rows = _index(torch, dec, d_in, len(a.data), len(zl.NAMES))
    assert m == len(zl.NAMES) and rows.tolist() == zl.rows_of(a)
    return a, d_in, rows


def _image(offs, sel, datas, size):
    want = np.full(size, CANARY, dtype=np.uint8)
    for at, k in zip(offs, sel):
        want[at:at + len(datas[k])] = np.frombuffer(datas[k], dtype=np.uint8)
    return want


M = len(zl.NAMES)
SELECTIONS = {
    "directory order": list(range(M)),
    "reversed": list(range(M))[::-1],
    "the 3 MiB entry twice": [zl.entry("text3m"), zl.entry("small0"), zl.entry("text3m"),
                              zl.entry("stored2m+1")],
    "small only": list(zl.SMALL),
    "large only": list(zl.LARGE),
}


@pytest.mark.parametrize("large_min", (20000, NEVER))
@pytest.mark.parametrize("which", list(SELECTIONS))
def test_large_archive_reads_as_zipfile_reads_it(torch, dec, big, which, large_min):
    """entries of 3 MiB + 17, exactly one piece, one piece + 1, stored blocks
    inside DEFLATE, 4 MiB from a few KiB, stored 2 MiB + 1 and 2 MiB, nothing,
    and small ones in between: every byte, and 0xA5 everywhere else"""
    a, d_in, rows = big
    sel = SELECTIONS[which]
    for align in (1, 256):
        offs, res, host = _read(torch, dec, "read_zip_large", d_in, len(a.data), rows, sel, align,
                                large_min=large_min)
        assert res == [SUCCESS] * len(sel)
        assert np.array_equal(host, _image(offs, sel, a.datas, len(host))), align


def test_the_many_wave_decoder_answers_for_a_large_entry(torch, dec, big):
    from libdeflate_amd import binding
    a, d_in, rows = big
    sel = [zl.entry("text3m")]
    before = binding.stream_stats()
    _, res, host = _read(torch, dec, "read_zip_large", d_in, len(a.data), rows, sel, 1,
                         large_min=NEVER)
    assert res == [SUCCESS] and binding.stream_stats() == before
    _, res, host = _read(torch, dec, "read_zip_large", d_in, len(a.data), rows, sel, 1,
                         large_min=65536)
    after = binding.stream_stats()
    assert res == [SUCCESS] and host[:-64].tobytes() == a.datas[sel[0]]
    assert after["parallel"] == 1 and after["chunks_decoded"] > 1 and after != before
    _read(torch, dec, "read_zip_large", d_in, len(a.data), rows, sel, 1, large_min=NEVER)
    assert binding.stream_stats() == after
    # large_min 0 is the library's default, which a 1 MiB entry of text at
    # level 1 (some 400 KiB of DEFLATE) reaches and a 20 000-byte entry does not
    sel = [zl.entry("small3"), zl.entry("text1m")]
    assert int(rows[sel[1]][5]) > 256 * 1024 and int(rows[sel[0]][5]) < 20000
    _, res, host = _read(torch, dec, "read_zip_large", d_in, len(a.data), rows, sel[:1], 1,
                         large_min=0)
    assert res == [SUCCESS] and binding.stream_stats() == after
    _, res, host = _read(torch, dec, "read_zip_large", d_in, len(a.data), rows, sel, 1,
                         large_min=0)
    last = binding.stream_stats()
    assert res == [SUCCESS] * 2 and last != after and last["parallel"] == 1


def _flip(data, at):
    b = bytearray(data)
    b[at] ^= 0x55
    return bytes(b)


def _damage(case, a, rows):
    """-> (file, rows, the damaged entry)"""
    rows = rows.copy()
    name, what = case
    k = zl.entry(name)
    data_off, csize = int(rows[k][4]), int(rows[k][5])
    if what == "byte in the middle":
        return _flip(a.data, data_off + csize // 2), rows, k
    if what == "last byte":
        return _flip(a.data, data_off + csize - 1), rows, k
    if what == "crc^1":
        rows[k][3] ^= 1
    elif what == "usize+1":
        rows[k][6] += 1
    elif what == "usize-1":
        rows[k][6] -= 1
    elif what == "csize+1":
        assert data_off + csize + 1 <= len(a.data)
        rows[k][5] += 1
    return a.data, rows, k


DAMAGE = (("text3m", "byte in the middle"), ("stored2m+1", "last byte"), ("zeros", "crc^1"),
          ("text3m", "usize+1"), ("text3m", "usize-1"), ("zeros", "usize+1"),
          ("zeros", "usize-1"), ("stored2m+1", "usize+1"), ("stored2m+1", "usize-1"),
          ("text3m", "csize+1"), ("text1m", "csize+1"))


@pytest.mark.parametrize("case", DAMAGE, ids=lambda c: f"{c[0]} {c[1]}")
def test_damage_in_a_large_entry_fails_it_alone(torch, dec, big, case):
    """bad data behind result codes, never a fault: the entry's result is the
    batch call's for the same rows and file, every neighbour's bytes are
    intact, and the canary behind out_avail stands (_read)"""
    a, d_in, rows = big
    data, drows, k = _damage(case, a, rows)
    d_bad = d_in if data is a.data else _up(torch, data)
    sel = list(range(M))
    _, ref, _ = _read(torch, dec, "read_zip_batch", d_bad, len(data), drows, sel, 1)
    assert ref[k] != SUCCESS and not any(ref[:k] + ref[k + 1:])
    for large_min in (20000, NEVER):
        offs, res, host = _read(torch, dec, "read_zip_large", d_bad, len(data), drows, sel, 1,
                                large_min=large_min)
        assert res == ref, (large_min, res, ref)
        for r in sel:
            if r != k:
                got = host[offs[r]:offs[r] + len(a.datas[r])].tobytes()
                assert got == a.datas[r], (large_min, zl.NAMES[r])
