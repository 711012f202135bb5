"""ZIP archives written on the GPU (libdeflate_amd_zip_compress_batch).  No
tolerance anywhere: the archive equals, byte for byte, what the CPU model
(tools/models/zip_write.py) builds from the streams the same compressor object
returns for every entry alone; result words and index rows equal the model's;
zipfile and the project's own reader read every entry back; and nothing is
written where nothing may be."""
import io
import zipfile
import zlib

import numpy as np
import pytest

from tests import datagen
from tools.models import zip_write

pytestmark = pytest.mark.gpu

SUCCESS, INSUFFICIENT_SPACE = 0, 3
STORE, FORCE_ZIP64 = 1, 2
CANARY = 0xA5
DATETIME = (2024 - 1980) << 25 | 2 << 21 | 29 << 16 | 13 << 11 | 7 << 5 | 9
TEXT_SIZES = (0, 1, 2, 100, 4095, 4096, 4097, 65535, 65536, 65537, 131071, 131072, 131073, 300000)
NAME_LENS = (1, 2, 15, 16, 17, 255)


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


def _name(k, kind):
    """unique per entry; kind 6 is the UTF-8 name"""
    if kind == 6:
        return ("déjà vu/漢字 %d.txt" % k).encode("utf-8")
    return (chr(97 + k) + "%d/" % k + "n" * 255)[:NAME_LENS[kind]].encode("ascii")


@pytest.fixture(scope="module")
def case(torch):
    """the entries, their names, and one device buffer that holds them at
    offsets of their own, with gaps between them"""
    text = datagen.text_chunk(sum(TEXT_SIZES), 0x21D)
    entries, at = [], 0
    for n in TEXT_SIZES:
        entries.append(text[at:at + n])
        at += n
    # random bytes do not compress: stored, the second as segments that fit
    # their slots while their sum does not win; zeros compress to almost nothing
    entries += [datagen.random_chunk(1000, 1), datagen.random_chunk(200000, 2), bytes(70000)]
    names = [_name(k, k % 7) for k in range(len(entries))]
    assert len(set(names)) == len(names)
    # gaps between the entries, chosen so that in the stored archive entry k's
    # destination lies k bytes mod 16 behind its source: every disagreement
    # mod 16 between the two
    buf, offs, dst, shifts = bytearray(b"\xEE" * 5), [], 0, set()
    for k, (nm, e) in enumerate(zip(names, entries)):
        buf += b"\xEE" * (1 + (dst + 30 + len(nm) - k - len(buf) - 1) % 16)
        offs.append(len(buf))
        shifts.add((dst + 30 + len(nm) - len(buf)) % 16)
        buf += e
        dst += 30 + len(nm) + len(e)
    buf += b"\xEE" * 7
    assert len(shifts) == 16
    d_in = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    return names, entries, offs, [len(e) for e in entries], d_in


_COMPRESSORS, _STREAMS = {}, {}


def _comp(level):
    from libdeflate_amd import api
    if level not in _COMPRESSORS:
        _COMPRESSORS[level] = api.Compressor(level)
    return _COMPRESSORS[level]


def _streams(level, entries):
    """what the object's single-buffer call returns for every entry alone:
    computed once per level, shared by the cases"""
    if level not in _STREAMS:
        c = _comp(level)
        _STREAMS[level] = [c.compress("deflate", e) if e else None for e in entries]
    return _STREAMS[level]


def _write(torch, comp, names, d_in, offs, sizes, out_avail, flags=0, dt=0):
    """-> (result words, d_out as numpy (out_avail + 64 bytes, 0xA5 where
    nothing was written), index rows (-1 where nothing was written))"""
    out = torch.full((out_avail + 64,), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * max(len(names), 1),), -1, dtype=torch.int64, device="cuda")
    comp.compress_zip_batch(names, d_in, offs, sizes, out, res, index=idx, dos_datetime=dt,
                            flags=flags, out_avail=out_avail)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert not (host[out_avail:] != CANARY).any(), "bytes written past out_avail"
    return [int(x) for x in res.cpu().tolist()], host, idx.cpu().numpy().reshape(-1, 8)


def _read_back(torch, dec, archive, n, total):
    """the project's reader on the archive -> (index words, index rows,
    decompress words, per-entry results, output)"""
    d_arc = torch.frombuffer(bytearray(archive), dtype=torch.uint8).cuda()
    m = max(n, 1)
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * m,), -1, dtype=torch.int64, device="cuda")
    per = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    dec.index_zip_batch(d_arc, m, res, per, index=idx)
    torch.cuda.synchronize()
    iwords, irows = [int(x) for x in res.cpu().tolist()], idx.cpu().numpy().reshape(-1, 8)
    out = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
    dec.decompress_zip_batch(d_arc, m, out, res, per, index=idx, out_avail=total)
    torch.cuda.synchronize()
    return (iwords, irows, [int(x) for x in res.cpu().tolist()], per.cpu().numpy()[:n],
            out.cpu().numpy())


def _check_archive(torch, dec, comp, names, entries, offs, sizes, d_in, streams, flags, dt,
                   once=False):
    """once: one write into exactly enough room (the large archives)"""
    n = len(names)
    model = zip_write.build(names, entries, streams, dt, flags)
    size = model.words[1]
    bound = comp.zip_bound(names, sizes, flags)
    assert size <= bound == zip_write.bound([len(x) for x in names], sizes, flags)[0]
    # room to spare, and exactly enough: the same bytes, nothing behind them
    words, host, rows = _write(torch, comp, names, d_in, offs, sizes, size if once else bound,
                               flags, dt)
    assert words == model.words
    assert bytes(host[:size]) == model.data
    assert not (host[size:] != CANARY).any(), "bytes written behind the archive"
    assert rows[:n].tolist() == model.rows
    if once:
        return _read_archive_back(torch, dec, model, names, entries, sizes, words, rows)
    words2, host2, rows2 = _write(torch, comp, names, d_in, offs, sizes, size, flags, dt)
    assert words2 == words and np.array_equal(rows2, rows)       # (a repeat: identical bytes)
    assert np.array_equal(host2[:size], host[:size]) and not (host2[size:] != CANARY).any()
    # one byte short: INSUFFICIENT_SPACE, the size still told, nothing written at all
    if n == 0:      # (below the end records alone the call is refused)
        with pytest.raises(RuntimeError, match="out_avail"):
            _write(torch, comp, names, d_in, offs, sizes, size - 1, flags, dt)
    else:
        words3, host3, rows3 = _write(torch, comp, names, d_in, offs, sizes, size - 1, flags, dt)
        assert words3 == [INSUFFICIENT_SPACE] + model.words[1:]
        assert not (host3 != CANARY).any() and (rows3 == -1).all()
    return _read_archive_back(torch, dec, model, names, entries, sizes, words, rows)


def _read_archive_back(torch, dec, model, names, entries, sizes, words, rows):
    n = len(names)
    # zipfile reads every entry back
    zfile = zipfile.ZipFile(io.BytesIO(model.data))
    infos = zfile.infolist()
    assert [zi.orig_filename.encode("utf-8" if zi.flag_bits & 0x800 else "cp437")
            for zi in infos] == list(names)
    for zi, raw, row in zip(infos, entries, model.rows):
        assert (zi.CRC, zi.file_size, zi.compress_size) == (zlib.crc32(raw), len(raw), row[5])
        assert zfile.open(zi).read() == raw
    # ... and so does the project's reader, whose index is d_index
    total = sum(sizes)
    iwords, irows, dwords, per, out = _read_back(torch, dec, model.data, n, total)
    assert iwords == dwords == [SUCCESS, n, words[2], total, 1 if model.zip64 else 0]
    assert np.array_equal(irows[:n], rows[:n])
    assert not per.any()
    assert bytes(out[:total]) == b"".join(entries) and not (out[total:] != CANARY).any()
    return model


@pytest.mark.parametrize("flags", (0, STORE, FORCE_ZIP64, STORE | FORCE_ZIP64))
@pytest.mark.parametrize("level", (0, 1, 6, 9, 12))
def test_archive_is_the_models(torch, dec, case, level, flags):
    """entries of 0 bytes to 300 000 - below, at and above the small-buffer
    kernel's 4 KiB, 64 KiB and the 128 KiB from which an entry is cut into
    segments -, incompressible ones whole and segmented, zeros; names of 1 to
    255 bytes and a UTF-8 one"""
    names, entries, offs, sizes, d_in = case
    comp = _comp(level)
    streams = _streams(level, entries)
    dt = DATETIME if flags & FORCE_ZIP64 else 0
    model = _check_archive(torch, dec, comp, names, entries, offs, sizes, d_in, streams, flags, dt)
    methods = [row[2] & 0xFFFF for row in model.rows]
    if level == 0 or flags & STORE:
        assert model.words[3] == 0 and not any(methods)
    else:
        # every text entry that can win does; random bytes and the empty entry are stored
        assert methods[TEXT_SIZES.index(4095):len(TEXT_SIZES)] == [8] * (len(TEXT_SIZES) - 4)
        assert methods[0] == 0 and methods[-3:] == [0, 0, 8]
        # the segmented random entry's pieces all fitted their slots: it is
        # stored because the sum does not win
        assert len(streams[-2]) >= len(entries[-2])
    assert model.zip64 == bool(flags & FORCE_ZIP64)
    # the same object, its scratch grown by the archive above, on a small one
    small = [1, 4, len(entries) - 1]
    _check_archive(torch, dec, comp, [names[k] for k in small], [entries[k] for k in small],
                   [offs[k] for k in small], [sizes[k] for k in small], d_in,
                   [streams[k] for k in small], flags, 0)


def test_empty_archive_and_empty_entries(torch, dec):
    comp = _comp(6)
    d_in = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for flags in (0, FORCE_ZIP64):
        _check_archive(torch, dec, comp, [], [], [], [], d_in, [], flags, 0)
        _check_archive(torch, dec, comp, [b"a", b"bb"], [b"", b""], [16, 0], [0, 0], d_in,
                       [None, None], flags, 0)
    # d_in NULL with in_avail 0
    words, host, _ = _write(torch, comp, [b"a"], d_in[:0], [0], [0], 200)
    assert words == [SUCCESS, 30 + 1 + 46 + 1 + 22, 31, 0]
    assert bytes(host[:words[1]]) == zip_write.build([b"a"], [b""], [None]).data


def test_65600_small_entries_are_zip64_by_their_count(torch, dec):
    """ZIP64 from the count alone; zipfile and the project's reader agree"""
    n = 65600
    comp = _comp(6)
    rng = np.random.default_rng(0x21E)
    lens = rng.integers(0, 17, n)
    noise = datagen.lowentropy_chunk(int(lens.sum()) + 16, 0x21F)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
    # every seventh entry is a run of zeros
    entries = [bytes(int(ln)) if k % 7 == 0 else noise[int(o):int(o) + int(ln)]
               for k, (o, ln) in enumerate(zip(offs, lens))]
    text = b"".join(entries) + b"\0"
    names = [b"d%d/%d" % (k % 100, k) for k in range(n)]
    d_in = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    streams = comp.compress_batch_host("deflate", entries)
    model = zip_write.build(names, entries, streams)
    assert model.zip64
    words, host, rows = _write(torch, comp, names, d_in, offs, lens, model.words[1])
    assert words == model.words
    assert bytes(host[:words[1]]) == model.data
    assert rows.tolist() == model.rows
    zfile = zipfile.ZipFile(io.BytesIO(model.data))
    infos = zfile.infolist()
    assert [zi.orig_filename.encode() for zi in infos] == names
    assert [(zi.CRC, zi.file_size) for zi in infos] == [(zlib.crc32(e), len(e)) for e in entries]
    for k in range(0, n, 41):
        assert zfile.open(infos[k]).read() == entries[k]
    total = int(lens.sum())
    iwords, irows, dwords, per, out = _read_back(torch, dec, model.data, n, total)
    assert iwords == dwords == [SUCCESS, n, words[2], total, 1]
    assert np.array_equal(irows, rows) and not per.any()
    assert bytes(out[:total]) == text[:total]


def _numbered(base, n):
    """n bytes of `base` repeated, every 4 KiB block stamped with its number:
    no two pieces alike, so a misplaced piece or a wrong CRC-32 shows"""
    arr = np.tile(np.frombuffer(base, dtype=np.uint8), -(-n // len(base)))[:n].copy()
    pos = np.arange(0, n - 4, 4096)
    for b in range(4):
        arr[pos + b] = (pos >> (12 + 8 * b)) & 0xFF
    return arr.tobytes()


@pytest.fixture(scope="module")
def large_case(torch):
    """entries of many pieces - more than 64 (a second round of the place
    kernel's wave scan, runs of several pieces per lane in the CRC-32
    combine) - in every segment size: 1.5 MiB (96 x 16 KiB), 5 MiB (160 x
    32 KiB), 9 MiB and 34 MiB (144 + 544 x 64 KiB: a group of more than
    32 MiB, two compress launches), 3 MiB of random bytes (192 pieces that
    fit their slots, stored) - with small and whole entries between them"""
    text = datagen.text_chunk(1 << 20, 0x220)
    mib = 1 << 20
    entries = [_numbered(text, 3 * mib // 2), text[:3000], _numbered(text[5:], 5 * mib),
               datagen.random_chunk(3 * mib, 3), _numbered(text[11:], 9 * mib), text[:70001],
               _numbered(text[17:], 34 * mib + 12345), b""]
    names = [b"big/%d.bin" % k for k in range(len(entries))]
    buf, offs = bytearray(b"\xEE" * 3), []
    for k, e in enumerate(entries):
        offs.append(len(buf))
        buf += e + b"\xEE" * (k + 1)
    d_in = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    return names, entries, offs, [len(e) for e in entries], d_in


@pytest.mark.parametrize("level,flags", ((6, 0), (1, 0), (1, STORE)))
def test_large_entries_of_every_segment_size(torch, dec, large_case, level, flags):
    """deflated at two levels and stored: the archive equals the model fed
    with the single-buffer call's stream per entry, and zipfile and the
    reader - which check every entry's CRC-32 - read every byte back"""
    names, entries, offs, sizes, d_in = large_case
    comp = _comp(level)
    streams = [None] * len(entries) if flags & STORE else \
        [comp.compress("deflate", e) if e else None for e in entries]
    model = _check_archive(torch, dec, comp, names, entries, offs, sizes, d_in, streams, flags, 0,
                           once=True)
    methods = [row[2] & 0xFFFF for row in model.rows]
    assert methods == ([0] * 8 if flags & STORE else [8, 8, 8, 0, 8, 8, 8, 0])
