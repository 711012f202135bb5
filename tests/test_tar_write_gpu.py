"""tar archives written on the GPU (libdeflate_amd_tar_write_batch,
libdeflate_amd_targz_compress_batch).  No tolerance anywhere: the archive is
byte for byte what Python's tarfile writes for the same entries, every byte
below the size is written and none at or past it, the host index rows are the
rows the project's own reader finds, and the .tar.gz is what
compress_large_batch gives for tarfile's bytes."""
import gzip
import zlib

import numpy as np
import pytest

from tests import tar_write_cases as tw

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 4096
SIZES = [0, 1, 15, 16, 17, 511, 512, 513, 4096, 65024, 65535, 65536, 65537, 200000]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def comp():
    from libdeflate_amd import api
    c = api.Compressor(6)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dec():
    from libdeflate_amd import api
    d = api.Decompressor()
    yield d
    d.close()


def _odd_layout(datas):
    """the entries in one buffer, every one at an odd offset with other bytes
    around it -> (buffer, offsets)"""
    buf, offs = bytearray(b"#"), []
    for d in datas:
        if len(buf) % 2 == 0:
            buf += b"#"
        offs.append(len(buf))
        buf += d + b"##"
    return bytes(buf), offs


def _write(torch, comp, names, datas, out_shift=1, layout=None, mtime=tw.MTIME, stream=None):
    """-> (the archive's bytes from the device, the host index rows); d_out is
    pre-filled with 0xA5, begins out_shift bytes into its allocation and has
    4096 bytes behind the archive's size that must stay"""
    buf, offs = layout if layout is not None else _odd_layout(datas)
    sizes = [len(d) for d in datas]
    size = comp.tar_write_size(names, sizes)
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    whole = torch.full((out_shift + size + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    out = whole[out_shift:]
    rows = comp.write_tar_batch(names, d_in, offs, sizes, out, mtime=mtime, out_avail=size,
                                stream=stream)
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert not (host[:out_shift] != CANARY).any(), "bytes written in front of d_out"
    assert not (host[out_shift + size:] != CANARY).any(), "bytes written at or past the size"
    return host[out_shift:out_shift + size].tobytes(), rows


def _same(got, want):
    assert len(got) == len(want)
    if got != want:
        a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"{int((a != b).sum())} bytes differ, the first at {at} "
                             f"(block {at // 512}, byte {at % 512}): "
                             f"{got[at:at + 16]!r} for {want[at:at + 16]!r}")


def _check(torch, comp, names, datas, **kw):
    got, rows = _write(torch, comp, names, datas, **kw)
    _same(got, tw.tarfile_bytes(names, datas, kw.get("mtime", tw.MTIME)))
    return got, rows


@pytest.mark.parametrize("out_shift", [1, 16])
def test_bytes_equal_tarfiles(torch, comp, out_shift):
    """every entry size at a block, tile or 16-byte edge, sources at odd
    offsets, d_out one byte and sixteen bytes into its allocation"""
    names = [f"dir/file{k:02d}.txt" for k in range(len(SIZES))]
    datas = [tw.payload(k, s) for k, s in enumerate(SIZES)]
    _check(torch, comp, names, datas, out_shift=out_shift)
    # and the largest and the smallest first, so every size meets other offsets
    order = [13, 0, 9, 1, 12, 2, 11, 3, 10, 4, 8, 5, 7, 6]
    _check(torch, comp, [names[k] for k in order], [datas[k] for k in order],
           out_shift=out_shift)


def test_names(torch, comp):
    """1, 99, 100 and 101 ASCII bytes; 100 bytes with one character that is
    not ASCII; more than 100 characters of 2 and 3 bytes; the pax record on
    each side of its decimal's steps; two blocks of pax data; 65 535 bytes"""
    names = tw.edge_names()
    datas = [tw.payload(k, (37 * k) % 1500) for k in range(len(names))]
    got, rows = _check(torch, comp, names, datas)
    # header names where tarfile keeps them in the header, pax values elsewhere
    src = [int(r[3]) >> 8 for r in rows]
    assert src[:3] == [0, 0, 0] and set(src[3:]) == {2}
    for name, r in zip(names, rows):
        raw = name.encode("utf-8")
        assert got[int(r[1]):int(r[1]) + int(r[2])] == raw


def test_tile_edges(torch, comp):
    """more than 64 headers in one tile; data that begins in the last block of
    a tile; a header that is the first block of a tile; a 65 535-byte name
    whose pax data crosses a tile boundary; a pax header that ends a tile"""
    names = [f"e{k}" for k in range(300)]
    got, _ = _check(torch, comp, names, [b""] * 300)
    assert len(got) == 10240 * 15 + 10240 and 300 * 512 > 2 * tw.TILE
    # header 0, 125 blocks: the next header is block 126, its data begins in
    # block 127 and runs into the next tile; then up to block 256 exactly, so
    # the header behind it is the first block of the third tile
    first = 125 * 512
    second = 512 + 700
    third = (256 - 126 - 1 - 3 - 1) * 512   # (entry 1 is 1 + 3 blocks)
    datas = [tw.payload(0, first), tw.payload(1, second), tw.payload(2, third - 5),
             tw.payload(3, 3000)]
    got, rows = _check(torch, comp, ["a", "b", "c", "d"], datas)
    assert int(rows[1][4]) == 127 * 512 and int(rows[3][0]) == 2 * tw.TILE
    # the long name's pax header at block 119, its data in blocks 120 .. 248
    long_name = "n" * 65535
    got, rows = _check(torch, comp, ["lead", long_name, "tail"],
                       [tw.payload(4, 118 * 512), tw.payload(5, 100), b"x"])
    assert int(rows[1][1]) // tw.TILE == 0 and int(rows[1][0]) // tw.TILE == 1
    # a pax header as the last block of a tile, its data at the next one's start
    got, rows = _check(torch, comp, ["lead", "é" * 70], [tw.payload(6, 126 * 512), b"yz"])
    assert int(rows[1][1]) // 512 == 128


def test_ends(torch, comp):
    """no entries; entries that end at a multiple of 10 240 minus 1024 (the
    end blocks just fit), minus 512 and minus 0 (they spill)"""
    got, rows = _check(torch, comp, [], [])
    assert got == bytes(10240) and rows.shape == (0, 8)
    for data, want in ((10240 - 512 - 1024, 10240), (10240 - 512 - 512, 20480),
                       (10240 - 512, 20480), (6 * 10240 + 10240 - 512 - 1024, 7 * 10240),
                       (6 * 10240 + 10240 - 512, 8 * 10240)):
        got, _ = _check(torch, comp, ["end"], [tw.payload(7, data)])
        assert len(got) == want


def test_overlapping_entries(torch, comp):
    """the same range twice, nested ranges, ranges that share an edge"""
    buf = tw.payload(8, 5000)
    ranges = [(100, 3000), (100, 3000), (0, 5000), (101, 2998), (1500, 1), (3100, 1900), (4999, 1)]
    names = [f"r{k}" for k in range(len(ranges))]
    datas = [buf[o:o + n] for o, n in ranges]
    _check(torch, comp, names, datas, layout=(buf, [o for o, _ in ranges]))


def test_round_trip_through_the_reader(torch, comp, dec):
    """tar_index_batch finds the writer's host rows word for word, with EOF
    and HAS_PAX; tar_extract_batch gives the entries back; tar_read_batch
    takes the writer's rows as they are"""
    from libdeflate_amd import api, binding
    names = ["plain", "é" * 60, "x" * 150, "dir/" + "y" * 90, "empty", "z" * 100]
    datas = [tw.payload(20 + k, s) for k, s in enumerate((70000, 513, 1, 4096, 0, 65536))]
    buf, offs = _odd_layout(datas)
    sizes = [len(d) for d in datas]
    size = comp.tar_write_size(names, sizes)
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    arc = torch.full((size + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    rows = comp.write_tar_batch(names, d_in, offs, sizes, arc, out_avail=size)
    m = 2 * len(names)
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * m,), -1, dtype=torch.int64, device="cuda")
    per = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    total = sum(sizes)
    out = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
    dec.extract_tar_batch(arc, m, out, res, per, index=idx, in_nbytes=size, out_avail=total)
    torch.cuda.synchronize()
    words = [int(x) for x in res.cpu().tolist()]
    end = int(rows[-1][4]) + -(-sizes[-1] // 512) * 512
    assert words == [0, len(names), end, total, binding.TAR_EOF | binding.TAR_HAS_PAX]
    found = idx.cpu().numpy().astype(np.uint64).reshape(-1, 8)
    assert found[:len(names)].tolist() == rows.tolist()
    assert per.cpu().numpy()[:len(names)].tolist() == [0] * len(names)
    host = out.cpu().numpy()
    assert host[:total].tobytes() == b"".join(datas) and (host[total:] == CANARY).all()
    assert api.tar_entry_names(arc, res, idx) == names
    # a shuffled selection with duplicates, through the writer's rows
    sel = [3, 0, 5, 1, 3, 4, 2]
    need = sum(sizes[k] for k in sel)
    out2 = torch.full((need + 64,), CANARY, dtype=torch.uint8, device="cuda")
    per2 = torch.full((len(sel),), -7, dtype=torch.int32, device="cuda")
    at = dec.read_tar_batch(arc, rows, sel, out2, per2, in_nbytes=size, out_avail=need)
    torch.cuda.synchronize()
    host = out2.cpu().numpy()
    assert host[:need].tobytes() == b"".join(datas[k] for k in sel)
    assert (host[need:] == CANARY).all() and per2.cpu().tolist() == [0] * len(sel)
    assert at.tolist() == np.concatenate(([0], np.cumsum([sizes[k] for k in sel]))).tolist()
    rng, rtotal = api.tar_ranges(rows, sel)
    assert rtotal == need and rng[:, 0].tolist() == [int(rows[k][4]) for k in sel]


@pytest.mark.parametrize("fmt", ["gzip", "zlib"])
@pytest.mark.parametrize("level", [1, 6])
def test_targz(torch, fmt, level):
    """d_out[:d_out_nbytes[0]] is compress_large_batch of tarfile's bytes - an
    archive above 128 KiB, where the segmented path runs, and a small one -,
    it decompresses to them, and one byte short leaves 0 and the bytes behind
    out_avail alone"""
    from libdeflate_amd import api
    c = api.Compressor(level)
    cases = [(["big/" + "é" * 40, "second", "t" * 120],
              [tw.payload(30, 150000), tw.payload(31, 70001), tw.payload(32, 5)]),
             (["small"], [tw.payload(33, 3000)])]
    for names, datas in cases:
        ref = tw.tarfile_bytes(names, datas)
        buf, offs = _odd_layout(datas)
        sizes = [len(d) for d in datas]
        assert c.tar_write_size(names, sizes) == len(ref)
        bound = c.bound(fmt, len(ref))
        d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        d_ref = torch.frombuffer(bytearray(ref), dtype=torch.uint8).cuda()
        want_buf = torch.full((bound + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        want_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        c.compress_large_batch(fmt, d_ref, want_buf, want_n, out_avail=bound)
        out = torch.full((1 + bound + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        out_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        rows = c.compress_targz_batch(fmt, names, d_in, offs, sizes, out[1:], out_n,
                                      mtime=tw.MTIME, out_avail=bound)
        torch.cuda.synchronize()
        n = int(out_n.item())
        assert n == int(want_n.item()) and 0 < n <= bound
        got = out.cpu().numpy()
        assert got[0] == CANARY and (got[1 + bound:] == CANARY).all()
        stream = got[1:1 + n].tobytes()
        assert stream == want_buf.cpu().numpy()[:n].tobytes()
        plain = gzip.decompress(stream) if fmt == "gzip" else zlib.decompress(stream)
        assert plain == ref
        # the rows are the archive's
        assert rows.tolist() == c.write_tar_batch(
            names, d_in, offs, sizes,
            torch.empty(len(ref), dtype=torch.uint8, device="cuda"), mtime=tw.MTIME).tolist()
        # one byte short
        out.fill_(CANARY)
        out_n.fill_(-1)
        c.compress_targz_batch(fmt, names, d_in, offs, sizes, out[1:], out_n, mtime=tw.MTIME,
                               out_avail=n - 1)
        torch.cuda.synchronize()
        assert int(out_n.item()) == 0
        got = out.cpu().numpy()
        assert got[0] == CANARY and (got[1 + n - 1:] == CANARY).all()
    c.close()


def test_stream_and_object_contract(torch, comp):
    """two calls back to back on one object and a stream that is not the
    default one, the host arrays overwritten between and after them: both
    archives come out right"""
    s = torch.cuda.Stream()
    sets = [(["one", "é" * 101], [tw.payload(40, 70000), tw.payload(41, 33)]),
            (["two/" + "w" * 200, "three"], [tw.payload(42, 513), tw.payload(43, 140000)])]
    outs, keep = [], []
    for names, datas in sets:
        buf, offs = _odd_layout(datas)
        blob, noffs, ino, inn = tw.call_arrays(names, [len(d) for d in datas], offs)
        size = comp.tar_write_size((blob, noffs), inn)
        with torch.cuda.stream(s):
            d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
            out = torch.full((size + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        blob, noffs = blob.copy(), noffs.copy()
        comp.write_tar_batch((blob, noffs), d_in, ino, inn, out, mtime=tw.MTIME, out_avail=size,
                             stream=s, index=False)
        # the call has returned: its host arrays are the caller's again
        blob[:] = 0x2F
        noffs[:] = 0
        ino[:] = 1 << 40
        inn[:] = 1 << 40
        outs.append((out, size))
        keep.append(d_in)
    s.synchronize()
    for (out, size), (names, datas) in zip(outs, sets):
        host = out.cpu().numpy()
        _same(host[:size].tobytes(), tw.tarfile_bytes(names, datas))
        assert (host[size:] == CANARY).all()
