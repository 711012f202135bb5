"""Adam7-interlaced PNG files decoded on the GPU (libdeflate_amd_png_index_batch_ex
and libdeflate_amd_png_decode_batch_ex).  No tolerance anywhere: every row word,
result and byte equals what the builder put in (tests/png_adam7_files.py), what
the CPU model states (tools/models/png_adam7.py, pinned against PIL by
tests/test_png_adam7_model.py) or what the older calls give for the
non-interlaced twin of the same image; and the sentinel bytes in front of d_out,
in every alignment gap and behind out_avail stay untouched.  The harness is
that of tests/test_png_gpu.py: files packed at unaligned offsets, the output in
exactly the room it needs.  Every test is one or a few batches of tiny files;
the shapes are the smallest at which a pass is absent, the unfilter starts a
second band inside a pass, a 16-byte piece or a tile of 1024 pieces ends."""
import random

import numpy as np
import pytest

from tests import png_adam7_files as p7
from tests import png_files as pf
from tests.test_png_gpu import CANARY, GUARD, UNSET, _index, _pack
from tools.models import png_adam7 as m7
from tools.models import png_model as pm
from tools.models import png_pixels_model as px

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE, UNSUPPORTED = 0, 1, 2, 3, 18
ADAM7, LE16 = m7.ADAM7, m7.LE16


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


def _index_ex(torch, dec, buf, offs, sizes, flags):
    """index_png_batch_ex -> (device input, host rows as lists, results), the
    words behind the last row and result untouched"""
    n = len(offs)
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_n = torch.tensor(sizes, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * n + 8,), -1, dtype=torch.int64, device="cuda")
    per = torch.full((n + 1,), UNSET, dtype=torch.int32, device="cuda")
    dec.index_png_batch_ex(d_in, d_off, d_n, idx, per, flags=flags)
    torch.cuda.synchronize()
    rows = idx.cpu().numpy().view(np.uint64).reshape(-1, 8)
    res = per.cpu().numpy()
    assert (rows[n] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and res[n] == UNSET
    return d_in, [[int(x) for x in r] for r in rows[:n]], res[:n].tolist()


def _call(torch, dec, d_in, rows, sel, fmt, align, flags, sizes_flags=ADAM7):
    """decode_png_batch_ex into exactly the room it needs, sentinels around it
    -> (results, the output bytes, offsets)"""
    from libdeflate_amd import api
    offs_want = m7.out_sizes(rows, sel, fmt, align)
    total = offs_want[-1]
    o2, t2 = api.png_out_sizes_ex(rows, sel, fmt, align, sizes_flags)
    assert o2.tolist() == offs_want and t2 == total
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    per = torch.full((len(sel) + 1,), UNSET, dtype=torch.int32, device="cuda")
    offs = dec.decode_png_batch_ex(d_in, rows, sel, whole[GUARD:], per, fmt, out_align=align,
                                   flags=flags, out_avail=total)
    torch.cuda.synchronize()
    assert offs.tolist() == offs_want
    host = whole.cpu().numpy()
    assert not (host[:GUARD] != CANARY).any(), "bytes written in front of d_out"
    assert not (host[GUARD + total:] != CANARY).any(), "bytes written past out_avail"
    res = per.cpu().numpy()
    assert res[len(sel)] == UNSET
    return res[:len(sel)].tolist(), host[GUARD:GUARD + total], offs_want


def _check(host, offs, sel, want):
    """want: per selection (result, bytes or None); the rooms' bytes, and the
    sentinel in every gap between them.  A failed selection's room is undefined."""
    expect = np.full(len(host), CANARY, dtype=np.uint8)
    defined = np.ones(len(host), dtype=bool)
    for r, (code, data, room) in enumerate(want):
        if data is not None:
            assert len(data) == room
            expect[offs[r]:offs[r] + room] = np.frombuffer(data, dtype=np.uint8)
        else:
            defined[offs[r]:offs[r] + room] = False
    bad = np.nonzero((host != expect) & defined)[0]
    assert bad.size == 0, "first wrong byte at %d of %d" % (bad[0], len(host))


_MODEL = {}


def _model(buf, row, flags, fmt):
    key = (buf[row[0]:row[0] + row[1]], tuple(row[2:]), row[0], flags & LE16, fmt)
    if key not in _MODEL:
        _MODEL[key] = m7.decode(buf, row, flags & LE16, fmt)
    return _MODEL[key]


def _room(row, fmt):
    if pm.is_zero(row):
        return 0
    return px.out_bytes(row, fmt) if fmt else (row[2] >> 32) * pm.row_rowbytes(row)


def _against_model(torch, dec, files, fmt=0, sel=None, align=1, flags=ADAM7, expect=None, seed=0):
    """index with the flag, decode, everything against the model"""
    buf, offs, sizes = _pack(files, seed)
    d_in, rows, res = _index_ex(torch, dec, buf, offs, sizes, ADAM7)
    want_idx = [m7.index(buf, o, s, ADAM7) for o, s in zip(offs, sizes)]
    assert res == [w[0] for w in want_idx] and rows == [w[1] for w in want_idx]
    sel = list(range(len(files))) if sel is None else sel
    got, host, o = _call(torch, dec, d_in, rows, sel, fmt, align, flags)
    want = [_model(buf, rows[k], flags, fmt) + (_room(rows[k], fmt),) for k in sel]
    assert got == [w[0] for w in want]
    if expect is not None:
        assert got == expect
    _check(host, o, sel, want)
    return rows, got, host, o


def _against_pixels(torch, dec, made, align=1, flags=ADAM7, seed=0):
    """format 0 against the pixels the builder put in"""
    buf, offs, sizes = _pack([g.data for g in made], seed)
    d_in, rows, res = _index_ex(torch, dec, buf, offs, sizes, ADAM7)
    assert res == [SUCCESS] * len(made)
    assert all(r[3] >> 16 & 0xFF == 1 for r in rows)
    sel = list(range(len(made)))
    got, host, o = _call(torch, dec, d_in, rows, sel, 0, align, flags)
    assert got == [SUCCESS] * len(made)
    want = []
    for g in made:
        data = pm.swap16(g.pixels) if flags & LE16 and g.depth == 16 else g.pixels
        want.append((SUCCESS, data, len(g.pixels)))
    _check(host, o, sel, want)


def test_index_with_the_flag_and_without(torch, dec):
    """flags 0: the rows and results of index_png_batch, over every defect of
    the plain reader and interlaced files and their defects; with the flag: the
    model's"""
    files = [data for data, _ in pf.defects().values()]
    files += [data for data, _, _ in p7.defects7().values()]
    files += [p7.make7(w, h, d, c, seed=w + d).data
              for (d, c), (w, h) in zip(pm.COMBOS, [(1, 1), (2, 3), (9, 9), (17, 5), (5, 17)] * 3)]
    files += [pf.make(7, 3, d, c, seed=d).data for d, c in pm.COMBOS[::4]]
    files.append(p7.make7(5, 5, before=[(b"ABCD", b"x")]).data)     # still refused
    buf, offs, sizes = _pack(files, 4)
    d_in, rows_old, res_old = _index(torch, dec, buf, offs, sizes)
    _, rows0, res0 = _index_ex(torch, dec, buf, offs, sizes, 0)
    assert rows0 == rows_old and res0 == res_old
    _, rows7, res7 = _index_ex(torch, dec, buf, offs, sizes, ADAM7)
    want = [m7.index(buf, o, s, ADAM7) for o, s in zip(offs, sizes)]
    assert res7 == [w[0] for w in want] and rows7 == [w[1] for w in want]
    names = list(pf.defects()) + list(p7.defects7())
    by_name = dict(zip(names, res7))
    assert by_name["adam7"] == SUCCESS and by_name["adam7_no_iend"] == BAD_DATA
    assert by_name["raw7_2_32"] == UNSUPPORTED and by_name["raw_2_32"] == UNSUPPORTED
    assert res7[-1] == UNSUPPORTED and res7.count(SUCCESS) == res_old.count(SUCCESS) + 5 + 1 + 15
    for r7, r0, code in zip(rows7, rows_old, res_old):
        if code == SUCCESS:
            assert r7 == r0         # a plain file's row does not change with the flag


def test_empty_passes_and_every_depth(torch, dec):
    """15 pairs x widths and heights 1 .. 9 without 6 - passes absent in every
    combination - with random filters, one call"""
    dims = (1, 2, 3, 4, 5, 7, 8, 9)
    made = [p7.make7(w, h, d, c, seed=d * 100 + c * 10 + w + 9 * h, filters="random:%d" % (w + 9 * h),
                     level=1)
            for d, c in pm.COMBOS for w in dims for h in dims]
    assert len(made) == 15 * 64
    _against_pixels(torch, dec, made, align=1)


@pytest.mark.parametrize("depth,colour,flags", ((8, 2, ADAM7), (16, 0, ADAM7 | LE16)))
def test_band_edges_inside_passes(torch, dec, depth, colour, flags):
    """height 131: pass 7 has 65 rows; height 513 at width 9: pass 1 has 65
    rows - the unfilter's second band starts inside a pass; all rows Up, all
    Average, all Paeth"""
    made = [p7.make7(w, h, depth, colour, seed=h + f, filters=f, level=1)
            for w, h in ((9, 131), (9, 513)) for f in (2, 3, 4)]
    _against_pixels(torch, dec, made, align=16, flags=flags)


def test_piece_and_tile_edges(torch, dec):
    """rows of 15, 18, 48, 51 and 99 bytes, 1-bit rows of 7, 8, 9, 127 and 129
    pixels, one image of more than one tile (150 rows of 7 pieces) between
    smaller ones; out_align 1, 16, 256"""
    made = [p7.make7(w, 6, 8, 2, seed=w, filters="random:%d" % w) for w in (5, 6, 16, 17, 33)]
    made += [p7.make7(w, 10, 1, 0, seed=w, filters="random:%d" % w) for w in (7, 8, 9, 127, 129)]
    made.insert(3, p7.make7(33, 150, 8, 2, seed=3, filters=1, level=1))
    made.append(p7.make7(300, 9, 2, 3, seed=5, filters=2))
    for align in (1, 16, 256):
        _against_pixels(torch, dec, made, align=align, seed=align)
    # the spare bits of the passes' rows set in the file: zeros in the output
    spoiled = []
    for w in (7, 9, 13):
        g = p7.make7(w, 9, 1, 0, seed=w, filters=0)

        def spoil(raws, w=w):
            out = []
            for p, r in raws:
                x0, y0, dx, dy = p7.PASSES[p]
                wp = -(-(w - x0) // dx)
                rb = (wp + 7) // 8
                a = np.frombuffer(r, dtype=np.uint8).reshape(-1, rb + 1).copy()
                a[:, -1] |= (1 << (rb * 8 - wp)) - 1
                out.append((p, a.tobytes()))
            return out
        spoiled.append(p7.make7(w, 9, 1, 0, pixels=g.pixels, filters=0, edit=spoil))
    _against_pixels(torch, dec, spoiled)


def _trns_for(g):
    """a tRNS that bites (tests/test_png_pixels_gpu.py)"""
    first = px.samples(g.pixels, g.width, g.height, g.depth, g.colour)[0, 0]
    if g.colour in (0, 2):
        return b"".join(int(v).to_bytes(2, "big") for v in first)
    if g.colour == 3:
        return bytes((i * 37 + 11) & 0xFF for i in range(max(1, (1 << g.depth) // 2)))
    return bytes(2 if g.colour == 4 else 6)


_TWINS = {}


def _twin_files():
    """all 15 pairs at 9 x 10 and 21 x 5 with a tRNS that bites: the interlaced
    files and their non-interlaced twins"""
    if not _TWINS:
        inter, plain = [], []
        for d, c in pm.COMBOS:
            for w, h in ((9, 10), (21, 5)):
                seed = d * 10 + c + w
                g = p7.make7(w, h, d, c, seed=seed, filters="random:%d" % seed)
                trns = _trns_for(g)
                inter.append(p7.make7(w, h, d, c, pixels=g.pixels, trns=trns,
                                      filters="random:%d" % seed).data)
                plain.append(pf.make(w, h, d, c, pixels=g.pixels, trns=trns,
                                     filters="random:%d" % seed).data)
        _TWINS["files"] = (_pack(inter, 3), _pack(plain, 8))
    return _TWINS["files"]


@pytest.mark.parametrize("fmt,flags", ((0, 0), (0, LE16), (px.RGB, 0), (px.RGBA | px.OUT16, 0),
                                       (px.RGBA | px.OUT16, LE16), (px.GRAY, 0)))
def test_the_twin_oracle(torch, dec, fmt, flags):
    """an interlaced file through decode_png_batch_ex gives byte for byte what
    its non-interlaced twin gives through the existing calls"""
    (buf7, offs7, sizes7), (buf, offs, sizes) = _twin_files()
    d_in7, rows7, res7 = _index_ex(torch, dec, buf7, offs7, sizes7, ADAM7)
    d_in, rows, res = _index(torch, dec, buf, offs, sizes)
    n = len(rows)
    assert res7 == res == [SUCCESS] * n
    assert [m7.plain_twin(r)[2:4] for r in rows7] == [r[2:4] for r in rows]
    sel = list(range(n))
    for align in (1, 64):
        got, host, o = _call(torch, dec, d_in7, rows7, sel, fmt, align, flags | ADAM7)
        old = torch.full((len(host),), CANARY, dtype=torch.uint8, device="cuda")
        per = torch.full((n,), UNSET, dtype=torch.int32, device="cuda")
        if fmt:
            o2 = dec.decode_png_pixels_batch(d_in, rows, sel, old, per, fmt, out_align=align,
                                             flags=flags)
        else:
            o2 = dec.decode_png_batch(d_in, rows, sel, old, per, out_align=align, flags=flags)
        torch.cuda.synchronize()
        assert o2.tolist() == o and per.tolist() == got == [SUCCESS] * n
        assert np.array_equal(old.cpu().numpy(), host)


@pytest.mark.parametrize("fmt", (0, px.RGB))
def test_one_mixed_call(torch, dec, fmt):
    """interlaced rows, plain rows, zero rows and duplicates, sel out of order:
    the same call on the older entry point with every interlaced file replaced
    by its twin gives the same offsets, results and bytes"""
    shapes = [(9, 10, 8, 2), (20, 70, 8, 2), (33, 9, 4, 3), (17, 5, 8, 0), (40, 40, 16, 4),
              (7, 7, 1, 0), (3, 131, 8, 6), (1, 1, 16, 2)]
    inter, plain = [], []
    for k, (w, h, d, c) in enumerate(shapes):
        g = pf.make(w, h, d, c, seed=k, filters="random:%d" % k)
        plain.append(g.data)
        inter.append(p7.make7(w, h, d, c, pixels=g.pixels, filters="random:%d" % k).data
                     if k % 2 == 0 else g.data)
    bad = pf.defects()["critical_unknown"][0]     # a zero row under either flag
    inter.insert(2, bad)
    plain.insert(2, bad)
    buf7, offs7, sizes7 = _pack(inter, 6)
    buf, offs, sizes = _pack(plain, 6)
    d_in7, rows7, res7 = _index_ex(torch, dec, buf7, offs7, sizes7, ADAM7)
    d_in, rows, res = _index(torch, dec, buf, offs, sizes)
    assert res7 == res and res[2] == UNSUPPORTED
    assert sum(m7.is_interlaced(r) for r in rows7) == 4
    rng = random.Random(fmt + 1)
    sel = list(range(len(inter))) + [rng.randrange(len(inter)) for _ in range(9)]
    rng.shuffle(sel)
    for align in (1, 16):
        got, host, o = _call(torch, dec, d_in7, rows7, sel, fmt, align, ADAM7 | LE16)
        old = torch.full((len(host),), CANARY, dtype=torch.uint8, device="cuda")
        per = torch.full((len(sel),), UNSET, dtype=torch.int32, device="cuda")
        if fmt:
            o2 = dec.decode_png_pixels_batch(d_in, rows, sel, old, per, fmt, out_align=align,
                                             flags=LE16)
        else:
            o2 = dec.decode_png_batch(d_in, rows, sel, old, per, out_align=align, flags=LE16)
        torch.cuda.synchronize()
        assert o2.tolist() == o and per.tolist() == got
        assert got == [UNSUPPORTED if k == 2 else SUCCESS for k in sel]
        assert np.array_equal(old.cpu().numpy(), host)


@pytest.mark.parametrize("fmt", (0, px.RGBA))
def test_defects(torch, dec, fmt):
    """a stream a pass row short, one row too long, a filter byte 5 in pass 3's
    first and pass 7's last row, a non-interlaced stream under an interlaced
    IHDR, a damaged stream, a foreign index row and a palette index out of
    range, good files between them: the model's verdicts, the neighbours exact"""
    def flip(z):
        return z[:len(z) // 2] + bytes([z[len(z) // 2] ^ 0x04]) + z[len(z) // 2 + 1:]
    d7 = p7.defects7()
    good = p7.make7(9, 10, 8, 2, seed=40).data
    names = ["short_by_a_row", "one_row_too_many", "filter_5_pass3_first", "filter_5_pass7_last",
             "plain_stream"]
    files = [good]
    for name in names:
        files += [d7[name][0], good]
    files += [p7.make7(9, 10, 8, 2, seed=41, damage=flip, level=0).data, good,
              p7.make7(2, 1, 8, 3, pixels=bytes([0, 3]), plte=pf.palette(3)).data, good,
              pf.make(9, 10, 8, 2, seed=42).data]
    expect = [SUCCESS]
    for name in names:
        expect += [d7[name][2], SUCCESS]
    expect += [BAD_DATA, SUCCESS, BAD_DATA if fmt else SUCCESS, SUCCESS, SUCCESS]
    for align in (1, 16):
        _against_model(torch, dec, files, fmt, align=align, expect=expect, seed=align)
    # a stale index: the row of one file over the bytes of another
    buf, offs, sizes = _pack([good, p7.make7(9, 10, 8, 2, seed=43, idat=50).data, good], 2)
    d_in, rows, res = _index_ex(torch, dec, buf, offs, sizes, ADAM7)
    stale = [list(r) for r in rows]
    stale[1][5] -= 1
    got, host, o = _call(torch, dec, d_in, stale, [0, 1, 2], fmt, 1, ADAM7)
    want = [_model(buf, r, 0, fmt) + (_room(r, fmt),) for r in stale]
    assert got == [w[0] for w in want] == [SUCCESS, BAD_DATA, SUCCESS]
    _check(host, o, [0, 1, 2], want)


def test_two_calls_on_one_object_with_growing_scratch(torch):
    """a small call, then one that needs more scratch of every kind, then the
    small one again, on a fresh object"""
    from libdeflate_amd import api
    d = api.Decompressor()
    try:
        small = [p7.make7(9, 3, 4, 3, seed=1).data, pf.make(9, 3, 8, 2, seed=2).data]
        _against_model(torch, d, small, px.RGB, expect=[SUCCESS] * 2)
        large = [p7.make7(200, 150, 8, 3, seed=3, filters=1, level=1),
                 p7.make7(200, 150, 8, 2, seed=4, filters=2, level=1),
                 p7.make7(150, 200, 16, 0, seed=5, filters=1, level=1)]
        _against_pixels(torch, d, large, align=256)
        _against_model(torch, d, small, px.RGBA, expect=[SUCCESS] * 2)
        _against_model(torch, d, small, 0, expect=[SUCCESS] * 2)
    finally:
        d.close()


@pytest.mark.parametrize("fmt", (0, px.RGB, px.GRAY_ALPHA | px.OUT16))
def test_a_batch_without_interlaced_rows_is_the_older_call(torch, dec, fmt):
    """bytes, offsets and results equal those of decode_png_batch /
    decode_png_pixels_batch, with the flag and without, a failed file among
    the selections"""
    def flip(z):
        return z[:len(z) // 2] + bytes([z[len(z) // 2] ^ 0x04]) + z[len(z) // 2 + 1:]
    files = [pf.make(w, h, d, c, seed=w + d, filters="random:%d" % w).data
             for (d, c), (w, h) in zip(pm.COMBOS, [(1, 1), (17, 3), (5, 70), (33, 9), (9, 9)] * 3)]
    files += [pf.make(20, 70, 8, 2, seed=5, damage=flip, level=0).data, pf.defects()["adam7"][0]]
    buf, offs, sizes = _pack(files, 1)
    d_in, rows, res = _index(torch, dec, buf, offs, sizes)
    assert res[-1] == UNSUPPORTED
    sel = list(range(len(files))) + [3, 3, 0]
    for flags in (0, LE16, ADAM7, ADAM7 | LE16):
        got, host, o = _call(torch, dec, d_in, rows, sel, fmt, 16, flags, sizes_flags=flags & ADAM7)
        old = torch.full((len(host),), CANARY, dtype=torch.uint8, device="cuda")
        per = torch.full((len(sel),), UNSET, dtype=torch.int32, device="cuda")
        if fmt:
            o2 = dec.decode_png_pixels_batch(d_in, rows, sel, old, per, fmt, out_align=16,
                                             flags=flags & LE16)
        else:
            o2 = dec.decode_png_batch(d_in, rows, sel, old, per, out_align=16, flags=flags & LE16)
        torch.cuda.synchronize()
        assert o2.tolist() == o and per.tolist() == got
        assert got[-5] == BAD_DATA and got[-4] == UNSUPPORTED
        assert np.array_equal(old.cpu().numpy(), host)
