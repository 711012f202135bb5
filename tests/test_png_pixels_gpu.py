"""PNG files decoded on the GPU to one pixel format
(libdeflate_amd_png_decode_pixels_batch).  No tolerance anywhere: every result
and every byte equal what the CPU model (tools/models/png_pixels_model.py)
states - which tests/test_png_pixels_model.py pins against hand-written
vectors and PIL - and the canary bytes in front of d_out, in every alignment
gap and behind out_avail stay untouched.  The harness is that of
tests/test_png_gpu.py: files packed at unaligned offsets, the index call first,
the output in exactly the room it needs.  The shapes are the smallest at which
the convert kernel takes another path: 16 pixels to a thread, 4096 to a tile,
a 16-byte piece of output, a scanline's padding bits."""
import random

import numpy as np
import pytest

from tests import png_files as pf
from tests.test_png_gpu import CANARY, GUARD, UNSET, _index, _pack
from tools.models import png_model as pm
from tools.models import png_pixels_model as px

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE, UNSUPPORTED = 0, 1, 2, 3, 18
V16 = [0, 127, 128, 129, 255, 256, 257, 383, 384, 385, 65407, 65408, 65535]
W16 = [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 255, 255, 255]


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


_MODEL = {}


def _model(buf, row, fmt, flags):
    """px.decode, computed once per file, row, format and flags"""
    key = (buf[row[0]:row[0] + row[1]], tuple(row[2:]), row[0], fmt, flags)
    if key not in _MODEL:
        _MODEL[key] = px.decode(buf, row, fmt, flags)
    return _MODEL[key]


def _decode(torch, dec, d_in, buf, rows, sel, fmt, align=1, flags=0, expect=None):
    """the call into exactly the room it needs, canaries around it; everything
    against the model.  -> (results, output bytes, offsets)"""
    from libdeflate_amd import api
    offs_want = px.out_sizes(rows, sel, fmt, align)
    total = offs_want[-1]
    o2, t2 = api.png_pixels_out_sizes(rows, sel, fmt, align)
    assert o2.tolist() == offs_want and t2 == total
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    out = whole[GUARD:]
    per = torch.full((len(sel) + 1,), UNSET, dtype=torch.int32, device="cuda")
    offs = dec.decode_png_pixels_batch(d_in, rows, sel, out, per, fmt, out_align=align,
                                       flags=flags, out_avail=total)
    torch.cuda.synchronize()
    assert offs.tolist() == offs_want
    host = whole.cpu().numpy()
    assert not (host[:GUARD] != CANARY).any(), "bytes written in front of d_out"
    assert not (host[GUARD + total:] != CANARY).any(), "bytes written past out_avail"
    host = host[GUARD:GUARD + total]
    res = per.cpu().numpy()
    assert res[len(sel)] == UNSET
    want = np.full(total, CANARY, dtype=np.uint8)
    defined = np.ones(total, dtype=bool)
    want_res = []
    for r, k in enumerate(sel):
        code, pixels = _model(buf, rows[k], fmt, flags)
        want_res.append(code)
        if pixels is not None:
            assert len(pixels) == px.out_bytes(rows[k], fmt)
            want[offs_want[r]:offs_want[r] + len(pixels)] = np.frombuffer(pixels, dtype=np.uint8)
        elif not pm.is_zero(rows[k]):
            # a failed selection's room is undefined - and nothing around it
            defined[offs_want[r]:offs_want[r] + px.out_bytes(rows[k], fmt)] = False
    assert res[:len(sel)].tolist() == want_res
    if expect is not None:
        assert want_res == expect
    bad = np.nonzero((host != want) & defined)[0]
    assert bad.size == 0, "first wrong byte at %d of %d" % (bad[0], total)
    return want_res, host, offs_want


def _both(torch, dec, files, fmt, sel=None, align=1, flags=0, expect=None, seed=0):
    buf, offs, sizes = _pack(files, seed)
    d_in, rows, res = _index(torch, dec, buf, offs, sizes)
    sel = list(range(len(files))) if sel is None else sel
    return rows, _decode(torch, dec, d_in, buf, rows, sel, fmt, align, flags, expect)


def _trns_for(g):
    """a tRNS that bites: the first pixel as the colour key of a grey or RGB
    image, alphas for half a palette, bytes to ignore for the others"""
    first = px.samples(g.pixels, g.width, g.height, g.depth, g.colour)[0, 0]
    if g.colour in (0, 2):
        return b"".join(int(v).to_bytes(2, "big") for v in first)
    if g.colour == 3:
        return bytes((i * 37 + 11) & 0xFF for i in range(max(1, (1 << g.depth) // 2)))
    return bytes(2 if g.colour == 4 else 6)


_FILES = {}


def _all_pairs(trns):
    """all 15 pairs at widths 1, 2, 7, 9, 17, 33 and heights 1 and 3, random
    pixels and filters"""
    if trns not in _FILES:
        files = []
        for depth, colour in pm.COMBOS:
            for w in (1, 2, 7, 9, 17, 33):
                for h in (1, 3):
                    seed = depth * 1000 + colour * 100 + w * 2 + h
                    g = pf.make(w, h, depth, colour, filters="random:%d" % seed, seed=seed)
                    if trns:
                        g = pf.make(w, h, depth, colour, filters="random:%d" % seed, seed=seed,
                                    trns=_trns_for(g))
                    files.append(g.data)
        _FILES[trns] = _pack(files, 7)
    return _FILES[trns]


@pytest.mark.parametrize("trns", (False, True))
@pytest.mark.parametrize("fmt", px.FORMATS)
def test_every_depth_and_colour_to_every_format(torch, dec, fmt, trns):
    """15 pairs x 6 widths x 2 heights in one call per out_align; with a tRNS
    that matches a pixel, and then little-endian where the samples are 16-bit"""
    buf, offs, sizes = _all_pairs(trns)
    d_in, rows, res = _index(torch, dec, buf, offs, sizes)
    assert res == [SUCCESS] * 180
    if trns:
        assert all(r[7] for r in rows)
    for align in (1, 16, 256):
        _decode(torch, dec, d_in, buf, rows, list(range(180)), fmt, align,
                flags=pm.LE16 if trns else 0, expect=[SUCCESS] * 180)


def test_piece_edges_of_three_channel_output(torch, dec):
    """15, 18, 48 and 51 bytes of RGB: below a piece, across one, three whole
    pieces, and a byte tail behind them"""
    files = [pf.make(w, 1, depth, colour, seed=w + depth, filters=1).data
             for w in (5, 6, 16, 17) for depth, colour in ((8, 0), (8, 3), (16, 2), (8, 6), (4, 0))]
    for align in (1, 16):
        _both(torch, dec, files, px.RGB, align=align, expect=[SUCCESS] * len(files))


@pytest.mark.parametrize("fmt", (px.GRAY, px.RGB))
def test_padding_bits_of_a_scanline(torch, dec, fmt):
    """depths 1, 2, 4 at widths 1 .. 9 and height 3: a row ends inside a byte
    and the next starts on one, with the spare bits set in the file"""
    files = []
    for depth in (1, 2, 4):
        for colour in (0, 3):
            for w in range(1, 10):
                rb = pm.rowbytes(w, depth, colour)
                a = np.random.RandomState(w * depth).randint(0, 256, (3, rb)).astype(np.uint8)
                files.append(pf.make(w, 3, depth, colour, pixels=a.tobytes(), filters=2).data)
    _both(torch, dec, files, fmt, expect=[SUCCESS] * len(files))


def test_palette_sizes_and_trns_lengths(torch, dec):
    files = []
    for entries, depth in ((1, 1), (1, 8), (3, 2), (3, 8), (256, 8)):
        for n_trns in (0, 1, entries, entries + 1):
            w, h = 19, 2
            idx = np.random.RandomState(entries + n_trns).randint(0, entries, (h, w))
            if depth == 8:
                pixels = idx.astype(np.uint8).tobytes()
            else:
                bits = ((idx[:, :, None] >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8)
                pixels = np.packbits(bits.reshape(h, -1), axis=1).tobytes()
            files.append(pf.make(w, h, depth, 3, pixels=pixels, plte=pf.palette(entries),
                                 trns=bytes((7 * i + 3) & 0xFF for i in range(n_trns)),
                                 filters="random:%d" % n_trns).data)
    for fmt in (px.RGBA, px.RGB, px.GRAY_ALPHA | px.OUT16):
        rows, _ = _both(torch, dec, files, fmt, expect=[SUCCESS] * len(files))
    assert sorted({r[6] >> 48 for r in rows}) == [1, 3, 256]
    assert rows[0][7] and rows[0][7] >> 48 == 0     # an empty tRNS is a tRNS


def test_palette_index_out_of_range(torch, dec):
    """one 2 x 1 image of 3 entries that holds index 3, at 8 and at 2 bits:
    BAD_DATA for it, its neighbours exact"""
    good = pf.make(9, 3, 8, 3, seed=1).data
    bad8 = pf.make(2, 1, 8, 3, pixels=bytes([0, 3]), plte=pf.palette(3)).data
    bad2 = pf.make(2, 1, 2, 3, pixels=bytes([0b10110000]), plte=pf.palette(3)).data
    ok2 = pf.make(2, 1, 2, 3, pixels=bytes([0b10011111]), plte=pf.palette(3)).data
    files = [good, bad8, good, bad2, good, ok2]
    for fmt in (px.RGB, px.RGBA | px.OUT16):
        for align in (1, 16):
            _both(torch, dec, files, fmt, align=align,
                  expect=[SUCCESS, BAD_DATA, SUCCESS, BAD_DATA, SUCCESS, SUCCESS])


def test_colour_keys(torch, dec):
    """a pixel equal to the key, one differing in the lowest bit, one in one
    channel; a tRNS of a wrong length and one on colour types 4 and 6 ignored"""
    files, alphas = [], []
    for depth in (1, 2, 4, 8, 16):
        top = (1 << depth) - 1
        key = top & 0xA5A6
        vals = [key, key ^ 1, key, top - key]
        if depth == 16:
            pixels = np.array(vals, dtype=">u2").tobytes()
        elif depth == 8:
            pixels = bytes(vals)
        else:
            bits = ((np.array(vals)[:, None] >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8)
            pixels = np.packbits(bits.reshape(-1)).tobytes()
        # bits above the depth are not part of the key
        word = key if depth == 16 else key | 0x5A00 & ~top
        files.append(pf.make(4, 1, depth, 0, pixels=pixels, trns=word.to_bytes(2, "big")).data)
        alphas.append([0 if v == key else 255 for v in vals])
        for n in (1, 3, 7):
            files.append(pf.make(4, 1, depth, 0, pixels=pixels, trns=bytes(n)).data)
            alphas.append([255] * 4)
    for depth in (8, 16):
        dt = ">u2" if depth == 16 else np.uint8
        k = [0x1234, 0x00FF, 0x8001] if depth == 16 else [0x12, 0xFF, 0x81]
        px_rows = [k, [k[0], k[1], k[2] ^ 1], [k[0] ^ 0x10, k[1], k[2]], k]
        pixels = np.array(px_rows, dtype=dt).tobytes()
        word = b"".join((v | (0x7700 if depth == 8 else 0)).to_bytes(2, "big") for v in k)
        files.append(pf.make(4, 1, depth, 2, pixels=pixels, trns=word).data)
        alphas.append([0, 255, 255, 0])
        for n in (1, 3, 7):
            files.append(pf.make(4, 1, depth, 2, pixels=pixels, trns=bytes(n)).data)
            alphas.append([255] * 4)
    files.append(pf.make(4, 1, 8, 4, pixels=bytes([0, 9, 0, 0, 1, 7, 0, 255]), trns=bytes(2)).data)
    alphas.append([9, 0, 7, 255])
    files.append(pf.make(4, 1, 8, 6, pixels=bytes([0, 0, 0, 9] * 4), trns=bytes(6)).data)
    alphas.append([9] * 4)
    for fmt in (px.GRAY_ALPHA, px.RGBA, px.RGBA | px.OUT16):
        rows, (codes, host, offs) = _both(torch, dec, files, fmt, expect=[SUCCESS] * len(files))
        if fmt == px.RGBA:      # the alphas by hand, not only the model's
            for k, want in enumerate(alphas):
                assert host[offs[k]:offs[k] + 16][3::4].tolist() == want, k


def test_depth_scaling_vectors(torch, dec):
    """16 -> 8 around the rounding points as one 13 x 1 image; 8 -> 16 of all
    256 values"""
    v16 = pf.make(13, 1, 16, 0, pixels=np.array(V16, dtype=">u2").tobytes()).data
    v8 = pf.make(256, 1, 8, 0, pixels=bytes(range(256)), filters=1).data
    rows, (codes, host, offs) = _both(torch, dec, [v16, v8], px.GRAY, expect=[SUCCESS] * 2)
    assert host[:13].tolist() == W16
    rows, (codes, host, offs) = _both(torch, dec, [v16, v8], px.RGB, expect=[SUCCESS] * 2)
    assert host[:39].tolist() == [v for v in W16 for _ in range(3)]
    rows, (codes, host, offs) = _both(torch, dec, [v16, v8], px.GRAY | px.OUT16, flags=pm.LE16,
                                      expect=[SUCCESS] * 2)
    assert host[:26].view("<u2").tolist() == V16
    assert host[26:].view("<u2").tolist() == [257 * i for i in range(256)]


@pytest.mark.parametrize("height", (65, 130))
def test_le16(torch, dec, height):
    """direct: 16-bit RGB and grey, width 3, all rows Up, Paeth and Average -
    the rows that read the band before, which the swap must not have touched;
    converted: grey 8 -> RGB16 and palette -> RGBA16"""
    for colour, fmt in ((2, px.RGB | px.OUT16), (0, px.GRAY | px.OUT16)):
        made = [pf.make(3, height, 16, colour, filters=f, seed=colour + height + f)
                for f in (2, 4, 3)]
        rows, (codes, host, offs) = _both(torch, dec, [g.data for g in made], fmt, flags=pm.LE16,
                                          expect=[SUCCESS] * 3)
        for k, g in enumerate(made):
            got = host[offs[k]:offs[k] + len(g.pixels)]
            assert np.array_equal(got.view("<u2"), np.frombuffer(g.pixels, dtype=">u2"))
        _both(torch, dec, [g.data for g in made], fmt, flags=0, align=16, expect=[SUCCESS] * 3)
    g8 = pf.make(3, height, 8, 0, filters=4, seed=height)
    pal = pf.make(3, height, 8, 3, filters=3, seed=height + 1, trns=bytes(range(100)))
    for fmt in (px.RGB | px.OUT16, px.RGBA | px.OUT16):
        rows, (codes, host, offs) = _both(torch, dec, [g8.data, pal.data], fmt, flags=pm.LE16,
                                          expect=[SUCCESS] * 2)
        ch = fmt & 0xF
        got = host[:3 * height * ch * 2].view("<u2").reshape(-1, ch)
        assert np.array_equal(got[:, 0], np.frombuffer(g8.pixels, dtype=np.uint8).astype(np.uint32) * 257)


@pytest.mark.parametrize("flags", (0, pm.LE16))
def test_direct_selections_are_decode_png_batch_bytes(torch, dec, flags):
    """a selection that already is the format gives byte for byte what
    decode_png_batch gives for the same row - compared to that call"""
    pairs = {px.GRAY: (8, 0), px.GRAY_ALPHA: (8, 4), px.RGB: (8, 2), px.RGBA: (8, 6),
             px.GRAY | px.OUT16: (16, 0), px.GRAY_ALPHA | px.OUT16: (16, 4),
             px.RGB | px.OUT16: (16, 2), px.RGBA | px.OUT16: (16, 6)}
    files = [pf.make(w, h, d, c, seed=d + c + w, filters="random:%d" % w).data
             for d, c in pairs.values() for w, h in ((1, 1), (17, 3), (5, 70))]
    buf, offs, sizes = _pack(files, 2)
    d_in, rows, res = _index(torch, dec, buf, offs, sizes)
    for fmt, (d, c) in pairs.items():
        sel = [k for k, r in enumerate(rows) if (r[3] & 0xFF, r[3] >> 8 & 0xFF) == (d, c)]
        assert len(sel) == 3 and all(px.is_direct(d, c, fmt) for _ in sel)
        codes, host, o = _decode(torch, dec, d_in, buf, rows, sel, fmt, 16, flags,
                                 expect=[SUCCESS] * 3)
        plain = torch.full((len(host),), CANARY, dtype=torch.uint8, device="cuda")
        per = torch.full((3,), UNSET, dtype=torch.int32, device="cuda")
        o2 = dec.decode_png_batch(d_in, rows, sel, plain, per, out_align=16, flags=flags)
        torch.cuda.synchronize()
        assert o2.tolist() == o and per.tolist() == [SUCCESS] * 3
        assert np.array_equal(plain.cpu().numpy(), host)


@pytest.mark.parametrize("fmt", (px.RGB, px.RGBA | px.OUT16))
def test_one_mixed_call(torch, dec, fmt):
    """direct and converted selections, a zero row, a damaged zlib stream, a
    filter byte 5 and a bad palette index in one call, shuffled and with
    duplicates: every result and every defined byte exact, nothing written
    outside the failed rooms"""
    def flip(z):
        return z[:len(z) // 2] + bytes([z[len(z) // 2] ^ 0x04]) + z[len(z) // 2 + 1:]
    depth = 16 if fmt & px.OUT16 else 8
    files = [pf.make(20, 70, depth, 2, seed=1, filters="random:1").data,    # direct for RGB
             pf.make(20, 70, depth, 6, seed=2, filters="random:2").data,    # direct for RGBA
             pf.make(33, 9, 4, 3, seed=3, trns=bytes(range(9))).data,
             pf.make(17, 5, 8, 0, seed=4, trns=bytes([0, 7])).data,
             pf.defects()["adam7"][0],
             pf.make(20, 70, 8, 2, seed=5, damage=flip, level=0).data,
             pf.make(20, 70, 8, 3, seed=6, damage=flip, level=0).data,
             pf.make(20, 70, depth, 2, seed=7, filters=[4] * 63 + [5] + [2] * 6).data,
             pf.make(20, 70, 8, 4, seed=8, filters=[3] * 64 + [5] + [1] * 5).data,
             pf.make(2, 1, 8, 3, pixels=bytes([0, 3]), plte=pf.palette(3)).data,
             pf.make(40, 40, 16, 4, seed=9).data,
             pf.make(7, 7, 1, 0, seed=10).data]
    buf, offs, sizes = _pack(files, 9)
    d_in, rows, res = _index(torch, dec, buf, offs, sizes)
    assert res == [SUCCESS] * 4 + [UNSUPPORTED] + [SUCCESS] * 7
    rng = random.Random(fmt)
    sel = list(range(len(files))) + [rng.randrange(len(files)) for _ in range(12)]
    rng.shuffle(sel)
    by_file = [SUCCESS, SUCCESS, SUCCESS, SUCCESS, UNSUPPORTED, BAD_DATA, BAD_DATA, BAD_DATA,
               BAD_DATA, BAD_DATA, SUCCESS, SUCCESS]
    for align in (1, 64):
        _decode(torch, dec, d_in, buf, rows, sel, fmt, align, flags=pm.LE16,
                expect=[by_file[k] for k in sel])


def test_tiles(torch, dec):
    """many tiles of one image, a tile's end inside a scanline and scanlines
    of one pixel, and 300 images of one pixel: 300 tiles of one thread"""
    big = pf.make(300, 300, 8, 3, seed=1, filters="random:1", trns=bytes(range(0, 256, 3)))
    _both(torch, dec, [big.data], px.RGB, expect=[SUCCESS])
    _both(torch, dec, [big.data], px.RGBA | px.OUT16, expect=[SUCCESS])
    wide = pf.make(70000, 1, 1, 0, seed=2, filters=1)
    tall = pf.make(1, 70000, 1, 0, seed=3, filters=0)
    _both(torch, dec, [wide.data, tall.data], px.GRAY, expect=[SUCCESS] * 2)
    ones = [pf.make(1, 1, d, c, seed=i, filters=i % 5).data
            for i, (d, c) in enumerate(pm.COMBOS * 20)]
    assert len(ones) == 300
    _both(torch, dec, ones, px.RGB, align=1, expect=[SUCCESS] * 300)
    _both(torch, dec, ones, px.GRAY_ALPHA | px.OUT16, align=16, expect=[SUCCESS] * 300)


def test_two_calls_on_one_object_with_growing_scratch(torch):
    """a small call, a decode_png_batch call, then a call that needs more
    scratch, all on a fresh object: each exact"""
    from libdeflate_amd import api
    d = api.Decompressor()
    try:
        small = [pf.make(9, 3, 4, 3, seed=1).data, pf.make(9, 3, 8, 2, seed=2).data]
        _both(torch, d, small, px.RGB, expect=[SUCCESS] * 2)
        buf, offs, sizes = _pack(small, 1)
        d_in, rows, res = _index(torch, d, buf, offs, sizes)
        total = pm.out_sizes(rows, [0, 1])[-1]
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        per = torch.full((2,), UNSET, dtype=torch.int32, device="cuda")
        d.decode_png_batch(d_in, rows, [0, 1], out, per)
        torch.cuda.synchronize()
        assert per.tolist() == [SUCCESS] * 2
        assert out.cpu().numpy().tobytes() == b"".join(pm.decode(buf, r)[1] for r in rows)
        large = [pf.make(200, 150, 8, 3, seed=3).data, pf.make(200, 150, 8, 2, seed=4).data,
                 pf.make(150, 200, 16, 0, seed=5).data]
        _both(torch, d, large, px.RGB, align=256, expect=[SUCCESS] * 3)
        _both(torch, d, small, px.RGBA, expect=[SUCCESS] * 2)
    finally:
        d.close()
