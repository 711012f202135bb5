"""PNG files written on the GPU (libdeflate_amd_png_encode_batch).  No tolerance
anywhere: every file equals, byte for byte, what the CPU model
(tools/models/png_write.py) assembles around the same compressor object's
libdeflate_zlib_compress() of the model's filtered scanlines; result words and
index rows equal the model's word for word; the canary bytes in front of d_out
and behind out_avail stay untouched; the project's own reader and PIL read the
files back."""
import io

import numpy as np
import pytest

from tests import png_files as pf
from tools.models import png_model as pm
from tools.models import png_write as pw

pytestmark = pytest.mark.gpu

SUCCESS, INSUFFICIENT_SPACE = 0, 3
CANARY = 0xA5
GUARD = 64
ADAPTIVE = pw.ADAPTIVE


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


_COMPRESSORS, _STREAMS = {}, {}


def _comp(level):
    from libdeflate_amd import api
    if level not in _COMPRESSORS:
        _COMPRESSORS[level] = api.Compressor(level)
    return _COMPRESSORS[level]


def _zlib(level, raw):
    """the object's own libdeflate_zlib_compress() of the scanlines, once per
    level and input"""
    key = (level, raw)
    if key not in _STREAMS:
        _STREAMS[key] = _comp(level).compress("zlib", raw)
    return _STREAMS[key]


class Batch:
    """images in one input buffer, at offsets of every residue mod 16, with
    junk between them; PLTE and tRNS data behind an image's pixels"""

    def __init__(self):
        self.buf, self.rows = bytearray(b"\xEE" * 3), []

    def add(self, w, h, d, c, pixels, plte=None, trns=None, le16=False):
        row = [len(self.buf), len(pixels), w | h << 32, d | c << 8, 0, 0, 0, 0]
        self.buf += pm.swap16(pixels) if le16 and d == 16 else pixels
        for word, data, count in ((6, plte, len(plte or b"") // 3), (7, trns, len(trns or b""))):
            if data is not None:
                self.buf += b"\xEE" * (len(self.rows) % 3)
                row[word] = len(self.buf) | count << 48
                self.buf += data
        self.buf += b"\xEE" * (1 + 5 * len(self.rows) % 16)
        self.rows.append(row)
        return self

    def device(self, torch):
        return torch.frombuffer(bytearray(self.buf), dtype=torch.uint8).cuda()


def _expect(level, batch, filt, flags=0, out_avail=None):
    """-> (files, result words, index rows, the filter types of every image)"""
    raws = [pw.image_scanlines(r, batch.buf, filt, flags) for r in batch.rows]
    streams = [_zlib(level, raw) for raw, _ in raws]
    files, words, index = pw.encode(batch.rows, batch.buf, streams, out_avail)
    return files, words, index, [t for _, t in raws]


def _encode(torch, level, batch, filt, flags=0, out_avail=None, stream=None, d_in=None):
    """the call with canaries around d_out -> (result words, d_out as numpy
    (out_avail bytes), index rows as lists)"""
    comp = _comp(level)
    n = len(batch.rows)
    bound = comp.png_encode_bound(batch.rows) if n else 0
    assert bound == pw.bound(batch.rows, level)
    avail = bound if out_avail is None else out_avail
    whole = torch.full((GUARD + avail + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((n + 1, 8), -1, dtype=torch.int64, device="cuda")
    d_in = batch.device(torch) if d_in is None else d_in
    comp.encode_png_batch(batch.rows, d_in, whole[GUARD:], res, idx, filter=filt, flags=flags,
                          stream=stream, out_avail=avail)
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert not (host[:GUARD] != CANARY).any(), "bytes written in front of d_out"
    assert not (host[GUARD + avail:] != CANARY).any(), "bytes written past out_avail"
    words = [int(x) for x in res.cpu().tolist()]
    assert words[4] == -1
    rows = idx.cpu().numpy().view(np.uint64)
    assert (rows[n] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    return words[:4], host[GUARD:GUARD + avail], [[int(x) for x in r] for r in rows[:n]]


def _check(torch, level, batch, filt, flags=0, **kw):
    files, want_words, want_index, types = _expect(level, batch, filt, flags)
    words, host, rows = _encode(torch, level, batch, filt, flags, **kw)
    assert words == want_words and words[0] == SUCCESS
    at = 0
    for k, f in enumerate(files):
        got = bytes(host[at:at + len(f)])
        if got != f:
            bad = next(i for i in range(len(f)) if got[i] != f[i])
            pytest.fail("image %d %s: first wrong byte %d of %d (the IDAT payload starts at %d)"
                        % (k, pw.geometry(batch.rows[k]), bad, len(f), want_index[k][4] + 8 - at))
        at += len(f)
    assert not (host[at:] != CANARY).any(), "bytes written behind the files"
    assert rows == want_index
    return files, words, rows, types, host


def _palette_pixels(w, h, d, entries, seed):
    """indices below `entries`"""
    idx = np.random.RandomState(seed).randint(0, entries, (h, w)).astype(np.uint8)
    bits = np.unpackbits(idx[:, :, None], axis=2)[:, :, 8 - d:].reshape(h, w * d)
    return np.packbits(bits, axis=1).tobytes()


def _any_image(batch, w, h, d, c, seed, builder=pf.pixels_random, **kw):
    px = builder(w, h, d, c, seed) if builder is not pf.pixels_constant else builder(w, h, d, c)
    plte = pf.palette(min(256, 1 << d)) if c == 3 else None
    return batch.add(w, h, d, c, px, plte=plte, **kw)


@pytest.mark.parametrize("filt", [ADAPTIVE, 3])
def test_every_pair_at_tiny_sizes(torch, filt):
    """rows shorter than the unit, than 16 bytes, ragged tails"""
    b = Batch()
    for d, c in pm.COMBOS:
        for w in (1, 2, 5, 17):
            for h in (1, 2, 3):
                _any_image(b, w, h, d, c, w * 7 + h)
    files, words, rows, types, _ = _check(torch, 6, b, filt)
    if filt == ADAPTIVE:
        k = [i for i, r in enumerate(b.rows) if pw.geometry(r)[:4] == (1, 1, 16, 2)][0]
        assert types[k] == [0]      # Sub ties with None: None wins


@pytest.mark.parametrize("filt", [ADAPTIVE, 4])
def test_grey_widths_at_the_group_edges(torch, filt):
    """the three group classes' edges and the rows of two passes"""
    b = Batch()
    for w in (15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1040, 2100):
        for h in (3, 67):
            _any_image(b, w, h, 8, 0, w + h, pf.pixels_smooth)
    _check(torch, 6, b, filt)


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4, ADAPTIVE])
def test_filters_over_three_kinds_of_pixels(torch, filt):
    b = Batch()
    for builder in (pf.pixels_random, pf.pixels_smooth, pf.pixels_constant):
        for w, h, d, c in ((70, 9, 8, 2), (300, 5, 8, 0), (64, 64, 8, 2), (33, 7, 16, 6),
                           (1030, 4, 8, 4), (50, 6, 2, 0)):
            _any_image(b, w, h, d, c, 11, builder)
    files, words, rows, types, _ = _check(torch, 6, b, filt)
    if filt == ADAPTIVE:
        assert len(set(types[6 + 2])) >= 3          # the smooth 64 x 64 RGB: mixed types
        for k in range(12, 18):                     # constant: Up ties with Paeth, Up wins
            assert set(types[k][1:]) == {2}


@pytest.mark.parametrize("filt", [1, 2, 3, 4, ADAPTIVE])
def test_le16_input(torch, filt):
    b, plain = Batch(), Batch()
    for w, h, c in ((9, 4, 0), (21, 5, 2), (130, 3, 6), (1, 1, 2)):
        px = pf.pixels_smooth(w, h, 16, c, 5)
        b.add(w, h, 16, c, px, le16=True)
        plain.add(w, h, 16, c, px)
    b.add(20, 3, 8, 2, pf.pixels_random(20, 3, 8, 2, 1))        # not 16 bits: unchanged
    plain.add(20, 3, 8, 2, pf.pixels_random(20, 3, 8, 2, 1))
    swapped = _check(torch, 6, b, filt, flags=pw.LE16)[0]
    # the same pixels big-endian without the flag: the same files
    assert _check(torch, 6, plain, filt)[0] == swapped
    # and without the flag the little-endian buffer is taken as it is
    _check(torch, 6, b, filt, flags=0)


def test_palettes_and_trns(torch):
    b = Batch()
    for d in (1, 2, 4, 8):
        for entries in (1, 2, 256):
            if entries > 1 << d:
                continue
            px = _palette_pixels(13, 5, d, entries, d)
            b.add(13, 5, d, 3, px, plte=pf.palette(entries), trns=bytes(range(entries))[:max(1, entries - 1)])
    b.add(8, 3, 8, 3, _palette_pixels(8, 3, 8, 7, 1), plte=pf.palette(7))      # no tRNS
    b.add(6, 4, 8, 2, pf.pixels_random(6, 4, 8, 2, 2), trns=b"\0\1\0\2\0\3")
    b.add(6, 4, 8, 2, pf.pixels_random(6, 4, 8, 2, 3), plte=pf.palette(256))  # a suggested palette
    b.add(6, 4, 8, 6, pf.pixels_random(6, 4, 8, 6, 4), plte=pf.palette(3))
    b.add(5, 2, 16, 0, pf.pixels_random(5, 2, 16, 0, 5), trns=b"\x12\x34")
    _check(torch, 6, b, ADAPTIVE)


@pytest.mark.parametrize("level", [1, 6])
def test_the_segmentation_edge(torch, level):
    """scanlines of 131 071, 131 072 and 131 073 bytes - the last whole image,
    the first two of 16 KiB segments - and one image near the 32 KiB class"""
    b = Batch()
    for w, h in ((131070, 1), (1023, 128), (43690, 3)):
        _any_image(b, w, h, 8, 0, w, pf.pixels_smooth)
    assert [r[1] + (r[2] >> 32) for r in b.rows] == [131071, 131072, 131073]
    _any_image(b, 1024, 1025, 8, 6, 9, pf.pixels_smooth)
    _check(torch, level, b, ADAPTIVE)


def _mixed(n=300):
    """every group class and every launch group (small-buffer kernel, whole
    images, segments), in an order that mixes them"""
    rng = np.random.RandomState(77)
    b = Batch()
    for k in range(n):
        d, c = pm.COMBOS[rng.randint(len(pm.COMBOS))]
        kind = k % 10
        if k % 60 == 7:
            w, h, d, c = 256, 180 + k % 7, 8, 2          # segmented: above 128 KiB
        elif kind < 6:
            w, h = rng.randint(1, 40), rng.randint(1, 24)           # small
        elif kind < 8:
            w, h = rng.randint(40, 300), rng.randint(8, 40)
        else:
            w, h = rng.randint(300, 1200), rng.randint(2, 12)
        _any_image(b, w, h, d, c, k, (pf.pixels_random, pf.pixels_smooth)[k % 2])
    return b


def test_a_mixed_batch_in_caller_order(torch, dec):
    from libdeflate_amd import api
    b = _mixed()
    classes = {0 if pw.geometry(r)[4] <= 64 else 1 if pw.geometry(r)[4] <= 256 else 2
               for r in b.rows}
    scans = [r[1] + (r[2] >> 32) for r in b.rows]
    assert classes == {0, 1, 2}
    assert min(scans) <= 4096 and max(scans) >= 131072 and any(4096 < s < 131072 for s in scans)
    files, words, rows, types, host = _check(torch, 6, b, ADAPTIVE)
    # the round trip: the written buffer and d_index through the reader
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for f in files if Image else ():
        Image.open(io.BytesIO(f)).load()
    d_files = torch.from_numpy(host[:words[1]].copy()).cuda()
    n = len(rows)
    d_off = torch.tensor([r[0] for r in rows], dtype=torch.int64, device="cuda")
    d_n = torch.tensor([r[1] for r in rows], dtype=torch.int64, device="cuda")
    idx = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    per = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dec.index_png_batch(d_files, d_off, d_n, idx, per)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [0] * n
    assert idx.cpu().numpy().view(np.uint64).tolist() == rows
    sel = list(range(n))
    offs, total = api.png_out_sizes(rows, sel)
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    per = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dec.decode_png_batch(d_files, rows, sel, out, per)
    torch.cuda.synchronize()
    assert per.cpu().tolist() == [0] * n
    pixels = out.cpu().numpy().tobytes()
    for r, o in zip(b.rows, offs.tolist()):
        assert pixels[o:o + r[1]] == bytes(b.buf[r[0]:r[0] + r[1]])


def _short_mix():
    b = Batch()
    _any_image(b, 1, 1, 8, 0, 1)
    _any_image(b, 31, 2, 8, 2, 2, pf.pixels_smooth)
    _any_image(b, 100, 40, 8, 6, 3, pf.pixels_smooth)      # above 4 KiB
    _any_image(b, 19, 11, 4, 3, 4)
    _any_image(b, 256, 171, 8, 2, 5, pf.pixels_smooth)     # 131 499 bytes: segmented above level 0
    _any_image(b, 77, 5, 16, 4, 6)
    return b


@pytest.mark.parametrize("level", [0, 1, 6, 12])
def test_levels(torch, level):
    _check(torch, level, _short_mix(), ADAPTIVE)


def test_out_avail_exact_and_one_byte_short(torch):
    b = _short_mix()
    files, want_words, want_index, _ = _expect(6, b, ADAPTIVE)
    total = want_words[1]
    words, host, rows = _encode(torch, 6, b, ADAPTIVE, out_avail=total)
    assert words == want_words and bytes(host) == b"".join(files) and rows == want_index
    words, host, rows = _encode(torch, 6, b, ADAPTIVE, out_avail=total - 1)
    assert words == [INSUFFICIENT_SPACE] + want_words[1:]
    assert not (host != CANARY).any(), "bytes written though the files do not fit"
    assert rows == [[0xFFFFFFFFFFFFFFFF] * 8] * len(b.rows)


def test_no_images(torch):
    words, host, rows = _encode(torch, 6, Batch(), ADAPTIVE, out_avail=16)
    assert words == [SUCCESS, 0, 0, 0] and not (host != CANARY).any() and rows == []


def test_two_calls_back_to_back_on_a_stream(torch):
    """the second call's plan goes up while the first call's kernels may still
    run: the object's pinned block and scratch are shared in stream order"""
    a, b = _short_mix(), Batch()
    for w in (17, 300, 64):
        _any_image(b, w, 9, 8, 2, w, pf.pixels_smooth)
    comp = _comp(6)
    st = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(st):
        d_a, d_b = a.device(torch), b.device(torch)
        for batch, d_in in ((a, d_a), (b, d_b)):
            n = len(batch.rows)
            out = torch.full((comp.png_encode_bound(batch.rows),), CANARY, dtype=torch.uint8,
                             device="cuda")
            res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
            idx = torch.full((n, 8), -1, dtype=torch.int64, device="cuda")
            comp.encode_png_batch(batch.rows, d_in, out, res, idx, filter=2, stream=st)
            outs.append((batch, out, res, idx))
    st.synchronize()
    for batch, out, res, idx in outs:
        files, want_words, want_index, _ = _expect(6, batch, 2)
        assert [int(x) for x in res.cpu().tolist()] == want_words
        assert bytes(out.cpu().numpy()[:want_words[1]]) == b"".join(files)
        assert idx.cpu().numpy().view(np.uint64).tolist() == want_index
