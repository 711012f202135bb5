"""PNG files decoded on the GPU (libdeflate_amd_png_index_batch /
_png_decode_batch).  No tolerance anywhere: every index row word, every result
and every pixel byte equal what the CPU model (tools/models/png_model.py)
states - which tests/test_png_model.py pins against PIL - and the canary bytes
in front of d_out, in every alignment gap and behind out_avail stay untouched.
Everything queues on the default stream and synchronises once per call."""
import io
import random

import numpy as np
import pytest

from tests import png_files as pf
from tools.models import png_model as pm

pytestmark = pytest.mark.gpu

SUCCESS, BAD_DATA, SHORT_OUTPUT, INSUFFICIENT_SPACE, UNSUPPORTED = 0, 1, 2, 3, 18
CANARY = 0xA5
UNSET = -7      # d_results where nothing was written
GUARD = 64


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


def _pack(files, seed=0):
    """the files one behind the other at unaligned offsets, junk between them
    -> (buffer, offsets, sizes)"""
    rng = random.Random(seed)
    buf, offs = bytearray(), []
    for f in files:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 8)))
        offs.append(len(buf))
        buf += f
    buf += b"IDAT" * 5      # behind the last file: never read as part of it
    return bytes(buf), offs, [len(f) for f in files]


def _index(torch, dec, buf, offs, sizes):
    """the index call -> (host rows as lists, results), checked against the model"""
    n = len(offs)
    d_in = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_n = torch.tensor(sizes, dtype=torch.int64, device="cuda")
    idx = torch.full((8 * n + 8,), -1, dtype=torch.int64, device="cuda")
    per = torch.full((n + 1,), UNSET, dtype=torch.int32, device="cuda")
    dec.index_png_batch(d_in, d_off, d_n, idx, per)
    torch.cuda.synchronize()
    rows = idx.cpu().numpy().view(np.uint64).reshape(-1, 8)
    res = per.cpu().numpy()
    assert (rows[n] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and res[n] == UNSET
    want = [pm.index(buf, o, s) for o, s in zip(offs, sizes)]
    got_rows = [[int(x) for x in r] for r in rows[:n]]
    assert res[:n].tolist() == [w[0] for w in want]
    assert got_rows == [w[1] for w in want]
    for r, w in zip(got_rows, want):
        if w[0] != SUCCESS:
            assert r[2:] == [0] * 6
    return d_in, got_rows, res[:n].tolist()


def _decode(torch, dec, d_in, buf, rows, sel, align=1, flags=0, expect=None):
    """the decode call into exactly the room it needs, canaries around it;
    everything against the model.  -> (results, output bytes, offsets)"""
    from libdeflate_amd import api
    offs_want = pm.out_sizes(rows, sel, align)
    total = offs_want[-1]
    o2, t2 = api.png_out_sizes(rows, sel, align)
    assert o2.tolist() == offs_want and t2 == total
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    out = whole[GUARD:]
    per = torch.full((len(sel) + 1,), UNSET, dtype=torch.int32, device="cuda")
    offs = dec.decode_png_batch(d_in, rows, sel, out, per, out_align=align, flags=flags,
                                out_avail=total)
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
        code, pixels = _model(buf, rows[k], flags)
        want_res.append(code)
        if pixels is not None:
            want[offs_want[r]:offs_want[r] + len(pixels)] = np.frombuffer(pixels, dtype=np.uint8)
        elif not pm.is_zero(rows[k]):
            # a failed selection's room is undefined - and nothing around it
            size = (rows[k][2] >> 32) * pm.row_rowbytes(rows[k])
            defined[offs_want[r]:offs_want[r] + size] = False
    assert res[:len(sel)].tolist() == want_res
    if expect is not None:
        assert want_res == expect
    bad = np.nonzero((host != want) & defined)[0]
    assert bad.size == 0, "first wrong byte at %d of %d" % (bad[0], total)
    return want_res, host, offs_want


_MODEL = {}


def _model(buf, row, flags):
    """pm.decode, computed once per file, row and flags"""
    key = (buf[row[0]:row[0] + row[1]], row[4] - row[0], tuple(row[2:4]), row[5], flags)
    if key not in _MODEL:
        _MODEL[key] = pm.decode(buf, row, flags)
    return _MODEL[key]


def _both(torch, dec, files, sel=None, align=1, flags=0, expect=None, seed=0):
    buf, offs, sizes = _pack(files, seed)
    d_in, rows, res = _index(torch, dec, buf, offs, sizes)
    sel = list(range(len(files))) if sel is None else sel
    return rows, res, _decode(torch, dec, d_in, buf, rows, sel, align, flags, expect)


def test_geometry(torch, dec):
    """heights around the band of 64 rows (two hand-overs and a partial band),
    rowbytes around the 16-byte piece, one column and one row"""
    files = [pf.make(rb, h, 8, 0, filters="random:%d" % (rb + h), seed=rb * h).data
             for h in (1, 63, 64, 65, 130) for rb in (1, 15, 16, 17, 33)]
    files += [pf.make(1, 65, 8, 2, filters="random:1").data,
              pf.make(65, 1, 8, 2, filters="random:2").data,
              pf.make(1, 65, 16, 6, filters=4).data, pf.make(65, 1, 1, 0, filters=3).data]
    _both(torch, dec, files, expect=[SUCCESS] * len(files))


@pytest.mark.parametrize("filters", [0, 1, 2, 3, 4, "random:7"])
def test_every_depth_and_colour_with_every_filter(torch, dec, filters):
    """all 15 pairs, so all six filter units, 65 wide and 67 high: uniform
    random bytes (Paeth ties, Average carries) and constant content (every
    predictor exact)"""
    files = []
    for depth, colour in pm.COMBOS:
        files.append(pf.make(65, 67, depth, colour, filters=filters, seed=depth + colour).data)
        files.append(pf.make(65, 67, depth, colour, filters=filters,
                             pixels=pf.pixels_constant(65, 67, depth, colour)).data)
    rows, res, _ = _both(torch, dec, files, expect=[SUCCESS] * 30)
    assert sorted({r[3] >> 24 & 0xFF for r in rows}) == [1, 2, 3, 4, 6, 8]


def test_idat_layouts(torch, dec):
    """the stream in one chunk, in 1-byte chunks (the zlib header and the
    Adler-32 split), in 8192-byte chunks, with an empty IDAT in the middle and
    behind the end, ancillary chunks around the run, bytes behind IEND"""
    big = dict(width=130, height=65, depth=16, colour=2, seed=4, filters="random:4")
    small = dict(width=17, height=9, depth=8, colour=0, seed=5, filters="random:5")
    text = [(b"tEXt", b"Comment\0hello"), (b"gAMA", b"\0\0\xb1\x8f")]
    files = [pf.make(**big).data, pf.make(idat=8192, **big).data, pf.make(idat=1, **small).data,
             pf.make(idat=[100, 0, 0, 200], **big).data, pf.make(idat=[0, 5], **small).data,
             pf.make(before=text, after=text[:1], idat=3000, **big).data,
             pf.make(tail=b"IDAT after the end", trns=b"\0\1", **small).data]
    big_z = len(files[0]) - 33 - 24
    assert big_z > 3 * 8192
    rows, res, _ = _both(torch, dec, files, expect=[SUCCESS] * len(files))
    assert rows[6][7] >> 48 == 2 and rows[5][5] == rows[0][5]
    # an empty IDAT behind the stream's end belongs to the run
    g = pf.make(**small)
    z_end = len(g.data) - 12
    extra = g.data[:z_end] + pf.chunk(b"IDAT") + g.data[z_end:]
    _both(torch, dec, [extra, g.data], expect=[SUCCESS, SUCCESS])


def _mixed_batch():
    rng = random.Random(11)
    defects = list(pf.defects().items())
    files, names = [], []
    for i in range(300):
        if i % 6 == 5:
            name, (data, _) = defects[(i // 6) % len(defects)]
            files.append(data)
            names.append(name)
            continue
        depth, colour = pm.COMBOS[rng.randrange(15)]
        w, h = rng.choice((1, 3, 16, 17, 40)), rng.choice((1, 2, 31, 64, 65, 70))
        kind = rng.randrange(3)
        px = (pf.pixels_smooth(w, h, depth, colour, i) if kind == 0 else
              pf.pixels_constant(w, h, depth, colour, i & 0xFF) if kind == 1 else None)
        files.append(pf.make(w, h, depth, colour, pixels=px, seed=i,
                             filters=rng.choice(("adaptive", "random:%d" % i, 4, 3)),
                             idat=rng.choice((None, None, 7, 500))).data)
        names.append("good")
    return files, names


@pytest.mark.parametrize("align", (1, 64))
def test_batch_of_mixed_files(torch, dec, align):
    """300 files at unaligned offsets, the defect files among them: each gets
    its stated result and a zero row, and its good neighbours' bytes stay
    exact; a selection in shuffled order with duplicates, refused files
    selected too (UNSUPPORTED, no room)"""
    files, names = _mixed_batch()
    verdicts = {n: v for n, (_, v) in pf.defects().items()}
    buf, offs, sizes = _pack(files, 3)
    d_in, rows, res = _index(torch, dec, buf, offs, sizes)
    assert res == [SUCCESS if n == "good" else verdicts[n] for n in names]
    rng = random.Random(align)
    sel = list(range(300)) + [rng.randrange(300) for _ in range(60)]
    rng.shuffle(sel)
    got, _, offs_out = _decode(torch, dec, d_in, buf, rows, sel, align)
    assert got == [SUCCESS if names[k] == "good" else UNSUPPORTED for k in sel]
    assert all(o % align == 0 for o in offs_out)


def test_decode_time_failures(torch, dec):
    """a filter byte of 5 in the last row of band 0 and in the first row of
    band 1, a flipped byte in the zlib body, a stream one row short and one row
    long, and index rows whose IDAT sum was altered on the host: each its own
    result, the good files between them exact, nothing outside the rooms"""
    geo = dict(width=20, height=70, depth=8, colour=2)
    good = pf.make(seed=1, filters="random:1", **geo).data

    def flip(z):
        return z[:len(z) // 2] + bytes([z[len(z) // 2] ^ 0x04]) + z[len(z) // 2 + 1:]
    files = [good,
             pf.make(seed=2, filters=[4] * 63 + [5] + [2] * 6, **geo).data, good,
             pf.make(seed=3, filters=[3] * 64 + [5] + [1] * 5, **geo).data, good,
             pf.make(seed=4, damage=flip, level=0, **geo).data, good,
             pf.make(seed=5, rows_delta=-1, **geo).data, good,
             pf.make(seed=6, rows_delta=1, **geo).data, good,
             pf.make(seed=7, idat=[50, 60], **geo).data, good,
             pf.make(seed=8, idat=[50, 60], **geo).data, good]
    buf, offs, sizes = _pack(files, 5)
    d_in, rows, res = _index(torch, dec, buf, offs, sizes)
    assert res == [SUCCESS] * len(files)
    rows[11][5] -= 1    # within what the call accepts: the gather finds it
    rows[13][5] += 1
    expect = [SUCCESS, BAD_DATA, SUCCESS, BAD_DATA, SUCCESS, BAD_DATA, SUCCESS, SHORT_OUTPUT,
              SUCCESS, INSUFFICIENT_SPACE, SUCCESS, BAD_DATA, SUCCESS, BAD_DATA, SUCCESS]
    for align in (1, 64):
        _decode(torch, dec, d_in, buf, rows, list(range(len(files))), align, expect=expect)


@pytest.mark.parametrize("height", (65, 130))
def test_le16(torch, dec, height):
    """16-bit grey, RGB and RGBA with all rows Up, all Paeth and all Average -
    the rows that read the band before - against the model's bytes swapped;
    an 8-bit image under the flag is unchanged"""
    files, plain = [], []
    for colour in (0, 2, 6):
        for filters in (2, 4, 3, "random:9"):
            g = pf.make(19, height, 16, colour, filters=filters, seed=colour + height)
            files.append(g.data)
            plain.append(g.pixels)
    g8 = pf.make(19, height, 8, 6, filters=4, seed=8)
    files.append(g8.data)
    rows, res, (codes, host, offs) = _both(torch, dec, files, flags=pm.LE16,
                                           expect=[SUCCESS] * len(files))
    for k, px in enumerate(plain):
        got = host[offs[k]:offs[k] + len(px)]
        assert np.array_equal(got.view("<u2"), np.frombuffer(px, dtype=">u2"))
    assert host[offs[-2]:offs[-1]].tobytes() == g8.pixels
    _both(torch, dec, files, flags=0, align=64, expect=[SUCCESS] * len(files))


def test_pil_written_files(torch, dec):
    """files PIL writes, where PIL imports, come out as PIL's own pixels (the
    model's in any case)"""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    h, w = 70, 45
    y, x = np.mgrid[0:h, 0:w]
    rgb = np.stack([x * 5 + y, x + y * 3, (x * y) // 7], axis=2).astype(np.uint8)
    if Image is None:
        files = [pf.make(w, h, 8, 2, pixels=rgb.tobytes()).data]
        _both(torch, dec, files, expect=[SUCCESS])
        return
    images = [Image.fromarray(rgb), Image.fromarray(rgb[:, :, 0]),
              Image.fromarray(np.dstack([rgb, rgb[:, :, :1]])),
              Image.fromarray((x * 900 + y * 31).astype(np.uint16)),
              Image.fromarray(rgb).quantize(16)]
    files = []
    for im in images:
        f = io.BytesIO()
        im.save(f, "PNG")
        files.append(f.getvalue())
    from libdeflate_amd import api
    rows, res, (codes, host, offs) = _both(torch, dec, files, flags=pm.LE16,
                                           expect=[SUCCESS] * len(files))
    shapes = api.png_shapes(rows)
    for k, im in enumerate(images[:4]):
        hh, ww, ch, depth, colour = shapes[k]
        back = np.asarray(Image.open(io.BytesIO(files[k])))
        got = host[offs[k]:offs[k] + hh * ww * ch * depth // 8]
        got = got.view(np.uint16 if depth == 16 else np.uint8).reshape(back.shape)
        assert np.array_equal(got, back), k
    assert shapes[4][3:] == (4, 3) and rows[4][6] >> 48 == 16
