"""Adam7-interlaced PNG files built by hand for the tests and the benchmark of
the PNG reader's _ex calls, on tests/png_files.py: the pixel bits of an image
taken apart into the seven passes (bits[y0::dy, x0::dx]), every pass repacked
to its own row bytes and filtered on its own, the passes concatenated and
compressed; and the defects the decode has a verdict for."""
import zlib

import numpy as np

from tests import png_files as pf
from tools.models import png_model as pm

# (x0, y0, dx, dy), PNG specification 8.2 - written out here, not taken from
# the model under test
PASSES = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2),
          (0, 1, 1, 2))


def pass_images(pixels, width, height, depth, colour):
    """[(pass number 0 .. 6, h_p, rb_p, the h_p * rb_p bytes)] of the present
    passes, in order"""
    bits = depth * pm.channels(colour)
    rows = np.frombuffer(pixels, dtype=np.uint8).reshape(height, pm.rowbytes(width, depth, colour))
    grid = np.unpackbits(rows, axis=1)[:, :width * bits].reshape(height, width, bits)
    out = []
    for p, (x0, y0, dx, dy) in enumerate(PASSES):
        part = grid[y0::dy, x0::dx]
        if part.shape[0] == 0 or part.shape[1] == 0:
            continue
        packed = np.packbits(part.reshape(part.shape[0], -1), axis=1)
        out.append((p, part.shape[0], packed.shape[1], packed.tobytes()))
    return out


def make7(width, height, depth=8, colour=2, pixels=None, filters="adaptive", idat=None,
          before=(), after=(), level=6, seed=1, plte=None, trns=None, interlace=1,
          edit=None, damage=None, tail=b""):
    """An interlaced PNG file whose image is `pixels` (height * rowbytes bytes,
    default: random) -> png_files.Png, its .pixels those of the non-interlaced
    twin.  filters: as png_files.scanlines takes them, applied to every pass
    ("random:<seed>" draws on per pass); or a dict {pass number: filters} with
    "adaptive" for the others.  edit(raws) -> raws: applied to the list of the
    present passes' filtered scanlines [(pass number, bytes)] before they are
    joined.  damage, idat, before, after, plte, trns, tail: as
    png_files.make."""
    unit = pm.bpp(depth, colour)
    if pixels is None:
        pixels = pf.pixels_random(width, height, depth, colour, seed)
    raws = []
    for p, hp, rb, data in pass_images(pixels, width, height, depth, colour):
        f = filters
        if isinstance(f, dict):
            f = f.get(p, "adaptive")
        elif isinstance(f, str) and f.startswith("random"):
            f = "random:%d" % (int(f.split(":")[1]) * 7 + p if ":" in f else p)
        raws.append((p, pf.scanlines(data, hp, rb, unit, f)))
    if edit:
        raws = edit(raws)
    z = zlib.compress(b"".join(r for _, r in raws), level)
    if damage:
        z = damage(z)
    if plte is None and colour == 3:
        plte = pf.palette(min(256, 1 << depth))
    out = [pm.SIGNATURE, pf.ihdr(width, height, depth, colour, interlace=interlace)]
    if plte is not None:
        out.append(pf.chunk(b"PLTE", plte))
    if trns is not None:
        out.append(pf.chunk(b"tRNS", trns))
    out += [pf.chunk(t, d) for t, d in before]
    out += [pf.chunk(b"IDAT", part) for part in pf.split(z, idat)]
    out += [pf.chunk(t, d) for t, d in after]
    out += [pf.chunk(b"IEND"), tail]
    return pf.Png(b"".join(out), pixels, width, height, depth, colour)


def _row_bytes_of(width, height, depth, colour, p):
    for q, hp, rb, _ in pass_images(bytes(height * pm.rowbytes(width, depth, colour)), width,
                                    height, depth, colour):
        if q == p:
            return hp, rb
    raise ValueError("pass %d is absent" % p)


def defects7():
    """name -> (file bytes, the verdict of index_png_batch_ex with PNG_ADAM7,
    the verdict of its decode or None where there is no row to decode).  The
    image is 9 x 10 RGB8: all seven passes, raw7 = 290 against 10 * 28 = 280."""
    w, h, depth, colour = 9, 10, 8, 2
    out = {}

    def drop_last_row(raws):
        p, r = raws[-1]
        hp, rb = _row_bytes_of(w, h, depth, colour, p)
        return raws[:-1] + [(p, r[:-(rb + 1)])]

    def one_more_row(raws):
        p, r = raws[-1]
        hp, rb = _row_bytes_of(w, h, depth, colour, p)
        return raws[:-1] + [(p, r + r[-(rb + 1):])]

    def filter_byte(p, row):
        def edit(raws):
            hp, rb = _row_bytes_of(w, h, depth, colour, p)
            at = (row % hp) * (rb + 1)
            return [(q, r[:at] + b"\x05" + r[at + 1:]) if q == p else (q, r) for q, r in raws]
        return edit
    out["short_by_a_row"] = (make7(w, h, seed=11, edit=drop_last_row).data, pf.SUCCESS,
                             pf.SHORT_OUTPUT)
    out["one_row_too_many"] = (make7(w, h, seed=12, edit=one_more_row).data, pf.SUCCESS,
                               pf.INSUFFICIENT_SPACE)
    out["filter_5_pass3_first"] = (make7(w, h, seed=13, filters=0, edit=filter_byte(2, 0)).data,
                                   pf.SUCCESS, pf.BAD_DATA)
    out["filter_5_pass7_last"] = (make7(w, h, seed=14, filters=0, edit=filter_byte(6, -1)).data,
                                  pf.SUCCESS, pf.BAD_DATA)
    # the non-interlaced stream of the same image under an interlaced IHDR
    plain = pf.make(w, h, depth, colour, seed=15)
    out["plain_stream"] = (plain.data[:8] + pf.ihdr(w, h, depth, colour, interlace=1) +
                           plain.data[33:], pf.SUCCESS, pf.SHORT_OUTPUT)
    # raw7 is 3.5 * height at width 2, the image 3 * height: headers only
    big_h = 1300000000
    assert 3 * big_h < 1 << 32 <= 3 * big_h + big_h // 2
    out["raw7_2_32"] = (pm.SIGNATURE + pf.ihdr(2, big_h, 8, 0, interlace=1) +
                        pf.chunk(b"IDAT", b"x") + pf.chunk(b"IEND"), pf.UNSUPPORTED, None)
    data, verdict = pf.defects()["adam7_no_iend"]
    out["adam7_no_iend"] = (data, verdict, None)
    return out
