"""The PNG reader's decode to one pixel format on the CPU
(libdeflate_amd_png_pixels_out_sizes / _png_decode_pixels_batch,
include/libdeflate_amd.h): png_model.decode followed by the five steps of the
header - the samples at the file's depth, the palette with its tRNS alphas, the
colour key, the depth, the channels - vectorised with numpy.  The GPU tests
compare every result and every pixel byte with this;
tests/test_png_pixels_model.py pins it against hand-written vectors and PIL."""
import numpy as np

from tools.models import png_model as pm

SUCCESS, BAD_DATA, UNSUPPORTED = pm.SUCCESS, pm.BAD_DATA, pm.UNSUPPORTED
GRAY, GRAY_ALPHA, RGB, RGBA, OUT16 = 1, 2, 3, 4, 0x10
LE16 = pm.LE16
TILE = 4096     # pixels of a tile of the convert kernel
FORMATS = [c | o for o in (0, OUT16) for c in (GRAY, GRAY_ALPHA, RGB, RGBA)]
_MASK48 = (1 << 48) - 1


def format_ok(fmt):
    return 1 <= (fmt & 0xF) <= 4 and not fmt & ~(0xF | OUT16)


def fmt_channels(fmt):
    return fmt & 0xF


def fmt_depth(fmt):
    return 16 if fmt & OUT16 else 8


def is_direct(depth, colour, fmt):
    """the file already stores the format: the unfilter writes the room"""
    return colour != 3 and depth == fmt_depth(fmt) and pm.CHANNELS[colour] == fmt_channels(fmt)


def out_bytes(row, fmt):
    h, w = row[2] >> 32, row[2] & 0xFFFFFFFF
    return h * w * fmt_channels(fmt) * (fmt_depth(fmt) // 8)


def out_sizes(rows, sel, fmt, align=1):
    """-> the n_sel + 1 offsets of a selection in the output"""
    at, offs = 0, []
    for k in sel:
        offs.append(at)
        if not pm.is_zero(rows[k]):
            at += (out_bytes(rows[k], fmt) + align - 1) // align * align
    return offs + [at]


def shapes(rows, fmt):
    """((H, W, C) per row - zeros for a zero row -, the numpy dtype name)"""
    ch = fmt_channels(fmt)
    return ([(0, 0, 0) if pm.is_zero(r) else (r[2] >> 32, r[2] & 0xFFFFFFFF, ch) for r in rows],
            "uint16" if fmt & OUT16 else "uint8")


def samples(pixels, width, height, depth, colour):
    """step 1: the samples at the file's depth -> uint32 (H, W, channels);
    depths 1, 2, 4 most-significant-bit first, a row's spare bits dropped"""
    ch = pm.CHANNELS[colour]
    rb = pm.rowbytes(width, depth, colour)
    a = np.frombuffer(pixels, dtype=np.uint8).reshape(height, rb)
    if depth == 16:
        s = a.view(">u2")
    elif depth == 8:
        s = a
    else:
        bits = np.unpackbits(a, axis=1)[:, :width * depth].reshape(height, width, depth)
        s = (bits.astype(np.uint32) << np.arange(depth - 1, -1, -1, dtype=np.uint32)).sum(axis=2)
    return s.astype(np.uint32).reshape(height, width, ch)


def scale(v, depth, out_depth):
    """step 4: bit replication upwards, round to nearest downwards"""
    v = v.astype(np.uint32)
    if depth < 8:
        v = v * {1: 0xFF, 2: 0x55, 4: 0x11}[depth]
        depth = 8
    if depth == 8 and out_depth == 16:
        return v * 257
    if depth == 16 and out_depth == 8:
        return (v * 255 + 32895) >> 16
    return v


def gray_of(r, g, b):
    """step 5, RGB -> grey; the coefficients sum to 65536"""
    return (19595 * r.astype(np.uint32) + 38470 * g.astype(np.uint32) +
            7471 * b.astype(np.uint32) + 32768) >> 16


def convert(pixels, width, height, depth, colour, fmt, plte=None, trns=None, flags=0):
    """The pixel bytes png_model.decode returns (PNG order) -> (result, bytes in
    the format).  plte: the PLTE chunk's data; trns: the tRNS chunk's data, or
    None where the index row's word 7 is 0."""
    s = samples(pixels, width, height, depth, colour)
    res = SUCCESS
    if colour == 3:
        entries = len(plte) // 3
        table = np.zeros((256, 4), dtype=np.uint32)
        table[:entries, :3] = np.frombuffer(plte, dtype=np.uint8)[:3 * entries].reshape(-1, 3)
        table[:entries, 3] = 255
        if trns is not None:
            n = min(len(trns), entries)
            table[:n, 3] = np.frombuffer(trns, dtype=np.uint8)[:n]
        idx = s[:, :, 0]
        if (idx >= entries).any():
            return BAD_DATA, None
        rgba = table[idx]
        depth = 8
    else:
        maxv = (1 << depth) - 1
        alpha = np.full((height, width), maxv, dtype=np.uint32)
        if colour == 0 and trns is not None and len(trns) == 2:
            key = int.from_bytes(trns, "big") & maxv
            alpha[s[:, :, 0] == key] = 0
        elif colour == 2 and trns is not None and len(trns) == 6:
            key = np.array([int.from_bytes(trns[2 * k:2 * k + 2], "big") & maxv for k in range(3)],
                           dtype=np.uint32)
            alpha[(s == key).all(axis=2)] = 0
        if colour in (4, 6):
            alpha = s[:, :, -1]
        colours = s[:, :, :3] if colour in (2, 6) else np.repeat(s[:, :, :1], 3, axis=2)
        rgba = np.concatenate([colours, alpha[:, :, None]], axis=2)
    rgba = scale(rgba, depth, fmt_depth(fmt))
    ch = fmt_channels(fmt)
    if ch <= 2:
        grey = gray_of(rgba[:, :, 0], rgba[:, :, 1], rgba[:, :, 2])
        out = np.stack([grey, rgba[:, :, 3]], axis=2)[:, :, :ch]
    else:
        out = rgba[:, :, :ch]
    if fmt & OUT16:
        return res, out.astype("<u2" if flags & LE16 else ">u2").tobytes()
    return res, out.astype(np.uint8).tobytes()


def chunks_of(buf, row):
    """(PLTE data or None, tRNS data or None) as the row's words 6 and 7 name them"""
    plte = trns = None
    if row[6]:
        off, n = row[6] & _MASK48, row[6] >> 48
        plte = bytes(buf[off:off + 3 * n])
    if row[7]:
        off, n = row[7] & _MASK48, row[7] >> 48
        trns = bytes(buf[off:off + n])
    return plte, trns


def decode(buf, row, fmt, flags=0):
    """One selection -> (result, the bytes in the format or None): the first of
    png_model.decode's verdicts, BAD_DATA for a palette index out of range,
    SUCCESS."""
    res, pixels = pm.decode(buf, row, 0)
    if res != SUCCESS:
        return res, None
    h, w, _, depth, colour = pm.shape(row)
    plte, trns = chunks_of(buf, row)
    return convert(pixels, w, h, depth, colour, fmt, plte, trns, flags)
