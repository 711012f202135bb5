"""The chunks the OpenEXR tests share (tests/test_exr_read_gpu.py,
tests/test_exr_write_gpu.py, tests/test_exr_model.py): the shapes that aim at
the kernels' edges, their pixels, whole images through exr.assemble(), and the
fixture files of tests/golden/exr."""
import glob
import os

import numpy as np

from tools.models import exr_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "exr")

H, F = False, True      # a channel of 2-byte (HALF) and of 4-byte (FLOAT, UINT) samples
# the channel sets of the issue: 1, 3 and 4 HALF, 4 and 1 FLOAT, RGBA HALF + Z
# FLOAT (the file's order A, B, G, R, Z), and 5 and 16 channels for the generic path
FORMATS = [[H], [H, H, H], [H, H, H, H], [F, F, F, F], [F], [H, H, H, H, F], [H] * 5,
           [H, F, F, H, H, H, F, H, F, F, H, H, F, H, H, F]]
UNIFORM = [w for w in FORMATS if len(w) <= 4]

# raw sizes at the undo kernels' edges (exr_plan.h: a lane 32 bytes, a wave's
# tile 2048, a workgroup 4 tiles).  Every sample has 2 or 4 bytes, so a chunk's
# size is even: the even neighbours of the issue's 1, 3, 15, 17, 31, 33 and of
# tile +- 1 stand in for the odd ones, and sizes of 2 (mod 4) make the second
# half start at an odd place.
EDGE_SIZES = [2, 4, 6, 14, 16, 18, 30, 32, 34, 62, 64, 66,
              em.TILE - 2, em.TILE, em.TILE + 2,                # one wave's bytes
              2 * em.TILE - 2, 2 * em.TILE + 2, 3000,           # the first half ends inside a tile
              em.WG_TILES * em.TILE - 2, em.WG_TILES * em.TILE, em.WG_TILES * em.TILE + 2,
              3 * em.TILE + 6, 5 * em.TILE + 1022,              # carries across two and more boundaries
              37 * em.TILE + 10]                                # several workgroups


def fixtures():
    """[(name, the file's bytes, the pixels: height x width x pixel bytes, in
    the file's channel order)] of tests/golden/exr"""
    out = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, "*.exr"))):
        out.append((os.path.basename(f)[:-4], open(f, "rb").read(), np.load(f[:-4] + ".npy")))
    return out


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def few_bytes(seed, n):
    """bytes that deflate - long runs of very few values - and whose running
    sum is not zero"""
    rng = np.random.default_rng(seed)
    runs = rng.integers(0, 3, size=n // 24 + 1, dtype=np.uint8) * 5 + 3
    return np.repeat(runs, 24)[:n].tobytes()


class Chunk:
    """one chunk: wide - the channels; size (width, lines); layout, slots and
    the pitch's surplus `extra` on the pixel side; raw - the raw chunk, random
    or few-valued; stored - what a file holds for it (the model's decision)"""

    def __init__(self, wide, size, layout=em.LINES, slots=None, extra=0, few=False, seed=0,
                 level=6, head=()):
        self.wide, self.size, self.layout, self.extra, self.few = wide, size, layout, extra, few
        self.slots = slots if layout == em.PIXELS else None
        self.head = head
        self.lb = size[0] * sum(em.sizes_of(wide))
        self.n = self.lb * size[1]
        key = [seed, len(wide), size[0], size[1], int(few)]
        self.raw = few_bytes(key, self.n) if few else random_bytes(key, self.n)
        self.stored = em.data_of(self.raw, level)
        self.want, self.room = 0, "pixels"

    @property
    def pitch(self):
        return self.lb + self.extra

    def row(self, data_off, pix_off, data_n=None):
        return em.row(data_off, len(self.stored) if data_n is None else data_n, pix_off, self.pitch,
                      self.size, self.wide, self.layout, self.slots, self.head)

    def lines(self):
        """the lines on the pixel side"""
        return em.expected(self.row(0, 0), self.raw)


def reverse(wide):
    return list(range(len(wide) - 1, -1, -1))


def edge_chunks():
    """every edge size as one line of one HALF channel and, where it divides,
    as two lines, random (stored raw) and few-valued (a zlib stream), dealt
    round the layouts; then the cross of formats, lines, widths and layouts"""
    out, k = [], 0
    for n in EDGE_SIZES:
        for few in (False, True):
            lines = 2 if n % 4 == 0 and k % 3 == 0 else 1
            lay = k % 4
            out.append(Chunk([H], (n // 2 // lines, lines), em.PIXELS if lay == 3 else em.LINES,
                             [0], extra=(0, 5, 0, 3)[lay], few=few, seed=k))
            k += 1
    line_counts = [1, 2, 15, 16, 17]
    widths = [1, 7, 8, 9, 31, 32, 33, 64]
    for f, wide in enumerate(FORMATS):
        for j in range(10):
            lines, w = line_counts[(j + f) % 5], widths[(3 * j + f) % 8]
            lay = (j + f) % 4
            out.append(Chunk(wide, (w, lines), em.LINES if lay < 2 else em.PIXELS,
                             None if lay == 2 else reverse(wide), extra=(0, 7, 0, 16)[lay],
                             few=j % 2 == 1, seed=1000 + k))
            k += 1
    # tiles of 32 x 32 and 64 x 64 and their narrower edge tiles, RGBA half to pixels
    for w, lines in [(32, 32), (64, 64), (13, 32), (64, 5), (1, 64), (1, 1)]:
        for few in (False, True):
            out.append(Chunk([H] * 4, (w, lines), em.PIXELS, [3, 2, 1, 0], extra=24, few=few,
                             seed=2000 + k))
            k += 1
    return out


def image(width, height, channels, seed, smooth=True):
    """-> per-channel arrays (height x width, uint16 or uint32) of an image;
    smooth ones deflate"""
    rng = np.random.default_rng(seed)
    out = []
    for _, t in channels:
        dt = np.uint16 if t == 1 else np.uint32
        if smooth:
            a = (np.add.outer(np.arange(height), np.arange(width)) // 3 + rng.integers(0, 2, (height, width)))
            out.append(a.astype(dt) + dt(0x3C00))
        else:
            out.append(rng.integers(0, 1 << (16 if t == 1 else 32), (height, width)).astype(dt))
    return out


def raw_chunk(planes, x0, y0, w, lines):
    """the raw chunk of a region of an image: line by line, channel by channel"""
    return b"".join(p[y, x0:x0 + w].astype("<" + p.dtype.str[1:]).tobytes()
                    for y in range(y0, y0 + lines) for p in planes)


def interleaved(planes, order=None):
    """height x width x pixel bytes: the channels in `order` (indices; None: as given)"""
    idx = range(len(planes)) if order is None else order
    cols = [planes[k].astype("<" + planes[k].dtype.str[1:]).view(np.uint8).reshape(
        planes[k].shape[0], planes[k].shape[1], -1) for k in idx]
    return np.concatenate(cols, axis=2)


def image_file(width, height, channels, compression, tile=None, seed=0, smooth=True, level=6):
    """a whole file with Python's zlib and exr.assemble() -> (bytes, planes)"""
    from libdeflate_amd import exr
    planes = image(width, height, channels, seed, smooth)
    datas = []
    if tile:
        for y0 in range(0, height, tile[1]):
            for x0 in range(0, width, tile[0]):
                raw = raw_chunk(planes, x0, y0, min(tile[0], width - x0), min(tile[1], height - y0))
                datas.append(em.data_of(raw, level) if compression else raw)
    else:
        per = exr.LINES_PER_CHUNK[compression]
        for y0 in range(0, height, per):
            raw = raw_chunk(planes, 0, y0, width, min(per, height - y0))
            datas.append(em.data_of(raw, level) if compression else raw)
    return exr.assemble(width, height, channels, compression, datas, tile), planes
