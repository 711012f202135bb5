"""The segments the TIFF tests share (tests/test_tiff_read_gpu.py,
tests/test_tiff_write_gpu.py): the shapes that aim at the unpredict kernel's
edges, their pixels, and the fixture files of tests/golden/tiff."""
import glob
import os

import numpy as np

from tools.models import tiff_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff")

# (spp, bps): every pixel size the kernel keeps in registers ...
REG_FORMATS = [(1, 1), (2, 1), (1, 2), (4, 1), (2, 2), (1, 4), (8, 1), (4, 2), (2, 4), (1, 8),
               (16, 1), (8, 2), (4, 4), (2, 8), (3, 1), (6, 1), (3, 2), (12, 1), (6, 2), (3, 4),
               (12, 2), (6, 4), (3, 8), (12, 4), (6, 8)]
# ... and sizes that take the generic path
GENERIC_FORMATS = [(5, 1), (7, 1), (5, 2), (5, 4), (16, 8), (9, 2)]


def fixtures():
    """[(name, the file's bytes, the pixels' bytes)] of tests/golden/tiff"""
    out = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, "*.tif"))):
        out.append((os.path.basename(f)[:-4], open(f, "rb").read(),
                    np.load(f[:-4] + ".npy").tobytes()))
    return out


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def widths(spp, bps, pred):
    """coded widths whose scanned row bytes sit at the group sizes' and the
    passes' edges: 1 pixel, 15 / 16 / 17 bytes, G * piece - 1, G * piece,
    G * piece + 1 for G 4, 16 and 64, and two passes plus one pixel"""
    px = spp * bps
    st = spp if pred == 3 else px
    piece = tm.lane_bytes(st)
    targets = [1, 15, 16, 17, 128 * piece + px]
    for g in (4, 16, 64):
        targets += [g * piece - 1, g * piece, g * piece + 1]
    # predictor 3 scans the coded row's bytes, bps planes of width * spp
    return sorted({max(1, (t + px - 1) // px) for t in targets} | {max(1, t // px) for t in targets})


def shapes():
    """[(spp, bps, predictor, coded (w, r), kept (w, r), extra pitch)]: the
    cross of formats, predictors and widths, with rows 1, 2, 63, 64, 65, kept
    smaller than coded in width, in rows and in both, and pitches larger than
    the row, dealt round"""
    out, k = [], 0
    for spp, bps in REG_FORMATS + GENERIC_FORMATS:
        for pred in (2, 3) if bps > 1 else (2,):
            for w in widths(spp, bps, pred):
                rb = w * spp * bps
                r = (1, 2, 3, 63, 64, 65)[k % 6] if rb <= 1100 else (1, 2, 3)[k % 3]
                crop = (k // 2) % 4
                kw = max(1, w - 1 - k % 3) if crop in (1, 3) else w
                kr = max(1, r - 1) if crop in (2, 3) else r
                out.append((spp, bps, pred, (w, r), (kw, kr), (0, 0, 5, 16, 1)[k % 5]))
                k += 1
    # predictor 1 that is not direct: cropped, or at a pitch of its own
    out += [(3, 1, 1, (40, 5), (33, 4), 0), (1, 2, 1, (700, 3), (700, 3), 7),
            (4, 4, 1, (9, 70), (9, 70), 1), (2, 8, 1, (100, 2), (1, 2), 3)]
    return out
