#!/usr/bin/env python3
"""Regenerates tests/golden/tiff/: small deflate TIFFs written by Pillow
(libtiff) with compression="tiff_adobe_deflate", tag 317 (Predictor) and tag 278
(RowsPerStrip) set, each with its pixels as .npy.  8-bit L, RGB and RGBA with
predictors 1 and 2, 16-bit grey with predictor 2, float32 with predictors 2 and
3; widths 1, 53 and 300; one strip, and five strips with a short last one;
random walks and, per mode and predictor, one image of uniformly random
samples, so that the sums wrap.  The tests read the committed files: Pillow is
needed here only.

    python tools/gen_tiff_fixtures.py [--check]

--check writes nothing: it regenerates the pixels and compares them with the
committed .npy files, and opens the committed .tif files with Pillow."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tiff")

# (Pillow mode, channels, numpy dtype, predictors)
MODES = [("L", 1, np.uint8, (1, 2)), ("RGB", 3, np.uint8, (1, 2)), ("RGBA", 4, np.uint8, (1, 2)),
         ("I;16", 1, np.uint16, (2,)), ("F", 1, np.float32, (2, 3))]
# (width, height, rows per strip, content)
SHAPES = [(1, 7, 7, "walk"), (53, 23, 5, "walk"), (300, 11, 11, "walk"), (300, 14, 3, "walk"),
          (53, 23, 5, "rand")]


def name(mode, pred, w, h, rps, content):
    return "%s_p%d_w%d_h%d_rps%d_%s" % (mode.replace(";", "").lower(), pred, w, h, rps, content)


def pixels(mode, c, dtype, pred, w, h, rps, content):
    rng = np.random.default_rng([ord(ch) for ch in name(mode, pred, w, h, rps, content)])
    if content == "rand":
        raw = rng.integers(0, 256, size=h * w * c * np.dtype(dtype).itemsize, dtype=np.uint8)
        a = raw.view(dtype).reshape(h, w, c)
        if dtype is np.float32:         # (no NaN payloads that a library might not carry through)
            bits = a.view(np.uint32)
            bits[(bits & 0x7F800000) == 0x7F800000] &= 0xBFFFFFFF
            a = bits.view(np.float32)
    else:
        steps = rng.integers(-3, 4, size=(h, w, c))
        walk = 100 + np.cumsum(np.cumsum(steps, axis=1), axis=0) // 4
        a = (walk / 8.0).astype(np.float32) if dtype is np.float32 else walk.astype(dtype)
    return np.ascontiguousarray(a if c > 1 else a.reshape(h, w))


def cases():
    for mode, c, dtype, preds in MODES:
        for pred in preds:
            for w, h, rps, content in SHAPES:
                yield mode, c, dtype, pred, w, h, rps, content


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    for mode, c, dtype, pred, w, h, rps, content in cases():
        base = os.path.join(OUT, name(mode, pred, w, h, rps, content))
        a = pixels(mode, c, dtype, pred, w, h, rps, content)
        if args.check:
            assert np.array_equal(np.load(base + ".npy").view(np.uint8), a.view(np.uint8)), base
            with Image.open(base + ".tif") as im:
                got = np.asarray(im)
            assert got.tobytes() == a.tobytes(), base
            continue
        Image.fromarray(a).save(base + ".tif", compression="tiff_adobe_deflate",
                                tiffinfo={317: pred, 278: rps})
        np.save(base + ".npy", a)
        assert os.path.getsize(base + ".tif") <= 65536, base
    print("tiff fixtures %s: %d files" % ("checked" if args.check else "written",
                                          len(list(cases()))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
