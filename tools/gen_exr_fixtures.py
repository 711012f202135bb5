#!/usr/bin/env python3
"""Regenerates tests/golden/exr/: small OpenEXR files written by
libdeflate_amd/exr.py's assemble() with Python's zlib and the CPU model of the
chunk coding (tools/models/exr_model.py), each with its pixels - height x width
x pixel bytes, the channels in the file's order - as .npy.  Scanline ZIP, ZIPS
and NONE and tiled ZIP; RGBA half, RGBA half + Z float, one float channel;
smooth images, whose chunks are zlib streams, and one of random samples, whose
chunks a writer must store raw.

No OpenEXR implementation was at hand: these files pin the parser and the model
against regressions.  They do NOT pin the format against the OpenEXR library.

    python tools/gen_exr_fixtures.py [--check]

--check writes nothing: it regenerates files and pixels and compares them with
the committed ones."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "exr")

RGBA = [("A", 1), ("B", 1), ("G", 1), ("R", 1)]
# (name, width, height, channels, compression, tile, smooth)
CASES = [("rgba_zip_w70_h37", 70, 37, RGBA, 3, None, True),
         ("rgba_zips_w33_h5", 33, 5, RGBA, 2, None, True),
         ("rgba_none_w17_h3", 17, 3, RGBA, 0, None, True),
         ("rgba_zip_tiles32_w70_h40", 70, 40, RGBA, 3, (32, 32), True),
         ("rgbaz_zip_w41_h18", 41, 18, RGBA + [("Z", 2)], 3, None, True),
         ("y_float_zip_tiles16_w20_h20", 20, 20, [("Y", 2)], 3, (16, 16), True),
         ("rgba_zip_w24_h16_rand", 24, 16, RGBA, 3, None, False),
         ("rgba_zips_w1_h2", 1, 2, RGBA, 2, None, True)]


def main():
    from tests import exr_chunks as ec
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    for k, (name, w, h, channels, comp, tile, smooth) in enumerate(CASES):
        base = os.path.join(OUT, name)
        data, planes = ec.image_file(w, h, channels, comp, tile, seed=[77, k], smooth=smooth)
        pixels = ec.interleaved(planes)
        if args.check:
            assert open(base + ".exr", "rb").read() == data, base
            assert np.array_equal(np.load(base + ".npy"), pixels), base
            continue
        with open(base + ".exr", "wb") as f:
            f.write(data)
        np.save(base + ".npy", pixels)
        assert len(data) <= 16384, (base, len(data))
    print("exr fixtures %s: %d files" % ("checked" if args.check else "written", len(CASES)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
