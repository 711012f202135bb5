"""The host arithmetic of libdeflate_amd_png_out_sizes_ex and
libdeflate_amd_png_decode_batch_ex (csrc/png_adam7_plan.h): the geometry of the
seven Adam7 passes against a walk over the pixel grid for all widths and
heights in 1 .. 17, raw7 and its 2^32 edge in 128-bit arithmetic, every refusal
with and without the flag, and the units, scratch rooms, convert and deinterlace
columns of mixed selections with duplicates against a serial model for every
alignment and format: tools/test_png_adam7_plan.cpp, a stand-alone program,
built with the host compiler under the address and undefined-behaviour
sanitizers and run here.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_png_adam7_plan_against_its_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_png_adam7_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_png_adam7_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "png adam7 plan ok" in r.stdout
