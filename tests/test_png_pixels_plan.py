"""The host arithmetic of libdeflate_amd_png_pixels_out_sizes and
libdeflate_amd_png_decode_pixels_batch (csrc/png_pixels_plan.h): the direct /
converted decision of all 15 depth and colour pairs x 8 formats x tRNS present
or absent against a table, sizes with overflowing products in 128-bit
arithmetic, the rooms, the three scratch areas, the converted selections'
columns and the tile prefix against a serial model for every alignment, and
every refusal:
tools/test_png_pixels_plan.cpp, a stand-alone program, built with the host
compiler under the address and undefined-behaviour sanitizers and run here.
No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_png_pixels_plan_against_its_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_png_pixels_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_png_pixels_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "png pixels plan ok" in r.stdout
