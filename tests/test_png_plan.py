"""The host arithmetic of libdeflate_amd_png_out_sizes and
libdeflate_amd_png_decode_batch (csrc/png_plan.h): rowbytes, filter unit and
channels of all 15 depth and colour pairs, overflowing products (width = height
= 2^31 - 1, 16-bit RGBA), every refusal of an index row and of a selection, and
the rooms and descriptor columns of selections with duplicates against a serial
model, for every alignment: tools/test_png_plan.cpp, a stand-alone program,
built with the host compiler under the address and undefined-behaviour
sanitizers and run here.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_png_plan_against_its_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_png_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_png_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "png plan ok" in r.stdout
