"""The host arithmetic of libdeflate_amd_png_encode_bound and
libdeflate_amd_png_encode_batch (csrc/png_write_plan.h): every refusal with its
reason, the bound, the overflowing products (width = height = 2^31 - 1, 16-bit
RGBA) in 128-bit arithmetic, the rooms, group classes and work list against a
serial model, and the piece columns equal to zipw_cut_pieces() called directly:
tools/test_png_write_plan.cpp, a stand-alone program, built with the host
compiler under the address and undefined-behaviour sanitizers and run here.
No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_png_write_plan_against_its_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_png_write_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_png_write_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "png write plan ok" in r.stdout
