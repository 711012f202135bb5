"""The host arithmetic of a compress batch call (csrc/compress_plan.h): which
kernel a batch takes, its scratch-limited slices, the layout of the kernels'
scratch, and the cut of a slice into a head and a tail, against a plain serial
model for 1, 8, 256 and 304 CUs, tails of 0, 1, 2 and 4 buffers per CU, five
size bounds and every batch size around each threshold:
tools/test_compress_plan.cpp, a stand-alone program, built with the host
compiler under the address and undefined-behaviour sanitizers and run here.
No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compress_plan_against_its_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_compress_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_compress_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "compress plan ok" in r.stdout
