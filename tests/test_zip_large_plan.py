"""The host arithmetic of libdeflate_amd_zip_read_large (csrc/zip_large_plan.h):
which entries go to the many-wave decoder, the piece tables, what is left of
the sibling's columns and every refusal, against a plain serial model for
pieces of 1, 7 and 4096 bytes, three values of large_min and every alignment:
tools/test_zip_large_plan.cpp, a stand-alone program, built with the host
compiler under the address and undefined-behaviour sanitizers and run here.
No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_zip_large_plan_against_its_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_zip_large_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_zip_large_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "zip large plan ok" in r.stdout
