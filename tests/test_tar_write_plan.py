"""The host arithmetic of libdeflate_amd_tar_write_batch and
libdeflate_amd_targz_compress_batch (csrc/tar_write_plan.h): every refusal, one
case per cause, the UTF-8 check and the self-counting length of the pax record,
and the entries' offsets, the archive's size and the index rows against a plain
serial model - entry sizes 0 and 8^11 - 1 and archives whose end blocks just
fit or just spill into another 10 240-byte record included:
tools/test_tar_write_plan.cpp, a stand-alone program, built with the host
compiler under the address and undefined-behaviour sanitizers and run here.
No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tar_write_plan_against_its_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_tar_write_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_tar_write_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "tar write plan ok" in r.stdout
