"""The host arithmetic of libdeflate_amd_gzip_members_compress_batch
(csrc/gzip_members_write_plan.h): the bound, every refusal, and the plan's
columns against a plain model - records of 0, 1, 131 071 / 131 072 / 131 073,
4 MiB +- 1, 8 MiB +- 1 and just below 4 GiB, with and without names, pieces
that tile their record, primes that never reach in front of it, slots that
never overlap and hold the compressor's bound, launch groups that cover every
piece once: tools/test_gzip_members_write_plan.cpp, a stand-alone program,
built with the host compiler under the address and undefined-behaviour
sanitizers and run here.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gzip_members_write_plan_against_its_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_gzip_members_write_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_gzip_members_write_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "gzip members write plan ok" in r.stdout
