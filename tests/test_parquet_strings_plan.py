"""The host arithmetic that libdeflate_amd_parquet_decode_batch_ex adds
(csrc/parquet_strings_plan.h): every refusal with its row and reason, rows
without the BYTE_ARRAY bit planned as before, the walk sections, the start
lists' capacities, the two slot prefixes, the tile counts at their edges and the
tile-sum area, all against a serial model: tools/test_parquet_strings_plan.cpp,
a stand-alone program, built with the host compiler under the address and
undefined-behaviour sanitizers and run here.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parquet_strings_plan_against_its_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_parquet_strings_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_parquet_strings_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "parquet strings plan ok" in r.stdout
