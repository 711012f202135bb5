"""The walk over a run of stored blocks (csrc/stored_rows.h) finds the same
chunks, results and stop position in the rows that describe a stream in device
memory as in the stream's bytes: tools/test_stored_rows.cpp, a stand-alone
program, built with the host compiler under the address and undefined-behaviour
sanitizers and run here.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_walk_equals_byte_walk(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_stored_rows")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_stored_rows.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "stored rows ok" in r.stdout
