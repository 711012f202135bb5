"""The host arithmetic of the many-wave single-stream decoder
(csrc/stream_plan.h): the planner's chunk starts and limits, the chain (walk,
repairs under doubling, phase groups and phase candidates, chunks under the
static codes, runs of stored blocks, every refusal) driven by a model of the
count kernel, and one_length_code() on hand-written dynamic headers:
tools/test_stream_plan.cpp, a stand-alone program, built with the host
compiler under the address and undefined-behaviour sanitizers and run here.
No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_plan_against_its_models(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "test_stream_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libdeflate_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "test_stream_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert r.stdout.strip().splitlines()[-1] == "stream plan ok"
