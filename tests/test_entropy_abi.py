"""The entropy kernel (deflate_entropy.hip) keeps its register budget: four
256-thread workgroups per CU (__launch_bounds__(256, 4)) leave 128 VGPRs, and
what deflate_blockend.h gains must not make it spill or drop below that.  The
report of the compile itself, with the Makefile's flags for the object; no GPU
needed."""
import os
import re
import subprocess

import pytest


def test_entropy_kernel_keeps_its_register_budget():
    csrc = os.path.join(os.path.dirname(__file__), "..", "libdeflate_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^NOLICM \?= .*\bdeflate_entropy\b", mk, re.M)
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off", "-mllvm",
                        "-disable-machine-licm", "-Rpass-analysis=kernel-resource-usage",
                        "--cuda-device-only", "-c", "deflate_entropy.hip", "-o", os.devnull],
                       cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_deflate_\w+)", rep) == ["lda_deflate_entropy_kernel"]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", rep)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", rep)]
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", rep)]
    assert vgprs and max(vgprs) <= 128, vgprs      # round 7: 113
    assert spills == [0], spills
    assert occ and min(occ) >= 4, occ
