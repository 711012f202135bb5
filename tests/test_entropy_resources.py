"""The entropy stage's kernels as the compiler reports them: no spilled VGPRs,
and the waves per SIMD - workgroups per CU, at one wave per SIMD per 256-thread
workgroup - that the kernel's __launch_bounds__ asks for, which is what the
static_assert on the LDS block is written against.  The stage is one file and
one kernel (deflate_entropy.hip: lda_deflate_entropy_kernel); a file added to
it has to be named here and in the Makefile's NOLICM list, the flag the
compress kernels' register counts depend on.  The report of the compile
itself, with the Makefile's flags for the object; no GPU needed."""
import glob
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(__file__), "..", "libdeflate_amd", "csrc")
STAGE = {"deflate_entropy.hip": ["lda_deflate_entropy_kernel"]}


def test_entropy_stage_files_are_known_and_built_without_machine_licm():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    nolicm = re.search(r"^NOLICM \?= (.*)$", mk, re.M).group(1).split()
    found = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.hip"))
                   if re.search(r"define\s+LDA_ENTROPY\b", open(f).read()))
    assert found == sorted(STAGE)
    for f in STAGE:
        assert f[:-4] in nolicm, f


@pytest.mark.parametrize("src", sorted(STAGE))
def test_entropy_stage_kernels_fit_their_launch_bounds(src):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    text = open(os.path.join(CSRC, src)).read()
    wgs = int(re.search(r"^#define ENTROPY_WGS (\d+)", text, re.M).group(1))
    assert re.search(r"__launch_bounds__\(NT, ENTROPY_WGS\)", text)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off", "-mllvm",
                        "-disable-machine-licm", "-Rpass-analysis=kernel-resource-usage",
                        "--cuda-device-only", "-c", src, "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = r.stderr
    assert re.findall(r"Function Name: (lda_\w+)", rep) == STAGE[src]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", rep)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", rep)]
    occ = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", rep)]
    assert spills == [0] * len(STAGE[src]), spills
    assert scratch == [0] * len(STAGE[src]), scratch
    assert occ == [wgs] * len(STAGE[src]), occ
