"""The per-level instances of the LZ77 stage (deflate_l1.hip ... deflate_l9.hip:
deflate_kernel.hip with one level's search depth, nice length and parse mode as
constants) exist to take instructions and spilled scalar registers out of a
kernel that is bound by instruction issue.  The report and the assembly of the
compile itself, with the Makefile's flags for each object, against the generic
kernel of the same build: no instance spills vector registers or uses scratch,
none has more VGPRs or more spilled SGPRs than the generic kernel, and the
level-6 and level-1 instances have fewer instructions.  No GPU needed."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "libdeflate_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LEVELS = tuple(range(1, 10))
GENERIC = "lda_deflate_batch_kernel"


def _flags(obj):
    """the Makefile's flags for obj.o (the instances must be on both lists)"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = []
    if obj in re.search(r"^NOLICM \?= (.*)$", mk, re.M).group(1).split():
        flags += ["-mllvm", "-disable-machine-licm"]
    if obj in re.search(r"^MAXILP \?= (.*)$", mk, re.M).group(1).split():
        sched = re.search(r"^SCHED  \?= (\S+)$", mk, re.M).group(1)
        flags += ["-mllvm", f"-amdgpu-sched-strategy={sched}"]
    return flags


def _compile(obj):
    """obj.hip -> {kernel: dict(vgprs, sgpr_spill, vgpr_spill, scratch, insts)}"""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fvisibility=hidden", "-ffp-contract=off", *_flags(obj),
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        obj + ".hip", "-o", "-"],
                       cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]

        def num(key, blk=blk):
            return int(re.search(r"remark:\s+%s: (\d+)" % re.escape(key), blk).group(1))
        out[name] = {"vgprs": num("VGPRs"), "sgpr_spill": num("SGPRs Spill"),
                     "vgpr_spill": num("VGPRs Spill"), "scratch": num("ScratchSize [bytes/lane]")}
    for name in out:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), r.stdout, re.M | re.S)
        assert m, name
        out[name]["insts"] = sum(1 for l in m.group(1).splitlines()
                                 if l.startswith("\t") and not l.lstrip().startswith((".", ";")))
    return out


@pytest.fixture(scope="module")
def reports():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    objs = ["deflate_kernel"] + [f"deflate_l{n}" for n in LEVELS]
    with ThreadPoolExecutor(max_workers=min(len(objs), os.cpu_count() or 1, 10)) as ex:
        reps = list(ex.map(_compile, objs))
    return dict(zip(objs, reps))


def test_instances_are_built_like_the_generic_kernel():
    assert _flags("deflate_kernel"), "the Makefile's lists were not read"
    for n in LEVELS:
        assert _flags(f"deflate_l{n}") == _flags("deflate_kernel"), n


def test_every_instance_is_one_kernel_without_vector_spills(reports):
    for n in LEVELS:
        rep = reports[f"deflate_l{n}"]
        kernels = [k for k in rep if k.startswith("lda_")]
        assert kernels == [f"{GENERIC}_l{n}"], kernels
        k = rep[kernels[0]]
        print(n, k)
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0, (n, k)


def test_no_instance_needs_more_registers_than_the_generic_kernel(reports):
    g = reports["deflate_kernel"][GENERIC]
    print("generic", g)
    for n in LEVELS:
        k = reports[f"deflate_l{n}"][f"{GENERIC}_l{n}"]
        assert k["vgprs"] <= g["vgprs"], (n, k, g)
        assert k["sgpr_spill"] <= g["sgpr_spill"], (n, k, g)


@pytest.mark.parametrize("level", [6, 1])
def test_instance_has_fewer_instructions(reports, level):
    g = reports["deflate_kernel"][GENERIC]
    k = reports[f"deflate_l{level}"][f"{GENERIC}_l{level}"]
    print(level, k["insts"], g["insts"])
    assert k["insts"] < g["insts"], (level, k, g)
