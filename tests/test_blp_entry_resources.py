"""CPU (cross-compile only): what the two instances of the union-find ILP launch cost in registers, from the compiler's own resource
remarks (as tests/test_kernel_resources.py reads them).

blp_uf_kernel used to copy its whole argument block at entry and keep the block's ~130 pointers alive through the kernel: at one wavefront
per SIMD every one of them lived in a VGPR lane ("SGPRs Spill") and every use was a lane move on the scan's critical path.  Both instances
now read the block from the argument segment where they use it; the plain instance (a plain forest's switches compiled in) must need fewer
spilled scalars than the generic one, and the generic one no more than it did before the arguments were read lazily."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymht_amd", "csrc")

# "SGPRs Spill" of blp_uf_kernel at the commit before the lazy argument reads, with AMD clang 22.0.0git (roc-7.2.0, HIP 7.2.26015)
PARENT_SGPR_SPILL = 765


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from pymht_amd.build import FLAGS
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC")]
    out = subprocess.run([hipcc] + flags + ["-c", "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"),
                                            os.path.join(CSRC, "mht_blp.hip"), "-o", str(tmp_path_factory.mktemp("blp") / "o.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stderr
    found = {}
    for m in re.finditer(r"Function Name: (\S+)", text):
        seg = text[m.end():m.end() + 4000]
        nxt = seg.find("Function Name:")
        seg = seg if nxt < 0 else seg[:nxt]
        found[m.group(1)] = {key: int(re.search(re.escape(key) + r": (\d+)", seg).group(1))
                             for key in ("ScratchSize [bytes/lane]", "VGPRs", "SGPRs Spill", "VGPRs Spill")}
    return found


def _instances(found):
    generic = [v for k, v in found.items() if "blp_uf_kernel" in k and "plain" not in k]
    plain = [v for k, v in found.items() if "blp_uf_kernel_plain" in k]
    assert len(generic) == 1 and len(plain) == 1, sorted(found)
    return generic[0], plain[0]


def test_both_instances_without_scratch(remarks):
    for r in _instances(remarks):
        assert r["ScratchSize [bytes/lane]"] == 0, r
        assert r["VGPRs"] <= 256, r


def test_plain_instance_spills_fewer_scalars_than_the_generic_one(remarks):
    """AMD clang 22.0.0git (roc-7.2.0): generic 443, plain 339 spilled SGPRs (parent commit: 765).  What separates the two once neither keeps
    the argument block alive: the plain instance's LDS capacities are compile-time constants, so the solver's ~30 table addresses are a
    base plus a literal folded into the access; the generic instance keeps one scalar per table through the whole solve."""
    generic, plain = _instances(remarks)
    print("SGPRs Spill: generic %d, plain %d (parent commit %d)" % (generic["SGPRs Spill"], plain["SGPRs Spill"], PARENT_SGPR_SPILL))
    assert plain["SGPRs Spill"] < generic["SGPRs Spill"], (plain, generic)


def test_generic_instance_spills_no_more_scalars_than_before(remarks):
    generic, _ = _instances(remarks)
    assert generic["SGPRs Spill"] <= PARENT_SGPR_SPILL, generic
