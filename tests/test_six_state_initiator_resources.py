"""CPU (cross-compile only): the six-state build (-DMHT_NX=6, libmht_amd6.so) carries the 4-state device initiator and the admission that
lifts its births into the forest's state space (mht_initiator_set_lift, csrc/mht_admit.h: AddArgs::lift).  The kernels that run them there
keep the budgets of their 4-state twins (tests/test_kernel_resources.py: BUDGET), and both libraries export the new entry point."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymht_amd", "csrc")

# kernel -> (max scratch bytes per lane, max VGPRs[, max spilled VGPRs]) in the six-state build; every instance whose name matches is checked
BUDGET6_INIT = {
    "mht_cluster.hip": {"cluster_init_kernel": (288, 128, 0)},
    "mht_forest.hip": {"commit_kernel": (0, 128), "add_targets_kernel": (0, 128), "post_scan_kernelILb0": (288, 128, 0),
                       "post_scan_kernelILb1": (288, 128, 0), "initiator_side_kernel": (288, 128, 0)},
    "mht_init.hip": {"initiator_kernel": (288, 128, 0)},
}


def _report(src, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from pymht_amd.build import FLAGS
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [hipcc] + flags + ["-DMHT_NX=6", "-c", "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"),
                             os.path.join(CSRC, src), "-o", str(tmp_path / "o.o")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stderr
    found = {}
    for m in re.finditer(r"Function Name: (\S+)", text):
        seg = text[m.end():m.end() + 4000]
        nxt = seg.find("Function Name:")
        seg = seg if nxt < 0 else seg[:nxt]
        found[m.group(1)] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", seg).group(1)),
                             int(re.search(r"VGPRs: (\d+)", seg).group(1)),
                             int(re.search(r"VGPRs Spill: (\d+)", seg).group(1)))
    return found


@pytest.mark.parametrize("src", sorted(BUDGET6_INIT))
def test_initiator_and_admission_kernels_within_budget_six_state_build(src, tmp_path):
    found = _report(src, tmp_path)
    for kern, budget in BUDGET6_INIT[src].items():
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert hits, "kernel %s not found in the compiler report of %s (-DMHT_NX=6)" % (kern, src)
        for name, (scratch, vgpr, spill) in hits:
            if len(budget) > 2:
                assert spill <= budget[2], "%s (six-state build) spills %d VGPRs (budget %d)" % (name, spill, budget[2])
            assert scratch <= budget[0], "%s (six-state build) uses %d B of scratch per lane (budget %d)" % (name, scratch, budget[0])
            assert vgpr <= budget[1], "%s (six-state build) needs %d VGPRs (budget %d)" % (name, vgpr, budget[1])


def test_set_lift_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    assert "mht_initiator_set_lift" in _lib.exported_symbols()
    for nx in (4, 6):
        assert hasattr(_lib.load(nx=nx), "mht_initiator_set_lift"), "the %d-state build does not export mht_initiator_set_lift" % nx
