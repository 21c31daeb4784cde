"""CPU (cross-compile only): the grow kernel of AIS forests with N-scan windows of 8..12 (fgrow_ais_kernel<8>: 32-int path / ancestor
records) within the budget of the other fgrow_ais_kernel instances -- <= 256 VGPRs (two workgroups per CU), <= 512 B of scratch per lane,
and no more spilled VGPRs than fgrow_ais_kernel<4>.  test_kernel_resources.py checks only the first instance whose name matches."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymht_amd", "csrc")


def _report(src, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from pymht_amd.build import FLAGS
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [hipcc] + flags + ["-c", "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, src),
                             "-o", str(tmp_path / "o.o")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stderr
    found = {}
    for m in re.finditer(r"Function Name: (\S+)", text):
        seg = text[m.end():m.end() + 4000]
        nxt = seg.find("Function Name:")
        seg = seg if nxt < 0 else seg[:nxt]
        found[m.group(1)] = dict(scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", seg).group(1)),
                                 vgpr=int(re.search(r"VGPRs: (\d+)", seg).group(1)),
                                 vspill=int(re.search(r"VGPRs Spill: (\d+)", seg).group(1)))
    return found


def _instance(found, pq):
    hits = [v for k, v in found.items() if "fgrow_ais_kernelILi%dE" % pq in k]
    assert len(hits) == 1, "fgrow_ais_kernel<%d>: %d instances in the compiler report" % (pq, len(hits))
    return hits[0]


def test_fgrow_ais_kernel_for_long_windows_within_budget(tmp_path):
    found = _report("mht_fgrow.hip", tmp_path)
    r4, r8 = _instance(found, 4), _instance(found, 8)
    assert r8["scratch"] <= 512, "fgrow_ais_kernel<8> uses %d B of scratch per lane (budget 512)" % r8["scratch"]
    assert r8["vgpr"] <= 256, "fgrow_ais_kernel<8> needs %d VGPRs (budget 256)" % r8["vgpr"]
    assert r8["vspill"] <= r4["vspill"], "fgrow_ais_kernel<8> spills %d VGPRs, <4> %d" % (r8["vspill"], r4["vspill"])
