"""CPU (cross-compile only): the AIS-aware smoother's kernels (csrc/mht_smooth_ais.hip: smooth_ais_kernel<COV>, with and without the
covariance recursion) in both code objects, held to what tests/test_smooth_resources.py asks of the linear ones.  A leg's matrices are
per-lane (26 doubles in vector registers where the plain step's sit in scalar ones) and an AIS node's backward step is two steps inlined:
neither may push a matrix into scratch.  Figures as read from the compiled objects.  Plus the seam's exports and its workspace size."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymht_amd", "csrc")

# instance -> (VGPRs, AGPRs) the compiler reports (identical in the two builds: the kernels do not depend on MHT_NX); the assertion is
# "no more than this", plus: no scratch, no spill, no LDS, and VGPRs + AGPRs within the 512 entries one wavefront per SIMD can have
READ = {
    "smooth_ais_kernelILb1E": (238, 0),
    "smooth_ais_kernelILb0E": (215, 0),
}


def _report(tmp_path, extra):
    """tests/test_smooth_resources.py::_report for mht_smooth_ais.hip."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from pymht_amd.build import FLAGS, SOURCES
    assert "mht_smooth_ais.hip" in SOURCES, "the AIS-aware smoother is not part of the library"
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [hipcc] + flags + list(extra) + ["-c", "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"),
                                           os.path.join(CSRC, "mht_smooth_ais.hip"), "-o", str(tmp_path / "o.o")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stderr
    found = {}
    num = lambda seg, pat: int(re.search(pat, seg).group(1))
    for m in re.finditer(r"Function Name: (\S+)", text):
        seg = text[m.end():m.end() + 4000]
        nxt = seg.find("Function Name:")
        seg = seg if nxt < 0 else seg[:nxt]
        found[m.group(1)] = dict(scratch=num(seg, r"ScratchSize \[bytes/lane\]: (\d+)"), vgpr=num(seg, r" VGPRs: (\d+)"), agpr=num(seg, r"AGPRs: (\d+)"),
                                 spill=num(seg, r"VGPRs Spill: (\d+)"), lds=num(seg, r"LDS Size \[bytes/block\]: (\d+)"))
    return found


@pytest.mark.parametrize("build_nx", [4, 6])
def test_ais_smoother_kernels_do_not_spill(build_nx, tmp_path):
    found = _report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    assert len(found) == 2 and not any("smooth_rts" in k for k in found), sorted(found)
    for kern, (vgpr, agpr) in READ.items():
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert len(hits) == 1, "kernel %s: %d instances in the compiler report of mht_smooth_ais.hip (%d-state build)" % (kern, len(hits), build_nx)
        name, r = hits[0]
        print(name, r)
        # (SGPR "spills" are not asserted, as for the linear kernels: wave-uniform model entries parked in lanes of a vector register)
        assert r["spill"] == 0, "%s spills %d VGPRs" % (name, r["spill"])
        assert r["scratch"] == 0, "%s uses %d B of scratch per lane: a matrix is indexed dynamically or registers spill" % (name, r["scratch"])
        assert r["lds"] == 0, "%s uses %d B of LDS" % (name, r["lds"])
        assert r["vgpr"] <= vgpr and r["agpr"] <= agpr, "%s needs %d VGPRs + %d AGPRs (read when written: %d + %d)" % (name, r["vgpr"], r["agpr"], vgpr, agpr)
        assert r["vgpr"] + r["agpr"] <= 512


def test_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    assert "mht_smooth_tracks_ais" in names and "mht_smooth_ais_work_bytes" in names
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert hasattr(lib, "mht_smooth_tracks_ais") and hasattr(lib, "mht_smooth_ais_work_bytes"), "the %d-state build does not export the seam" % nx
        # (pure host arithmetic, no GPU) the lengths, then two filtered states per node -- at the scan's time and at the message's
        # time -- of a mean and a packed covariance each: twice the linear four-state smoother's
        assert lib.mht_smooth_ais_work_bytes(2000, 400) == 8192 + 400 * 2 * (4 + 10) * 2000 * 8
        assert lib.mht_smooth_ais_work_bytes(3, 5) == 256 + 5 * 2 * (4 + 10) * 3 * 8
        assert lib.mht_smooth_ais_work_bytes(2000, 400) - 8192 == 2 * (lib.mht_smooth_work_bytes(4, 2000, 400) - 8192)
        assert lib.mht_smooth_ais_work_bytes(-1, 5) == 0 and lib.mht_smooth_ais_work_bytes(3, -1) == 0
        assert lib.mht_abi_version() == 6
