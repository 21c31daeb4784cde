"""CPU (cross-compile only): the constant-turn smoother's kernels (csrc/mht_smooth.hip: smooth_rts_ct_kernel<COV>, with and without the
covariance recursion) in both code objects, held to what tests/test_smooth_resources.py asks of the linear ones.  The transition is four
per-lane numbers and not a 6 x 6 matrix (csrc/mht_smooth_ct_math.h), and float64 sin / cos are recomputed in the backward pass: neither
may push a kernel that already fills the register file into scratch.  Figures as read from the compiled objects."""
import pytest

from test_smooth_resources import _report

# instance -> (VGPRs, AGPRs) the compiler reports (identical in the two builds); the assertion is "no more than this", plus: no scratch,
# no spill, no LDS, and VGPRs + AGPRs within the 512 entries one wavefront per SIMD can have
READ = {
    "smooth_rts_ct_kernelILb1E": (256, 142),
    "smooth_rts_ct_kernelILb0E": (253, 0),
}


@pytest.mark.parametrize("build_nx", [4, 6])
def test_constant_turn_smoother_kernels_do_not_spill(build_nx, tmp_path):
    found = _report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    for kern, (vgpr, agpr) in READ.items():
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert len(hits) == 1, "kernel %s: %d instances in the compiler report of mht_smooth.hip (%d-state build)" % (kern, len(hits), build_nx)
        name, r = hits[0]
        print(name, r)
        # (SGPR "spills" are not asserted, as for the linear kernels: wave-uniform model entries parked in lanes of a vector register)
        assert r["spill"] == 0, "%s spills %d VGPRs" % (name, r["spill"])
        assert r["scratch"] == 0, "%s uses %d B of scratch per lane: a matrix is indexed dynamically or registers spill" % (name, r["scratch"])
        assert r["lds"] == 0, "%s uses %d B of LDS" % (name, r["lds"])
        assert r["vgpr"] <= vgpr and r["agpr"] <= agpr, "%s needs %d VGPRs + %d AGPRs (read when written: %d + %d)" % (name, r["vgpr"], r["agpr"], vgpr, agpr)
        assert r["vgpr"] + r["agpr"] <= 512
