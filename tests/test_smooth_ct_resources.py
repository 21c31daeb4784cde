"""CPU (cross-compile only): the constant-turn smoother's kernels (csrc/mht_smooth.hip: smooth_rts_ct_kernel<COV>, with and without the
covariance recursion) in both code objects, held to what tests/test_smooth_resources.py asks of the linear ones.  The transition is four
per-lane numbers and not a 6 x 6 matrix (csrc/mht_smooth_ct_math.h), and float64 sin / cos are recomputed in the backward pass: neither
may push a kernel that already fills the register file into scratch.  Figures as read from the compiled objects."""
import pytest

from test_smooth_resources import _check_instances, _report

# instance -> (VGPRs, AGPRs) the compiler reports (identical in the two builds); the assertion is "no more than this", plus: no scratch,
# no spill, no LDS, and VGPRs + AGPRs within the 512 entries one wavefront per SIMD can have
READ = {
    "smooth_rts_ct_kernelILb1E": (256, 142),
    "smooth_rts_ct_kernelILb0E": (253, 0),
}


@pytest.mark.parametrize("build_nx", [4, 6])
def test_constant_turn_smoother_kernels_do_not_spill(build_nx, tmp_path):
    _check_instances(_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else []), READ, build_nx)
