"""CPU (cross-compile only): the AIS-aware smoother's kernels (csrc/mht_smooth.hip: smooth_ais_kernel<COV>, with and without the
covariance recursion) in both code objects, held to what tests/test_smooth_resources.py asks of the linear ones.  A leg's matrices are
per-lane (26 doubles in vector registers where the plain step's sit in scalar ones) and an AIS node's backward step is two steps inlined:
neither may push a matrix into scratch.  Figures as read from the compiled objects.  Plus the seam's exports and its workspace size."""
import pytest

import test_smooth_ct_resources
import test_smooth_resources
from test_smooth_resources import _check_instances, _report

# instance -> (VGPRs, AGPRs) the compiler reports (identical in the two builds: the kernels do not depend on MHT_NX); the assertion is
# "no more than this", plus: no scratch, no spill, no LDS, and VGPRs + AGPRs within the 512 entries one wavefront per SIMD can have
READ = {
    "smooth_ais_kernelILb1E": (238, 0),
    "smooth_ais_kernelILb0E": (215, 0),
}


@pytest.mark.parametrize("build_nx", [4, 6])
def test_ais_smoother_kernels_do_not_spill(build_nx, tmp_path):
    found = _report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    _check_instances(found, READ, build_nx)
    # the file's kernels are the linear, the constant-turn and these: eight instances and nothing else
    expected = list(test_smooth_resources.READ) + list(test_smooth_ct_resources.READ) + list(READ)
    assert len(expected) == 8 and len(found) == 8 and all(any(e in k for e in expected) for k in found), sorted(found)


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
