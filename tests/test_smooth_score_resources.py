"""CPU (cross-compile only): the score kernels (csrc/mht_smooth_score.hip: smooth_score_kernel<N, Steps> for the linear model at 4 and 6
states, the constant-turn and the AIS model, and smooth_score_theta_kernel<N>, the linear walk under per-track theta) in both code
objects, held to what tests/test_smooth_resources.py holds the smoother kernels to -- no scratch, no spill, no LDS -- and the seams,
their sizer and the ABI version.  Figures as read from the compiled objects: a forward pass keeps (x, P), one prediction and one gain
live and nothing of a backward step: 103 .. 162 registers under the batch's model and 128 / 204 under per-track theta (Q and R then
live in vector registers), none in the accumulator half -- against 203 and 400 for the covariance smoothers of the same state counts
(tests/test_smooth_resources.py)."""
import os

import pytest

import test_smooth_resources
from test_smooth_resources import CSRC, _check_instances, _report

# instance -> (VGPRs, AGPRs) the compiler reports, the same in the two builds
READ = {
    "smooth_score_kernelILi4ENS_11LinearStepsILi4EEEE": (103, 0),
    "smooth_score_kernelILi6ENS_11LinearStepsILi6EEEE": (157, 0),
    "smooth_score_kernelILi6ENS_17ConstantTurnStepsEE": (145, 0),
    "smooth_score_kernelILi4ENS_8AisStepsEE": (162, 0),
    "smooth_score_theta_kernelILi4EE": (128, 0),
    "smooth_score_theta_kernelILi6EE": (204, 0),
}


def score_report(tmp_path, extra):
    """_report for csrc/mht_smooth_score.hip, pointed at it the way tests/test_smooth_em_resources.py points it at the EM unit: through a
    directory whose mht_smooth.hip is one #include of the unit.  The module global is swapped for the length of the call and put back
    (pytest runs the tests of a process one after the other)."""
    src = tmp_path / "src"
    src.mkdir()
    (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(CSRC, "mht_smooth_score.hip"))
    test_smooth_resources.CSRC = str(src)
    try:
        return _report(tmp_path, list(extra))
    finally:
        test_smooth_resources.CSRC = CSRC


@pytest.mark.parametrize("build_nx", [4, 6])
def test_score_kernels_use_no_scratch_no_lds_and_few_registers(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_smooth_score.hip" in SOURCES, "the score kernels are not part of the library"
    found = score_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    _check_instances(found, READ, build_nx)
    assert len(found) == 6, sorted(found)
    # below the smoothers: not one of them needs the accumulator half
    assert all(r["agpr"] == 0 and r["vgpr"] < 256 for r in found.values()), found


def test_score_seams_are_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_score_work_bytes", "mht_score_tracks", "mht_score_tracks_ct", "mht_score_tracks_ais", "mht_smooth_tracks_em_ll")
    assert all(s in names for s in seams)
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the score seams" % nx
        assert lib.mht_abi_version() == 6
        # (the lengths, rounded up to 256 bytes: nothing per node)
        assert lib.mht_score_work_bytes(4, 3, 5) == 256 and lib.mht_score_work_bytes(6, 2000, 400) == 8192 == lib.mht_score_work_bytes(6, 2000, 1)
        assert lib.mht_score_work_bytes(6, 2000, 400) < lib.mht_smooth_work_bytes(6, 2000, 400)
        assert lib.mht_score_work_bytes(5, 3, 5) == 0 and lib.mht_score_work_bytes(4, -1, 5) == 0 and lib.mht_score_work_bytes(4, 3, -1) == 0
