"""CPU (cross-compile only): the grid score kernels (csrc/mht_smooth_score_grid.hip: smooth_score_grid_kernel<N, Steps> for the linear model
at 4 and 6 states and the constant-turn model) in both code objects, held to what tests/test_smooth_score_resources.py holds the score
kernels to -- no scratch, no spill, no LDS, nothing in the accumulator half -- and the seams, their sizer's presence and the ABI version.

The candidate's Q and R are read through a wavefront-uniform address (blockIdx.y), so they cannot need more vector registers than
the per-track theta of smooth_score_theta_kernel, whose Q and R are per lane: 128 registers at four states and 204 at six is the bound,
from that argument and not from these kernels.  Figures as read from the compiled objects, the same in the two builds: 102, 157 and 145
registers -- the score kernels' own 103, 157 and 145 under the batch's model: the candidate costs no vector register."""
import os

import pytest

import test_smooth_resources
from test_smooth_resources import CSRC, _check_instances, _report
from test_smooth_score_resources import READ as SCORE_READ

# instance -> (VGPRs, AGPRs): the bound, the per-track-theta instances' of the same state count (tests/test_smooth_score_resources.py)
BOUND = {
    "smooth_score_grid_kernelILi4ENS_11LinearStepsILi4EEEE": SCORE_READ["smooth_score_theta_kernelILi4EE"],
    "smooth_score_grid_kernelILi6ENS_11LinearStepsILi6EEEE": SCORE_READ["smooth_score_theta_kernelILi6EE"],
    "smooth_score_grid_kernelILi6ENS_17ConstantTurnStepsEE": SCORE_READ["smooth_score_theta_kernelILi6EE"],
}
# what the compiler reports for them
READ = {
    "smooth_score_grid_kernelILi4ENS_11LinearStepsILi4EEEE": (102, 0),
    "smooth_score_grid_kernelILi6ENS_11LinearStepsILi6EEEE": (157, 0),
    "smooth_score_grid_kernelILi6ENS_17ConstantTurnStepsEE": (145, 0),
}
SEAMS = ("mht_score_grid_work_bytes", "mht_score_tracks_grid", "mht_score_tracks_ct_grid")


def grid_report(tmp_path, extra):
    """_report for csrc/mht_smooth_score_grid.hip, pointed at it the way test_smooth_score_resources.score_report points it at the score
    unit: through a directory whose mht_smooth.hip is one #include of the unit, the module global swapped for the length of the call."""
    src = tmp_path / "src"
    src.mkdir()
    (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(CSRC, "mht_smooth_score_grid.hip"))
    test_smooth_resources.CSRC = str(src)
    try:
        return _report(tmp_path, list(extra))
    finally:
        test_smooth_resources.CSRC = CSRC


@pytest.mark.parametrize("build_nx", [4, 6])
def test_grid_kernels_use_no_scratch_no_lds_and_no_more_registers_than_a_per_lane_candidate(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_smooth_score_grid.hip" in SOURCES, "the grid score kernels are not part of the library"
    assert BOUND[next(k for k in BOUND if "ILi4E" in k)] == (128, 0) and all(BOUND[k] == (204, 0) for k in BOUND if "ILi6E" in k)
    found = grid_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    assert len(found) == 3, sorted(found)
    _check_instances(found, BOUND, build_nx)
    _check_instances(found, READ, build_nx)
    assert all(r["agpr"] == 0 for r in found.values()), found


def test_grid_seams_are_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    assert all(s in names for s in SEAMS)
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in SEAMS), "the %d-state build does not export the grid score seams" % nx
        assert lib.mht_abi_version() == 6
        assert lib.mht_score_grid_work_bytes(6, 2000, 400, 64) == lib.mht_score_work_bytes(6, 2000, 400) + 64 * 24 * 8
