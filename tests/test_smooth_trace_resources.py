"""CPU (cross-compile only): the trace kernels (csrc/mht_smooth_trace.hip: smooth_trace_kernel<N, Steps> for the linear model at 4 and 6
states, the constant-turn and the AIS model) in both code objects, held to what tests/test_smooth_score_resources.py holds the score
kernels to -- no scratch, no spill, no LDS, nothing in the accumulator half -- and the seams, their sizer and the ABI version.  Figures
as read from the compiled objects: 105 .. 166 registers, within a few of the score kernels' 103 .. 162 in either direction -- a node's
figures are stored in front of the gain, so the trace keeps nothing live that the score does not."""
import os

import pytest

import test_smooth_resources
from test_smooth_resources import CSRC, _check_instances, _report

# instance -> (VGPRs, AGPRs) the compiler reports, the same in the two builds
READ = {
    "smooth_trace_kernelILi4ENS_11LinearStepsILi4EEEE": (105, 0),
    "smooth_trace_kernelILi6ENS_11LinearStepsILi6EEEE": (150, 0),
    "smooth_trace_kernelILi6ENS_17ConstantTurnStepsEE": (135, 0),
    "smooth_trace_kernelILi4ENS_8AisStepsEE": (166, 0),
}


def trace_report(tmp_path, extra):
    """_report for csrc/mht_smooth_trace.hip, pointed at it the way tests/test_smooth_score_resources.py points it at the score unit:
    through a directory whose mht_smooth.hip is one #include of the unit.  The module global is swapped for the length of the call and
    put back (pytest runs the tests of a process one after the other)."""
    src = tmp_path / "src"
    src.mkdir()
    (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(CSRC, "mht_smooth_trace.hip"))
    test_smooth_resources.CSRC = str(src)
    try:
        return _report(tmp_path, list(extra))
    finally:
        test_smooth_resources.CSRC = CSRC


@pytest.mark.parametrize("build_nx", [4, 6])
def test_trace_kernels_use_no_scratch_no_lds_and_few_registers(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_smooth_trace.hip" in SOURCES, "the trace kernels are not part of the library"
    found = trace_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    _check_instances(found, READ, build_nx)
    assert len(found) == 4, sorted(found)
    assert all(r["agpr"] == 0 and r["vgpr"] < 256 for r in found.values()), found


def test_trace_seams_are_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_trace_work_bytes", "mht_trace_tracks", "mht_trace_tracks_ct", "mht_trace_tracks_ais")
    assert all(s in names for s in seams)
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the trace seams" % nx
        assert lib.mht_abi_version() == 6
        # (the lengths, rounded up to 256 bytes: nothing per node -- the score's workspace)
        assert lib.mht_trace_work_bytes(4, 3, 5) == 256 and lib.mht_trace_work_bytes(6, 2000, 400) == 8192 == lib.mht_trace_work_bytes(6, 2000, 1)
        assert lib.mht_trace_work_bytes(6, 2000, 400) == lib.mht_score_work_bytes(6, 2000, 400) < lib.mht_smooth_work_bytes(6, 2000, 400)
        assert lib.mht_trace_work_bytes(5, 3, 5) == 0 and lib.mht_trace_work_bytes(4, -1, 5) == 0 and lib.mht_trace_work_bytes(4, 3, -1) == 0
        assert lib.mht_trace_work_bytes(4, 0, 0) == 0      # (an empty batch needs nothing)
