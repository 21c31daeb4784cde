"""CPU (cross-compile only): the filter kernels (csrc/mht_smooth_filter.hip: smooth_filter_kernel<N, Steps> for the linear model at 4 and
6 states, the constant-turn and the AIS model) in both code objects, held to what tests/test_smooth_trace_resources.py holds the trace
kernels to -- no scratch, no spill, no LDS, nothing in the accumulator half -- and the seams, their sizer and the ABI version.  Figures
as read from the compiled objects: 78 .. 139 registers, below the trace kernels' 105 .. 166 -- the filter is the score walk with stores
in place of its sums, and keeps neither a logarithm nor a sum live."""
import os

import pytest

import test_smooth_resources
from test_smooth_resources import CSRC, _check_instances, _report

# instance -> (VGPRs, AGPRs) the compiler reports, the same in the two builds
READ = {
    "smooth_filter_kernelILi4ENS_11LinearStepsILi4EEEE": (78, 0),
    "smooth_filter_kernelILi6ENS_11LinearStepsILi6EEEE": (139, 0),
    "smooth_filter_kernelILi6ENS_17ConstantTurnStepsEE": (125, 0),
    "smooth_filter_kernelILi4ENS_8AisStepsEE": (112, 0),
}


def unit_report(tmp_path, unit, extra):
    """_report for another unit of csrc/, pointed at it the way tests/test_smooth_trace_resources.py points it at the trace unit:
    through a directory whose mht_smooth.hip is one #include of the unit.  The module global is swapped for the length of the call and
    put back (pytest runs the tests of a process one after the other)."""
    src = tmp_path / "src"
    src.mkdir()
    (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(CSRC, unit))
    test_smooth_resources.CSRC = str(src)
    try:
        return _report(tmp_path, list(extra))
    finally:
        test_smooth_resources.CSRC = CSRC


@pytest.mark.parametrize("build_nx", [4, 6])
def test_filter_kernels_use_no_scratch_no_lds_and_few_registers(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_smooth_filter.hip" in SOURCES, "the filter kernels are not part of the library"
    found = unit_report(tmp_path, "mht_smooth_filter.hip", ["-DMHT_NX=6"] if build_nx == 6 else [])
    _check_instances(found, READ, build_nx)
    assert len(found) == 4, sorted(found)
    assert all(r["agpr"] == 0 and r["vgpr"] < 256 for r in found.values()), found


def test_filter_seams_are_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_filter_work_bytes", "mht_filter_tracks", "mht_filter_tracks_ct", "mht_filter_tracks_ais")
    assert all(s in names for s in seams)
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the filter seams" % nx
        assert lib.mht_abi_version() == 6
        # (the lengths, rounded up to 256 bytes: nothing per node -- the score's workspace)
        assert lib.mht_filter_work_bytes(4, 3, 5) == 256 and lib.mht_filter_work_bytes(6, 2000, 400) == 8192 == lib.mht_filter_work_bytes(6, 2000, 1)
        for args in ((4, 3, 5), (6, 2000, 400), (4, 0, 0), (6, 65, 60)):
            assert lib.mht_filter_work_bytes(*args) == lib.mht_score_work_bytes(*args)
        assert lib.mht_filter_work_bytes(6, 2000, 400) < lib.mht_smooth_work_bytes(6, 2000, 400)
        assert lib.mht_filter_work_bytes(5, 3, 5) == 0 and lib.mht_filter_work_bytes(4, -1, 5) == 0 and lib.mht_filter_work_bytes(4, 3, -1) == 0
        assert lib.mht_filter_work_bytes(4, 0, 0) == 0      # (an empty batch needs nothing)
