"""CPU (cross-compile only): the IMM smoother's kernels (csrc/mht_imm_smooth.hip: imm_smooth_kernel<N, Steps> for the linear model at 4
and 6 states and the constant-turn model) in both code objects -- no scratch, no spill, no LDS, the register figures as read from the
compiled objects -- and the seams, their sizer and the ABI version.

At four states the kernel stays in the vector half: 255 registers, none in the accumulator half.  At six states it does not: 256 and
152 (linear), 256 and 162 (constant turn).  The peak is the backward step, which is the smoothers' own smooth_backward_gain --
tests/test_smooth_resources.py pins the plain six-state smoother at 256 and 144 -- plus what a lane of a quad carries through it (its
row of Pi, lnL_j, the pointers).  The mode's Q is read from the table where it is added and the terms run in a loop over the modes:
with Q held or the loop unrolled the six-state linear kernel needed 140 - 172 bytes of scratch per lane, which is not acceptable."""
import pytest

from test_filter_resources import unit_report
from test_smooth_resources import _check_instances

# instance -> (VGPRs, AGPRs) the compiler reports, the same in the two builds
READ = {
    "imm_smooth_kernelILi4ENS_11LinearStepsILi4EEEE": (255, 0),
    "imm_smooth_kernelILi6ENS_11LinearStepsILi6EEEE": (256, 152),
    "imm_smooth_kernelILi6ENS_17ConstantTurnStepsEE": (256, 162),
}


@pytest.mark.parametrize("build_nx", [4, 6])
def test_imm_smooth_kernels_use_no_scratch_no_lds_and_the_registers_read(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_imm_smooth.hip" in SOURCES, "the IMM smoother's kernels are not part of the library"
    found = unit_report(tmp_path, "mht_imm_smooth.hip", ["-DMHT_NX=6"] if build_nx == 6 else [])
    _check_instances(found, READ, build_nx)      # (no spill, no scratch, no LDS, no more registers than read, at most 512 in all)
    assert len(found) == 3, sorted(found)
    four = [r for k, r in found.items() if "ILi4E" in k]
    assert len(four) == 1 and four[0]["agpr"] == 0 and four[0]["vgpr"] < 256, found


def test_imm_smooth_seams_are_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_imm_smooth_work_bytes", "mht_imm_smooth_tracks", "mht_imm_smooth_tracks_ct")
    assert all(s in names for s in seams)
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the IMM smoother's seams" % nx
        assert lib.mht_abi_version() == 6
        # mht_imm_work_bytes' figure, then per node and mode the row [x | P packed | mu]: L_max r (nx + nx (nx + 1) / 2 + 1) n 8, rounded up to 256
        assert lib.mht_imm_smooth_work_bytes(4, 3, 5, 1) == 512 + 2048                        # 5 x 1 x 15 x 3 x 8 = 1800
        assert lib.mht_imm_smooth_work_bytes(4, 3, 5, 4) == 1024 + 7424                       # 5 x 4 x 15 x 3 x 8 = 7200
        assert lib.mht_imm_smooth_work_bytes(6, 2000, 400, 4) == 9216 + 716800000             # 400 x 4 x 28 x 2000 x 8
        assert lib.mht_imm_smooth_work_bytes(6, 2000, 1, 4) == 9216 + 1792000
        assert lib.mht_imm_smooth_work_bytes(6, 2000, 400, 2) == 8704 + 358400000
        assert lib.mht_imm_smooth_work_bytes(6, 100000, 3000, 4) == lib.mht_imm_work_bytes(6, 100000, 3000, 4) + 268800000000      # (past 2^32: size_t)
        for args in ((4, 3, 5, 1), (4, 3, 5, 4), (6, 2000, 400, 4)):
            assert lib.mht_imm_smooth_work_bytes(*args) > lib.mht_imm_work_bytes(*args) > 0
        for args in ((5, 3, 5, 2), (4, -1, 5, 2), (4, 3, -1, 2), (4, 3, 5, 0), (4, 3, 5, 5), (4, 3, 5, -1), (4, 0, 0, 2), (6, 0, 60, 4)):
            assert lib.mht_imm_smooth_work_bytes(*args) == 0 == lib.mht_imm_work_bytes(*args), args
