"""CPU (cross-compile only): the IMM kernels (csrc/mht_imm.hip: imm_kernel<N, Steps> for the linear model at 4 and 6 states and the
constant-turn model) in both code objects, held to what tests/test_filter_resources.py holds the filter kernels to -- no scratch, no
spill, no LDS, nothing in the accumulator half, fewer than 256 registers -- and the seams, their sizer and the ABI version.  Figures as
read from the compiled objects: 155 .. 220 registers against the filter kernels' 78 .. 139 -- a lane here is one mode of a track and
carries, on top of the filter's state, the row the other modes read, the mixed state being built from theirs and its own R (its Q is
read from the table where the advance adds it: held in registers as well, the six-state kernels came to 246 and past 256)."""
import pytest

from test_filter_resources import unit_report
from test_smooth_resources import _check_instances

# instance -> (VGPRs, AGPRs) the compiler reports, the same in the two builds
READ = {
    "imm_kernelILi4ENS_11LinearStepsILi4EEEE": (155, 0),
    "imm_kernelILi6ENS_11LinearStepsILi6EEEE": (211, 0),
    "imm_kernelILi6ENS_17ConstantTurnStepsEE": (220, 0),
}


@pytest.mark.parametrize("build_nx", [4, 6])
def test_imm_kernels_use_no_scratch_no_lds_and_fewer_than_256_registers(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_imm.hip" in SOURCES, "the IMM kernels are not part of the library"
    found = unit_report(tmp_path, "mht_imm.hip", ["-DMHT_NX=6"] if build_nx == 6 else [])
    _check_instances(found, READ, build_nx)
    assert len(found) == 3, sorted(found)
    assert all(r["agpr"] == 0 and r["vgpr"] < 256 for r in found.values()), found


def test_imm_seams_are_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_imm_work_bytes", "mht_imm_tracks", "mht_imm_tracks_ct")
    assert all(s in names for s in seams)
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the IMM seams" % nx
        assert lib.mht_abi_version() == 6
        # the lengths, then the modes [r][NS + 3], Pi [r][r] and mu0 [r], each part rounded up to 256 bytes: nothing per node
        assert lib.mht_imm_work_bytes(4, 3, 5, 1) == 256 + 256 and lib.mht_imm_work_bytes(4, 3, 5, 4) == 256 + 768      # 4 (13 + 4 + 1) 8 = 576
        assert lib.mht_imm_work_bytes(6, 2000, 400, 4) == 8192 + 1024 == lib.mht_imm_work_bytes(6, 2000, 1, 4)        # 4 (24 + 4 + 1) 8 = 928
        assert lib.mht_imm_work_bytes(6, 2000, 400, 2) == 8192 + 512                                                  # 2 (24 + 2 + 1) 8 = 432
        for args in ((5, 3, 5, 2), (4, -1, 5, 2), (4, 3, -1, 2), (4, 3, 5, 0), (4, 3, 5, 5), (4, 3, 5, -1)):
            assert lib.mht_imm_work_bytes(*args) == 0, args
        assert lib.mht_imm_work_bytes(4, 0, 0, 2) == 0 and lib.mht_imm_work_bytes(6, 0, 60, 4) == 0      # (an empty batch needs nothing)
