"""CPU (cross-compile only): the NEES kernels (csrc/mht_nees.hip: nees_kernel<4> and nees_kernel<6>) in both code objects -- one cell
per lane with the covariance, its factor and the substitution in registers: no scratch, no spill, no LDS, nothing in the accumulator
half -- and the seam and the ABI version.  Figures as read from the compiled objects: 62 and 92 registers, five and more wavefronts
per SIMD for a kernel that streams."""
import pytest

from test_filter_resources import unit_report
from test_smooth_resources import _check_instances

# instance -> (VGPRs, AGPRs) the compiler reports, the same in the two builds
READ = {
    "nees_kernelILi4EE": (62, 0),
    "nees_kernelILi6EE": (92, 0),
}


@pytest.mark.parametrize("build_nx", [4, 6])
def test_nees_kernels_use_no_scratch_no_lds_and_few_registers(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_nees.hip" in SOURCES, "the NEES kernels are not part of the library"
    found = unit_report(tmp_path, "mht_nees.hip", ["-DMHT_NX=6"] if build_nx == 6 else [])
    _check_instances(found, READ, build_nx)
    assert len(found) == 2, sorted(found)
    assert all(r["agpr"] == 0 and r["vgpr"] <= 96 for r in found.values()), found      # (96: five wavefronts a SIMD)


def test_nees_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    assert "mht_nees_nodes" in _lib.exported_symbols()
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert hasattr(lib, "mht_nees_nodes"), "the %d-state build does not export the NEES seam" % nx
        assert lib.mht_abi_version() == 6
