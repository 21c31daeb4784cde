"""CPU (cross-compile only): the encounter kernels (csrc/mht_encounter.hip: encounter_propagate_kernel<4>, <6> and
encounter_pair_kernel) in both code objects -- one entry per lane with x, P and Phi P in registers; one cell per lane with the row's
trajectory read through wave-uniform loads, so the staging needs no LDS at all: no scratch, no spill, no LDS, nothing in the
accumulator half -- and the seam and the ABI version.  Figures as read from the compiled objects: 74 and 133 registers for the
propagation, 128 for the pair kernel (four wavefronts per SIMD for a kernel bound by float64 transcendentals)."""
import pytest

from test_filter_resources import unit_report
from test_smooth_resources import _check_instances

# instance -> (VGPRs, AGPRs) the compiler reports, the same in the two builds
READ = {
    "encounter_propagate_kernelILi4EE": (74, 0),
    "encounter_propagate_kernelILi6EE": (133, 0),
    "encounter_pair_kernelE": (128, 0),
}


@pytest.mark.parametrize("build_nx", [4, 6])
def test_encounter_kernels_use_no_scratch_no_lds_and_no_spill(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_encounter.hip" in SOURCES, "the encounter kernels are not part of the library"
    found = unit_report(tmp_path, "mht_encounter.hip", ["-DMHT_NX=6"] if build_nx == 6 else [])
    _check_instances(found, READ, build_nx)      # (no VGPR spill, no scratch, LDS 0: the staging needs none)
    assert len(found) == 3, sorted(found)
    assert all(r["agpr"] == 0 and r["vgpr"] <= 168 for r in found.values()), found      # (168: three wavefronts a SIMD)


def test_encounter_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    assert "mht_encounters" in names and "mht_encounter_work_bytes" in names
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert hasattr(lib, "mht_encounters") and hasattr(lib, "mht_encounter_work_bytes"), "the %d-state build does not export the encounter seam" % nx
        assert lib.mht_abi_version() == 6
        assert lib.mht_encounter_work_bytes(3, 1) == 256 and lib.mht_encounter_work_bytes(0, 1) == 0 and lib.mht_encounter_work_bytes(3, 65) == 0
