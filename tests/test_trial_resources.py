"""CPU (cross-compile only): the trial-manoeuvre kernels (csrc/mht_trial.hip: trial_propagate_kernel<4>, <6>, trial_candidate_kernel,
trial_cell_kernel and trial_summary_kernel) in both code objects -- one track, one candidate, one cell per lane; the candidate's
trajectory of a tile read through wave-uniform loads; LDS only for the fold of a tile's four wavefronts: no scratch, no spill, nothing
in the accumulator half, 96 bytes of LDS in the cell kernel and none elsewhere -- and the seam and the ABI version.  Figures as read
from the compiled objects: 78 and 133 registers for the propagation (the encounter unit's 74 and 133, plus the staging's addresses), 77
for the candidates, 136 for the cell kernel (the pair kernel's 128 plus the fold: still three wavefronts per SIMD and more), 36 for the
summary."""
import pytest

from test_filter_resources import unit_report

# instance -> (VGPRs, AGPRs, LDS bytes a block) the compiler reports, the same in the two builds
READ = {
    "trial_propagate_kernelILi4EE": (78, 0, 0),
    "trial_propagate_kernelILi6EE": (133, 0, 0),
    "trial_candidate_kernelE": (77, 0, 0),
    "trial_cell_kernelE": (136, 0, 96),
    "trial_summary_kernelE": (36, 0, 0),
}


@pytest.mark.parametrize("build_nx", [4, 6])
def test_trial_kernels_use_no_scratch_no_spill_and_lds_for_the_fold_only(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_trial.hip" in SOURCES, "the trial-manoeuvre kernels are not part of the library"
    found = unit_report(tmp_path, "mht_trial.hip", ["-DMHT_NX=6"] if build_nx == 6 else [])
    assert len(found) == 5, sorted(found)
    for kern, (vgpr, agpr, lds) in READ.items():
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert len(hits) == 1, "kernel %s: %d instances in the compiler report of mht_trial.hip (%d-state build)" % (kern, len(hits), build_nx)
        name, r = hits[0]
        print(name, r)
        assert r["spill"] == 0, "%s spills %d VGPRs" % (name, r["spill"])
        assert r["scratch"] == 0, "%s uses %d B of scratch per lane" % (name, r["scratch"])
        assert r["lds"] == lds, "%s uses %d B of LDS (read when written: %d)" % (name, r["lds"], lds)
        assert r["vgpr"] <= vgpr and r["agpr"] == agpr == 0, "%s needs %d VGPRs + %d AGPRs (read when written: %d + %d)" % (name, r["vgpr"], r["agpr"], vgpr, agpr)
    assert all(r["vgpr"] <= 168 for r in found.values()), found      # (168: three wavefronts a SIMD, what the encounter kernels are held to)


def test_trial_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    assert "mht_trial_manoeuvres" in names and "mht_trial_work_bytes" in names
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert hasattr(lib, "mht_trial_manoeuvres") and hasattr(lib, "mht_trial_work_bytes"), "the %d-state build does not export the trial seam" % nx
        assert lib.mht_abi_version() == 6
        # (5 (K + 1) (n + G) doubles of trajectories, 4 G partials a tile, 27 (n + G) of staging, 3 G candidates: 155 doubles, rounded up to 256 bytes)
        assert lib.mht_trial_work_bytes(3, 1, 1) == 1280 and lib.mht_trial_work_bytes(0, 1, 1) == 0 and lib.mht_trial_work_bytes(3, 1, 65) == 0
        assert lib.mht_trial_work_bytes(3, 0, 1) == 0 and lib.mht_trial_work_bytes(3, 4097, 1) == 0 and lib.mht_trial_work_bytes(3, 4096, 64) > 0
