"""CPU (cross-compile only): the kernels of the trial manoeuvres against every hypothesis (csrc/mht_trial_hyp.hip: hyp_weight_kernel,
hyp_propagate_kernel<4>, <6>, hyp_candidate_kernel, hyp_cell_kernel and hyp_target_kernel) in both code objects -- one target, one leaf,
one candidate, one cell, one (candidate, target) per lane; LDS only for the tile's (pc, dcpa, w) that the heads of the pieces fold: no
scratch, no spill, nothing in the accumulator half, 6144 bytes of LDS in the cell kernel and none elsewhere, at most 168 registers --
and the seam, its sizer and the ABI version.  Figures as read from the compiled objects: the propagation and the candidates are
mht_trial.hip's 78, 133 and 77; 132 for the cell kernel, below that unit's 136 (the serial fold of a piece needs less than the
shuffles of a tile: still three wavefronts per SIMD and more); 50 for the weights and 42 for the targets."""
import pytest

from test_filter_resources import unit_report

# instance -> (VGPRs, AGPRs, LDS bytes a block) the compiler reports, the same in the two builds
READ = {
    "hyp_weight_kernelE": (50, 0, 0),
    "hyp_propagate_kernelILi4EE": (78, 0, 0),
    "hyp_propagate_kernelILi6EE": (133, 0, 0),
    "hyp_candidate_kernelE": (77, 0, 0),
    "hyp_cell_kernelE": (132, 0, 6144),
    "hyp_target_kernelE": (42, 0, 0),
}


@pytest.mark.parametrize("build_nx", [4, 6])
def test_hypothesis_kernels_use_no_scratch_no_spill_and_lds_for_the_tile_only(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_trial_hyp.hip" in SOURCES, "the hypothesis kernels are not part of the library"
    found = unit_report(tmp_path, "mht_trial_hyp.hip", ["-DMHT_NX=6"] if build_nx == 6 else [])
    assert len(found) == 6, sorted(found)
    for kern, (vgpr, agpr, lds) in READ.items():
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert len(hits) == 1, "kernel %s: %d instances in the compiler report of mht_trial_hyp.hip (%d-state build)" % (kern, len(hits), build_nx)
        name, r = hits[0]
        print(name, r)
        assert r["spill"] == 0, "%s spills %d VGPRs" % (name, r["spill"])
        assert r["scratch"] == 0, "%s uses %d B of scratch per lane" % (name, r["scratch"])
        assert r["lds"] == lds, "%s uses %d B of LDS (read when written: %d)" % (name, r["lds"], lds)
        assert r["vgpr"] <= vgpr and r["agpr"] == agpr == 0, "%s needs %d VGPRs + %d AGPRs (read when written: %d + %d)" % (name, r["vgpr"], r["agpr"], vgpr, agpr)
    assert all(r["vgpr"] <= 168 for r in found.values()), found      # (168: three wavefronts a SIMD, what the encounter kernels are held to)


def work_bytes(L, T, G, K):
    """The layout of csrc/mht_trial_hyp.hip: the trajectories 5 (K + 1) (L + G), the partials 6 G (tiles + T), the staging for six states
    27 (L + G), the candidates 3 G and the weights L, in doubles; behind them seg [T + 1], sel [T] and the leaves' targets [L] in int32;
    rounded up to 256 bytes"""
    doubles = 5 * (K + 1) * (L + G) + 6 * G * ((L + 255) // 256 + T) + 27 * (L + G) + 3 * G + L
    return (8 * doubles + 4 * (2 * T + 1 + L) + 255) // 256 * 256


def test_hypothesis_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    assert "mht_trial_hypotheses" in names and "mht_trial_hyp_work_bytes" in names
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert hasattr(lib, "mht_trial_hypotheses") and hasattr(lib, "mht_trial_hyp_work_bytes"), "the %d-state build does not export the hypothesis seam" % nx
        assert lib.mht_abi_version() == 6
        # (3 leaves of 1 target, 1 candidate, 1 step: 40 + 12 + 108 + 3 + 3 = 166 doubles and 6 int32, 1352 bytes)
        assert lib.mht_trial_hyp_work_bytes(3, 1, 1, 1) == 1536 == work_bytes(3, 1, 1, 1)
        for args in ((600, 9, 3, 7), (13000, 500, 64, 24), (100000, 2000, 64, 24), (1, 1, 4096, 64), (257, 257, 1, 1)):
            assert lib.mht_trial_hyp_work_bytes(*args) == work_bytes(*args), args
        for args in ((0, 1, 1, 1), (3, 0, 1, 1), (3, 4, 1, 1), (-1, 1, 1, 1), (3, 1, 0, 1), (3, 1, 4097, 1), (3, 1, 1, 0), (3, 1, 1, 65)):
            assert lib.mht_trial_hyp_work_bytes(*args) == 0, args
