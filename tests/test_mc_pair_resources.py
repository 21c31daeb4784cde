"""CPU (cross-compile only): the kernels of csrc/mht_mc_pair.hip in both code objects -- no scratch, no spill (vector or scalar), nothing
in the accumulator half, static LDS within 8 KB, at most 256 vector registers (two waves per SIMD by min(8, 512 / allocation)) -- and
the seam, its limit, its sizer against a restatement of the layout, and the ABI version.  Figures as read from the compiled object
when written, both builds alike (the unit does not depend on MHT_NX): vector registers, walk 164 at four states (three waves per
SIMD), 178 at six states constant turn and 248 at six states linear (two waves: the compiler keeps Phi's 36 and F's 21 entries in
registers over the walk); factor 60 and 74; fold 16.  The walk's LDS is 2.7 KB at four states and 2.9 KB at six: the wavefronts'
meeting (4 x 131 words) and the staged arguments.  The walk steps its two particles by ONE body run twice (csrc/mht_mc_pair.h): two
inlined copies took the six-state walk to 256 vector registers plus 26 (constant turn) and 96 (linear) accumulator registers."""
import ctypes as C
import os

import pytest

import mc_pair_ref as pref
import test_smooth_resources

VGPR_READ = {"mc_pair_walk_kernelILi4ELb0": 164, "mc_pair_walk_kernelILi6ELb0": 248, "mc_pair_walk_kernelILi6ELb1": 178, "mc_pair_factor_kernelILi4": 60,
             "mc_pair_factor_kernelILi6": 74, "mc_pair_fold_kernel": 16}


def pair_report(tmp_path, extra):
    """test_smooth_resources._report on csrc/mht_mc_pair.hip: through a directory whose mht_smooth.hip is one #include of the unit, as
    tests/test_mc_resources.py does for the own-ship unit."""
    src = tmp_path / "src"
    src.mkdir()
    (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(test_smooth_resources.CSRC, "mht_mc_pair.hip"))
    keep = test_smooth_resources.CSRC
    test_smooth_resources.CSRC = str(src)
    try:
        return test_smooth_resources._report(tmp_path, list(extra))
    finally:
        test_smooth_resources.CSRC = keep


@pytest.mark.parametrize("build_nx", [4, 6])
def test_pair_kernels_use_no_scratch_no_spill_and_two_waves_fit(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_mc_pair.hip" in SOURCES, "the pair unit is not part of the library"
    found = pair_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    assert len(found) == len(VGPR_READ), sorted(found)      # N = 4 and N = 6 (linear and constant turn) in BOTH builds
    for kern, read in VGPR_READ.items():
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert len(hits) == 1, (kern, sorted(found))
        name, r = hits[0]
        print("%d-state build: %s %r" % (build_nx, name, r))
        print("vector registers: %d (read when written: %d)" % (r["vgpr"], read))
        assert r["scratch"] == 0, "%s uses %d B of scratch per lane" % (name, r["scratch"])
        assert r["spill"] == 0 and r["sgpr_spill"] == 0, "%s spills (%d vector, %d scalar registers)" % (name, r["spill"], r["sgpr_spill"])
        assert r["agpr"] == 0, "%s uses %d accumulator registers" % (name, r["agpr"])
        assert r["lds"] <= 8 * 1024, "%s has %d B of static LDS" % (name, r["lds"])
        assert r["vgpr"] <= 256, "%s needs %d vector registers (read when written: %d)" % (name, r["vgpr"], read)
        if "walk" not in kern:
            assert r["lds"] == 0, name


def test_pair_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_mc_pair_work_bytes", "mht_mc_pair_encounters")
    assert all(s in names for s in seams)
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "mht_amd.h")).read()
    assert "#define MHT_MC_MAX_PAIRS 1048576" in hdr
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the pair seam" % nx
        assert lib.mht_abi_version() == 6
        assert lib.mht_mc_pair_encounters.argtypes is not None and len(lib.mht_mc_pair_encounters.argtypes) == 25
        assert lib.mht_mc_pair_work_bytes.restype is C.c_size_t
        # (nx, nComp, nTarget, nPair, steps, particles)
        for shape in ((4, 70, 70, 2415, 7, 4096), (6, 70, 70, 64, 7, 4096), (6, 13000, 500, 124750, 24, 4096), (4, 2, 2, 1, 1, 64), (4, 2, 2, 1, 64, 1 << 20),
                      (6, 5000, 3000, 1 << 20, 9, 320)):
            assert lib.mht_mc_pair_work_bytes(*shape) == pref.work_bytes(*shape) > 0, shape
        for bad in ((5, 6, 3, 2, 7, 128), (4, 0, 0, 2, 7, 128), (4, 6, 7, 2, 7, 128), (4, 6, 0, 2, 7, 128), (4, 6, 3, (1 << 20) + 1, 7, 128), (4, 6, 3, 0, 7, 128),
                    (4, 6, 3, -1, 7, 128), (4, 6, 3, 2, 0, 128), (4, 6, 3, 2, 65, 128), (4, 6, 3, 2, 7, 100), (4, 6, 3, 2, 7, 0), (4, 6, 3, 2, 7, 32),
                    (4, 6, 3, 2, 7, (1 << 20) + 64), (4, -1, 1, 1, 1, 64), (4, 6, -3, 2, 7, 128)):
            assert lib.mht_mc_pair_work_bytes(*bad) == 0, bad
