"""CPU (cross-compile only): the kernels of csrc/mht_mc.hip in both code objects -- no scratch, no spill (vector or scalar), nothing in
the accumulator half, static LDS within 48 KB -- and the seam, its limits and its sizer against a restatement of the layout, and the ABI
version.  Figures as read from the compiled object when written, both builds alike (the unit does not depend on MHT_NX): vector
registers, walk 110 at four states, 158 at six, linear and constant turn; factor 60 and 74; fold 24.  The walk's LDS is 19.6 to 19.8
KB: the workgroup's counts at the limits' size (16.9 KB), the staging of the wavefronts' popcounts (2 KB) and the staged arguments.
The walk keeps its by-value arguments in LDS because sin, cos and log hold some eighty scalar registers of constants over the loop:
read from the scalar argument block, the model and the launch's sizes spilled scalar registers into lanes of a vector register."""
import ctypes as C
import os

import pytest

import test_smooth_resources

VGPR_READ = {"mc_walk_kernelILi4ELb0": 110, "mc_walk_kernelILi6ELb0": 158, "mc_walk_kernelILi6ELb1": 158, "mc_factor_kernelILi4": 60, "mc_factor_kernelILi6": 74,
             "mc_fold_kernel": 24}


def mc_report(tmp_path, extra):
    """test_smooth_resources._report on csrc/mht_mc.hip: through a directory whose mht_smooth.hip is one #include of the unit, as
    tests/test_kbest_resources.py does for the k-best unit."""
    src = tmp_path / "src"
    src.mkdir()
    (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(test_smooth_resources.CSRC, "mht_mc.hip"))
    keep = test_smooth_resources.CSRC
    test_smooth_resources.CSRC = str(src)
    try:
        return test_smooth_resources._report(tmp_path, list(extra))
    finally:
        test_smooth_resources.CSRC = keep


@pytest.mark.parametrize("build_nx", [4, 6])
def test_mc_kernels_use_no_scratch_and_no_spill(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_mc.hip" in SOURCES, "the Monte-Carlo unit is not part of the library"
    found = mc_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    assert len(found) == len(VGPR_READ), sorted(found)      # N = 4 and N = 6 (linear and constant turn) in BOTH builds
    for kern, read in VGPR_READ.items():
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert len(hits) == 1, (kern, sorted(found))
        name, r = hits[0]
        print("%d-state build: %s %r" % (build_nx, name, r))
        print("vector registers: %d" % r["vgpr"])
        assert r["scratch"] == 0, "%s uses %d B of scratch per lane" % (name, r["scratch"])
        assert r["spill"] == 0 and r["sgpr_spill"] == 0, "%s spills (%d vector, %d scalar registers)" % (name, r["spill"], r["sgpr_spill"])
        assert r["agpr"] == 0, "%s uses %d accumulator registers" % (name, r["agpr"])
        assert r["lds"] <= 48 * 1024, "%s has %d B of static LDS" % (name, r["lds"])
        assert r["vgpr"] <= 168, "%s needs %d vector registers (read when written: %d)" % (name, r["vgpr"], read)
        if "walk" not in kern:
            assert r["lds"] == 0, name


def work_bytes(nx, nComp, T, G, K, S):
    """csrc/mht_mc.hip's layout restated: the factors, the chunks' counts (within, then ever), the components' and the targets' status"""
    import mc_ref
    chunks = mc_ref.chunks(T, S)[0]
    return (nx * (nx + 1) // 2 * nComp * 8 + chunks * G * (K + 1) * T * 4 + chunks * G * T * 4 + nComp * 4 + T * 4 + 255) // 256 * 256


def test_mc_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_mc_work_bytes", "mht_mc_encounters")
    assert all(s in names for s in seams)
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "mht_amd.h")).read()
    for name, value in (("MHT_MC_MAX_PATHS", 64), ("MHT_MC_MAX_STEPS", 64), ("MHT_MC_MAX_PARTICLES", 1 << 20), ("MHT_MC_WARP", 64), ("MHT_MC_OK", 0), ("MHT_MC_NAN", 1),
                        ("MHT_MC_NOT_PSD", 2)):
        assert "#define %s %d " % (name, value) in hdr, name
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the Monte-Carlo seam" % nx
        assert lib.mht_abi_version() == 6
        assert lib.mht_mc_encounters.argtypes is not None and lib.mht_mc_work_bytes.restype is C.c_size_t
        for shape in ((4, 70, 70, 2, 7, 4096), (6, 70, 70, 2, 7, 4096), (6, 13000, 500, 16, 24, 65536), (4, 1, 1, 1, 1, 64), (4, 1, 1, 64, 64, 1 << 20), (6, 5000, 3000, 3, 9, 320)):
            assert lib.mht_mc_work_bytes(*shape) == work_bytes(*shape), shape
        for bad in ((5, 6, 3, 2, 7, 128), (4, 0, 0, 2, 7, 128), (4, 6, 7, 2, 7, 128), (4, 6, 0, 2, 7, 128), (4, 6, 3, 65, 7, 128), (4, 6, 3, 0, 7, 128), (4, 6, 3, 2, 0, 128),
                    (4, 6, 3, 2, 65, 128), (4, 6, 3, 2, 7, 100), (4, 6, 3, 2, 7, 0), (4, 6, 3, 2, 7, (1 << 20) + 64), (4, -1, 1, 1, 1, 64)):
            assert lib.mht_mc_work_bytes(*bad) == 0, bad
