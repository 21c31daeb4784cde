"""CPU (cross-compile only): the kernels of csrc/mht_mc.hip -- both Monte-Carlo engines, own ship and pairs of targets -- in both code
objects: no scratch, no spill (vector or scalar), nothing in the accumulator half; the own-ship walk within 168 vector registers and
48 KB of static LDS, the pair walk within 256 vector registers (two waves per SIMD by min(8, 512 / allocation)) and 8 KB, the factor
and the fold, which both engines launch, within 168 and without LDS -- and the two seams, their limits and their sizers against
restatements of the layout, and the ABI version.  Figures as read from the compiled object when written, both builds alike (the unit
does not depend on MHT_NX): vector registers, own-ship walk 110 at four states, 158 at six, linear and constant turn; pair walk 164 at
four states (three waves per SIMD), 178 at six states constant turn and 248 at six states linear (two waves: the compiler keeps Phi's
36 and F's 21 entries in registers over the walk); factor 60 and 74; fold 16.  The own-ship walk's LDS is 19.5 to 19.8 KB: the
workgroup's counts at the limits' size (16.9 KB), the staging of the wavefronts' popcounts (2 KB) and the staged arguments; the pair
walk's is 2.7 KB at four states and 2.9 KB at six: the wavefronts' meeting (4 x 131 words) and the staged arguments.  The walks keep
their by-value arguments in LDS because sin, cos and log hold some eighty scalar registers of constants over the loop: read from the
scalar argument block, the model and the launch's sizes spilled scalar registers into lanes of a vector register.  The pair walk steps
its two particles by ONE body run twice (csrc/mht_mc_pair.h): two inlined copies took the six-state walk to 256 vector registers plus
26 (constant turn) and 96 (linear) accumulator registers."""
import ctypes as C
import os

import pytest

import mc_pair_ref as pref
import test_smooth_resources

# kernel: (vector registers read when written, the most it may have, the most static LDS it may have)
KERNELS = {"mc_walk_kernelILi4ELb0": (110, 168, 48 * 1024), "mc_walk_kernelILi6ELb0": (158, 168, 48 * 1024), "mc_walk_kernelILi6ELb1": (158, 168, 48 * 1024),
           "mc_pair_walk_kernelILi4ELb0": (164, 256, 8 * 1024), "mc_pair_walk_kernelILi6ELb0": (248, 256, 8 * 1024), "mc_pair_walk_kernelILi6ELb1": (178, 256, 8 * 1024),
           "mc_factor_kernelILi4": (60, 168, 0), "mc_factor_kernelILi6": (74, 168, 0), "mc_fold_kernel": (16, 168, 0)}


_reports = {}


def mc_report(build_nx, tmp_path_factory):
    """test_smooth_resources._report on csrc/mht_mc.hip, once per build: through a directory whose mht_smooth.hip is one #include of the
    unit, as tests/test_kbest_resources.py does for the k-best unit."""
    if build_nx not in _reports:
        tmp_path = tmp_path_factory.mktemp("mc_report_%d" % build_nx)
        src = tmp_path / "src"
        src.mkdir()
        (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(test_smooth_resources.CSRC, "mht_mc.hip"))
        keep = test_smooth_resources.CSRC
        test_smooth_resources.CSRC = str(src)
        try:
            _reports[build_nx] = test_smooth_resources._report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
        finally:
            test_smooth_resources.CSRC = keep
    return _reports[build_nx]


def _check_kernels(build_nx, tmp_path_factory, mine):
    """The rows of KERNELS that `mine` picks, in the report of the one unit"""
    from pymht_amd.build import SOURCES
    assert "mht_mc.hip" in SOURCES, "the Monte-Carlo unit is not part of the library"
    found = mc_report(build_nx, tmp_path_factory)
    # three own-ship walks and three pair walks (N = 4, N = 6 linear and constant turn), two factors, one fold, in BOTH builds
    assert len(found) == len(KERNELS) == 9, sorted(found)
    for kern, (read, vgpr, lds) in KERNELS.items():
        if not mine(kern):
            continue
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert len(hits) == 1, (kern, sorted(found))
        name, r = hits[0]
        print("%d-state build: %s %r" % (build_nx, name, r))
        print("vector registers: %d (read when written: %d)" % (r["vgpr"], read))
        assert r["scratch"] == 0, "%s uses %d B of scratch per lane" % (name, r["scratch"])
        assert r["spill"] == 0 and r["sgpr_spill"] == 0, "%s spills (%d vector, %d scalar registers)" % (name, r["spill"], r["sgpr_spill"])
        assert r["agpr"] == 0, "%s uses %d accumulator registers" % (name, r["agpr"])
        assert r["lds"] <= lds, "%s has %d B of static LDS" % (name, r["lds"])
        assert r["vgpr"] <= vgpr, "%s needs %d vector registers (read when written: %d)" % (name, r["vgpr"], read)


@pytest.mark.parametrize("build_nx", [4, 6])
def test_mc_kernels_use_no_scratch_and_no_spill(build_nx, tmp_path_factory):
    """The own-ship walks, and the factor and the fold that both engines launch"""
    _check_kernels(build_nx, tmp_path_factory, lambda kern: "pair" not in kern)


@pytest.mark.parametrize("build_nx", [4, 6])
def test_pair_kernels_use_no_scratch_no_spill_and_two_waves_fit(build_nx, tmp_path_factory):
    """The pair walks, and the factor and the fold that both engines launch"""
    _check_kernels(build_nx, tmp_path_factory, lambda kern: "mc_walk" not in kern)


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
