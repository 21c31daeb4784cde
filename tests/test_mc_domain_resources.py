"""CPU (cross-compile only): the kernels of csrc/mht_mc_domain.hip -- the domain engine's walk, three instances (four states, six states
linear and constant turn) -- in both code objects: no scratch, no spill (vector or scalar), nothing in the accumulator half, at most
256 vector registers and 48 KB of static LDS, of which the workgroup's counts at the limits' size (2 * 64 * 65 + 64 words, 33.5 KB) are
the larger part; and the seam, its limits and its sizer against a restatement of the layout, and the ABI version.  Figures as read from
the compiled object when written, both builds alike (the unit does not depend on MHT_NX): 114 vector registers at four states, 154 at
six states, linear and constant turn (three waves per SIMD either way); static LDS 42 504 bytes at four states and 42 744 at six: the
counts, the staged vertices (4 KB), boxes and domFirst, the staging of the wavefronts' popcounts (4 KB) and the staged arguments.  The
factor and the fold the seam launches are csrc/mht_mc.hip's, held by tests/test_mc_resources.py, which also pins that unit to its nine
kernels: the domain walk is a unit of its own."""
import ctypes as C
import os

import pytest

import mc_domain_ref as dref
import test_smooth_resources

# kernel: (vector registers as read when written, the most it may have, the most static LDS it may have)
KERNELS = {"mc_domain_walk_kernelILi4ELb0": (114, 256, 48 * 1024), "mc_domain_walk_kernelILi6ELb0": (154, 256, 48 * 1024),
           "mc_domain_walk_kernelILi6ELb1": (154, 256, 48 * 1024)}
COUNTS_BYTES = (2 * 64 * 65 + 64) * 4      # inside and firstAt [64 cells][65 steps], ever [64]: 33 536 bytes
LDS_READ = {4: 42504, 6: 42744}            # static LDS by the states of the instance, as read when written

_reports = {}


def domain_report(build_nx, tmp_path_factory):
    """test_smooth_resources._report on csrc/mht_mc_domain.hip, once per build: through a directory whose mht_smooth.hip is one #include
    of the unit, as tests/test_mc_resources.py does for csrc/mht_mc.hip."""
    if build_nx not in _reports:
        tmp_path = tmp_path_factory.mktemp("mc_domain_report_%d" % build_nx)
        src = tmp_path / "src"
        src.mkdir()
        (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(test_smooth_resources.CSRC, "mht_mc_domain.hip"))
        keep = test_smooth_resources.CSRC
        test_smooth_resources.CSRC = str(src)
        try:
            _reports[build_nx] = test_smooth_resources._report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
        finally:
            test_smooth_resources.CSRC = keep
    return _reports[build_nx]


@pytest.mark.parametrize("build_nx", [4, 6])
def test_domain_walks_use_no_scratch_no_spill_and_fit(build_nx, tmp_path_factory):
    from pymht_amd.build import SOURCES
    assert "mht_mc_domain.hip" in SOURCES, "the domain unit is not part of the library"
    found = domain_report(build_nx, tmp_path_factory)
    assert len(found) == len(KERNELS) == 3, sorted(found)      # the walk alone: the factor and the fold stay in csrc/mht_mc.hip
    for kern, (read, vgpr, lds) in KERNELS.items():
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert len(hits) == 1, (kern, sorted(found))
        name, r = hits[0]
        print("%d-state build: %s %r" % (build_nx, name, r))
        print("vector registers: %d (as read when written: %d)" % (r["vgpr"], read))
        assert r["scratch"] == 0, "%s uses %d B of scratch per lane" % (name, r["scratch"])
        assert r["spill"] == 0 and r["sgpr_spill"] == 0, "%s spills (%d vector, %d scalar registers)" % (name, r["spill"], r["sgpr_spill"])
        assert r["agpr"] == 0, "%s uses %d accumulator registers" % (name, r["agpr"])
        assert r["lds"] <= lds, "%s has %d B of static LDS" % (name, r["lds"])
        assert r["lds"] >= COUNTS_BYTES, "%s has %d B of static LDS: the counts are not in it at the limits' size" % (name, r["lds"])
        assert r["vgpr"] <= vgpr, "%s needs %d vector registers (as read when written: %d)" % (name, r["vgpr"], read)


def test_domain_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_mc_domain_work_bytes", "mht_mc_domain_encounters")
    assert all(s in names for s in seams)
    root = os.path.dirname(_lib.HERE)
    hdr = open(os.path.join(root, "include", "mht_amd.h")).read()
    assert "#define MHT_MC_DOMAIN_MAX_DOMAINS 4 " in hdr and "#define MHT_MC_DOMAIN_MAX_VERTS 256 " in hdr and "#define MHT_MC_DOMAIN_MAX_CELLS 64 " in hdr
    assert "size_t mht_mc_domain_work_bytes(" in hdr and "int mht_mc_domain_encounters(" in hdr
    own = open(os.path.join(_lib.HERE, "csrc", "mht_mc_domain.h")).read()
    assert "MC_DOMAIN_MAX_DOMAINS = 4;" in own and "MC_DOMAIN_MAX_VERTS = 256;" in own and "MC_DOMAIN_MAX_CELLS = 64;" in own
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the domain seam" % nx
        assert lib.mht_abi_version() == 6
        assert lib.mht_mc_domain_encounters.argtypes is not None and len(lib.mht_mc_domain_encounters.argtypes) == 28
        assert lib.mht_mc_domain_work_bytes.restype is C.c_size_t and len(lib.mht_mc_domain_work_bytes.argtypes) == 7
        # (nx, nComp, nTarget, G, nDomain, steps, particles)
        for shape in ((4, 70, 70, 6, 2, 7, 1024), (6, 70, 70, 6, 2, 7, 1024), (6, 13000, 500, 16, 4, 24, 4096), (4, 1, 1, 1, 1, 1, 64), (4, 1, 1, 64, 1, 64, 1 << 20),
                      (6, 5000, 3000, 3, 3, 9, 320), (4, 3, 3, 21, 3, 5, 768), (4, 1030, 1030, 2, 1, 7, 128)):
            assert lib.mht_mc_domain_work_bytes(*shape) == dref.work_bytes(*shape) > 0, shape
        for bad in ((5, 6, 3, 2, 2, 7, 128), (4, 0, 0, 2, 2, 7, 128), (4, 6, 7, 2, 2, 7, 128), (4, 6, 0, 2, 2, 7, 128), (4, 6, 3, 0, 2, 7, 128), (4, 6, 3, -1, 2, 7, 128),
                    (4, 6, 3, 2, 0, 7, 128), (4, 6, 3, 2, 5, 7, 128), (4, 6, 3, 2, -1, 7, 128), (4, 6, 3, 65, 1, 7, 128), (4, 6, 3, 33, 2, 7, 128), (4, 6, 3, 17, 4, 7, 128),
                    (4, 6, 3, 1 << 30, 4, 7, 128), (4, 6, 3, 2, 2, 0, 128), (4, 6, 3, 2, 2, 65, 128), (4, 6, 3, 2, 2, 7, 100), (4, 6, 3, 2, 2, 7, 0), (4, 6, 3, 2, 2, 7, 32),
                    (4, 6, 3, 2, 2, 7, (1 << 20) + 64), (4, -1, 1, 1, 1, 1, 64), (4, 6, -3, 2, 2, 7, 128)):
            assert lib.mht_mc_domain_work_bytes(*bad) == 0, bad
