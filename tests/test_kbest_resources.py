"""CPU (cross-compile only): kbest_kernel (csrc/mht_kbest.hip) in both code objects -- no scratch, no spill (vector or scalar), nothing
in the accumulator half, no static LDS in front of the dynamic tables -- and the seam, its sizer against a restatement of the layout,
and the ABI version.  Figures as read from the compiled object when written: 26 vector registers in either build (the kernel does
not depend on MHT_NX), LDS dynamic only: 46 872 bytes at the limits (1024 columns, 32 targets, depth 16), under the 48 KB a kernel
has without raising its limit."""
import ctypes as C
import os

import pytest

import test_smooth_resources

VGPR_READ = 26
LDS_AT_THE_LIMITS = 46872


def kbest_report(tmp_path, extra):
    """test_smooth_resources._report on csrc/mht_kbest.hip: through a directory whose mht_smooth.hip is one #include of the unit, as
    tests/test_gospa_resources.py does for the GOSPA unit."""
    src = tmp_path / "src"
    src.mkdir()
    (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(test_smooth_resources.CSRC, "mht_kbest.hip"))
    keep = test_smooth_resources.CSRC
    test_smooth_resources.CSRC = str(src)
    try:
        return test_smooth_resources._report(tmp_path, list(extra))
    finally:
        test_smooth_resources.CSRC = keep


@pytest.mark.parametrize("build_nx", [4, 6])
def test_kbest_kernel_uses_no_scratch_and_no_spill(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_kbest.hip" in SOURCES, "the k-best unit is not part of the library"
    found = kbest_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    hits = [(k, v) for k, v in found.items() if "kbest_kernel" in k]
    assert len(hits) == 1 and len(found) == 1, sorted(found)
    name, r = hits[0]
    print("%d-state build: %s %r" % (build_nx, name, r))
    print("vector registers: %d" % r["vgpr"])
    assert r["scratch"] == 0, "%s uses %d B of scratch per lane" % (name, r["scratch"])
    assert r["spill"] == 0 and r["sgpr_spill"] == 0, "%s spills (%d vector, %d scalar registers)" % (name, r["spill"], r["sgpr_spill"])
    assert r["agpr"] == 0, "%s uses %d accumulator registers" % (name, r["agpr"])
    assert r["lds"] == 0, "%s has %d B of static LDS in front of its dynamic tables" % (name, r["lds"])
    assert r["vgpr"] <= 168, "%s needs %d vector registers (read when written: %d)" % (name, r["vgpr"], VGPR_READ)


def table_bytes(max_t, max_col, depth):
    """csrc/mht_kbest.h restated: costs, the level stack (32 B a level), the targets (24 B, one behind the last), the ranking, the rows,
    the used-row bytes"""
    r8 = lambda n: (n + 7) // 8 * 8
    return max_col * 8 + max_t * 32 + (max_t + 1) * 24 + r8(max_col * 2) + r8(max_col * depth * 2) + 2048


def test_the_tables_fit_without_raising_the_limit(tmp_path):
    import kbest_ref as ref
    twin = ref.build_twin(tmp_path)
    for shape in ((1, 1, 0), (3, 17, 1), (32, 1024, 16), (32, 1000, 5), (7, 333, 13)):
        assert twin.kbest_table_bytes_host(*shape) == table_bytes(*shape), shape
    assert table_bytes(ref.MAX_TARGETS, ref.MAX_COLUMNS, ref.MAX_DEPTH) == LDS_AT_THE_LIMITS <= 48 * 1024


def test_kbest_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_kbest_work_bytes", "mht_kbest_hypotheses", "mht_forest_leaf_rows")
    assert all(s in names for s in seams)
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "mht_amd.h")).read()
    for name, value in (("MHT_KBEST_MAX_K", 64), ("MHT_KBEST_MAX_TARGETS", 32), ("MHT_KBEST_MAX_COLUMNS", 1024), ("MHT_KBEST_MAX_DEPTH", 16),
                        ("MHT_KBEST_MAX_ROWS", 2048), ("MHT_KBEST_OK", 0), ("MHT_KBEST_NODE_LIMIT", 1), ("MHT_KBEST_TOO_LARGE", 2), ("MHT_KBEST_BAD_ROWS", 3)):
        assert "#define %s %d " % (name, value) in hdr, name
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the k-best seam" % nx
        assert lib.mht_abi_version() == 6
        assert lib.mht_kbest_hypotheses.argtypes is not None and lib.mht_kbest_work_bytes.restype is C.c_size_t
        # (the listed tuples: 2 bytes per hypothesis and target, rounded up to 256; nothing per column or cluster)
        for nHyp, nT, nC, depth, K in ((5, 2, 1, 3, 8), (40000, 700, 300, 6, 64), (1, 1, 1, 0, 1), (100, 128, 4, 16, 1), (100, 129, 4, 16, 1), (0, 0, 0, 0, 5)):
            assert lib.mht_kbest_work_bytes(nHyp, nT, nC, depth, K) == (2 * K * nT + 255) // 256 * 256, (nHyp, nT, nC, depth, K)
        for bad in ((-1, 2, 1, 3, 8), (5, -1, 1, 3, 8), (5, 2, -1, 3, 8), (5, 2, 1, -1, 8), (5, 2, 1, 3, 0), (5, 2, 1, 3, 65), (5, 2, 1, 3, -4)):
            assert lib.mht_kbest_work_bytes(*bad) == 0, bad
