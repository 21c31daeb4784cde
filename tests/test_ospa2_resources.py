"""CPU (cross-compile only): the kernels of csrc/mht_ospa2.hip in both code objects -- no scratch, no spill, nothing in the accumulator
half, at most 128 vector registers; no static LDS anywhere, so ospa2_assign_kernel has none in front of its dynamic tables -- the
search they share with gospa_kernel still within that kernel's own bounds, and the seam, its sizer and the ABI version.  Figures as read
from the compiled object (neither build differs: the kernels do not depend on MHT_NX): ospa2_members_kernel 12, ospa2_base_kernel 70,
ospa2_assign_kernel 46 vector registers."""
import ctypes as C
import os

import pytest

import test_gospa_resources
import test_smooth_resources

KERNELS = ("ospa2_members_kernel", "ospa2_base_kernel", "ospa2_assign_kernel")


def ospa2_report(tmp_path, extra):
    """test_smooth_resources._report on csrc/mht_ospa2.hip, through a directory whose mht_smooth.hip is one #include of the unit"""
    src = tmp_path / "src"
    src.mkdir()
    (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(test_smooth_resources.CSRC, "mht_ospa2.hip"))
    keep = test_smooth_resources.CSRC
    test_smooth_resources.CSRC = str(src)
    try:
        return test_smooth_resources._report(tmp_path, list(extra))
    finally:
        test_smooth_resources.CSRC = keep


@pytest.mark.parametrize("build_nx", [4, 6])
def test_ospa2_kernels_use_no_scratch_no_spill_and_no_accumulator_registers(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_ospa2.hip" in SOURCES, "the OSPA(2) unit is not part of the library"
    found = ospa2_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    assert len(found) == len(KERNELS), sorted(found)
    for kern in KERNELS:
        hits = [(k, v) for k, v in found.items() if kern in k]
        assert len(hits) == 1, (kern, sorted(found))
        name, r = hits[0]
        print("%d-state build: %s %r" % (build_nx, name, r))
        print("vector registers of %s: %d" % (kern, r["vgpr"]))
        assert r["scratch"] == 0, "%s uses %d B of scratch per lane" % (name, r["scratch"])
        assert r["spill"] == 0 and r["sgpr_spill"] == 0, "%s spills (%d vector, %d scalar registers)" % (name, r["spill"], r["sgpr_spill"])
        assert r["agpr"] == 0, "%s uses %d accumulator registers" % (name, r["agpr"])
        assert r["lds"] == 0, "%s has %d B of static LDS" % (name, r["lds"])
        assert r["vgpr"] <= 128, "%s needs %d vector registers" % (name, r["vgpr"])


@pytest.mark.parametrize("build_nx", [4, 6])
def test_gospa_kernel_still_meets_its_own_bounds(build_nx, tmp_path):
    """The search became a template over its cost; gospa_kernel is held to what tests/test_gospa_resources.py holds it to."""
    test_gospa_resources.test_gospa_kernel_uses_no_scratch_no_spill_and_no_accumulator_registers(build_nx, tmp_path)


def test_ospa2_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_ospa2_work_bytes", "mht_ospa2_windows")
    assert all(s in names for s in seams)
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the OSPA(2) seam" % nx
        assert lib.mht_abi_version() == 6
        assert lib.mht_ospa2_windows.argtypes is not None and lib.mht_ospa2_work_bytes.restype is C.c_size_t
        # lo and hi; the member counts; the two index lists; one n x m float64 matrix per window -- each rounded up to 256 bytes
        assert lib.mht_ospa2_work_bytes(5, 3, 10, 1) == 256 + 256 + 256 + 256 + 256
        r256 = lambda b: (b + 255) // 256 * 256
        assert lib.mht_ospa2_work_bytes(500, 400, 100, 100) == 1024 + 1024 + r256(100 * 500 * 4) + r256(100 * 400 * 4) + 100 * 500 * 400 * 8
        assert lib.mht_ospa2_work_bytes(2048, 2048, 50, 200) > 2 ** 32      # (the offsets are 64-bit)
        assert lib.mht_ospa2_work_bytes(0, 7, 3, 2) == 256 + 256 + 0 + 256 + 0      # (tracks there are none: no matrix)
        for empty in ((5, 3, 10, 0), (5, 3, 0, 4)):      # an empty batch needs nothing
            assert lib.mht_ospa2_work_bytes(*empty) == 0
        for bad in ((-1, 3, 10, 1), (5, -1, 10, 1), (5, 3, -1, 1), (5, 3, 10, -1), (2049, 3, 10, 1), (5, 2049, 10, 1)):
            assert lib.mht_ospa2_work_bytes(*bad) == 0
