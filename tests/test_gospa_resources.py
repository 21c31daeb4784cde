"""CPU (cross-compile only): gospa_kernel (csrc/mht_gospa.hip) in both code objects -- no scratch, no spill, nothing in the
accumulator half, no static LDS in front of the dynamic tables (csrc/mht_gospa.h carves them at multiples of 16) -- and the seam, its
sizer and the ABI version.  Figures as read from the compiled object: 55 vector registers in either build (the kernel does not depend
on MHT_NX)."""
import ctypes as C
import os

import pytest

import test_smooth_resources

VGPR_READ = 55


def gospa_report(tmp_path, extra):
    """test_smooth_resources._report on csrc/mht_gospa.hip: through a directory whose mht_smooth.hip is one #include of the unit, as
    tests/test_smooth_trace_resources.py does for the trace unit."""
    src = tmp_path / "src"
    src.mkdir()
    (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(test_smooth_resources.CSRC, "mht_gospa.hip"))
    keep = test_smooth_resources.CSRC
    test_smooth_resources.CSRC = str(src)
    try:
        return test_smooth_resources._report(tmp_path, list(extra))
    finally:
        test_smooth_resources.CSRC = keep


@pytest.mark.parametrize("build_nx", [4, 6])
def test_gospa_kernel_uses_no_scratch_no_spill_and_no_accumulator_registers(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_gospa.hip" in SOURCES, "the GOSPA unit is not part of the library"
    found = gospa_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    hits = [(k, v) for k, v in found.items() if "gospa_kernel" in k]
    assert len(hits) == 1 and len(found) == 1, sorted(found)
    name, r = hits[0]
    print("%d-state build: %s %r" % (build_nx, name, r))
    print("vector registers: %d" % r["vgpr"])
    assert r["scratch"] == 0, "%s uses %d B of scratch per lane" % (name, r["scratch"])
    assert r["spill"] == 0 and r["sgpr_spill"] == 0, "%s spills (%d vector, %d scalar registers)" % (name, r["spill"], r["sgpr_spill"])
    assert r["agpr"] == 0, "%s uses %d accumulator registers" % (name, r["agpr"])
    assert r["lds"] == 0, "%s has %d B of static LDS in front of its dynamic tables" % (name, r["lds"])
    assert r["vgpr"] <= 128, "%s needs %d vector registers (read when written: %d)" % (name, r["vgpr"], VGPR_READ)


def test_gospa_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    seams = ("mht_gospa_work_bytes", "mht_gospa_steps")
    assert all(s in names for s in seams)
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert all(hasattr(lib, s) for s in seams), "the %d-state build does not export the GOSPA seam" % nx
        assert lib.mht_abi_version() == 6
        assert lib.mht_gospa_steps.argtypes is not None and lib.mht_gospa_work_bytes.restype is C.c_size_t
        # (the two offset arrays, rounded up to 256 bytes; nothing per object)
        assert lib.mht_gospa_work_bytes(1, 5, 5) == 256 and lib.mht_gospa_work_bytes(300, 40000, 39000) == 2560
        assert lib.mht_gospa_work_bytes(31, 0, 0) == 256 and lib.mht_gospa_work_bytes(32, 0, 0) == 512
        assert lib.mht_gospa_work_bytes(0, 0, 0) == 0      # (an empty batch needs nothing)
        assert lib.mht_gospa_work_bytes(-1, 5, 5) == 0 and lib.mht_gospa_work_bytes(3, -1, 5) == 0 and lib.mht_gospa_work_bytes(3, 5, -1) == 0
