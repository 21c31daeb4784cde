"""CPU (cross-compile only): the EM smoother's kernels (csrc/mht_smooth_em.hip: smooth_em_kernel<NX, LAST>, NX = 4 and 6; LAST = false is a
learning walk, LAST = true the walk that writes the output) in both code objects, held to what tests/test_smooth_resources.py holds the
other smoother kernels to; the seam, its sizer, the reference's self-consistency and the Python refusals that need no GPU.
Figures as read from the compiled objects."""
import os

import numpy as np
import pytest

import test_smooth_resources
from test_smooth_resources import CSRC, _check_instances, _report

READ = {
    "smooth_em_kernelILi4ELb1E": (227, 0),
    "smooth_em_kernelILi4ELb0E": (256, 8),
    "smooth_em_kernelILi6ELb1E": (256, 174),
    "smooth_em_kernelILi6ELb0E": (255, 250),
}


def em_report(tmp_path, extra):
    """_report for csrc/mht_smooth_em.hip: that function compiles the file called mht_smooth.hip in its module's CSRC, so it is pointed at
    a directory whose file of that name is one #include of the EM unit (a compile error it reports therefore names mht_smooth.hip).
    The module global is swapped for the length of the call and put back: NOT safe where tests of one process run in parallel threads
    (pytest runs them one after the other; separate worker processes each have their own module)."""
    src = tmp_path / "src"
    src.mkdir()
    (src / "mht_smooth.hip").write_text('#include "%s"\n' % os.path.join(CSRC, "mht_smooth_em.hip"))
    test_smooth_resources.CSRC = str(src)
    try:
        return _report(tmp_path, list(extra))
    finally:
        test_smooth_resources.CSRC = CSRC


@pytest.mark.parametrize("build_nx", [4, 6])
def test_em_kernels_do_not_spill(build_nx, tmp_path):
    from pymht_amd.build import SOURCES
    assert "mht_smooth_em.hip" in SOURCES, "the EM smoother is not part of the library"
    found = em_report(tmp_path, ["-DMHT_NX=6"] if build_nx == 6 else [])
    _check_instances(found, READ, build_nx)
    assert len(found) == 4, sorted(found)


def test_em_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    assert "mht_smooth_tracks_em" in names and "mht_smooth_em_work_bytes" in names
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert hasattr(lib, "mht_smooth_tracks_em") and hasattr(lib, "mht_smooth_em_work_bytes"), "the %d-state build does not export the EM smoother" % nx
        assert lib.mht_abi_version() == 6
        for shape in ((4, 3, 5), (6, 2000, 400), (6, 1, 1), (4, 130, 300)):
            assert lib.mht_smooth_em_work_bytes(*shape) >= lib.mht_smooth_work_bytes(*shape) > 0
        # (theta, the sums and the parked state: 2 nx + 4 nx (nx + 1) / 2 + 7 doubles a track)
        assert lib.mht_smooth_em_work_bytes(6, 2000, 400) == lib.mht_smooth_work_bytes(6, 2000, 400) + (12 + 84 + 7) * 2000 * 8
        assert lib.mht_smooth_em_work_bytes(5, 3, 5) == 0 and lib.mht_smooth_em_work_bytes(4, -1, 5) == 0 and lib.mht_smooth_em_work_bytes(4, 3, -1) == 0


def test_em_reference_is_self_consistent():
    """tests/smooth_em_ref.py in float64 against itself in np.longdouble; without an iteration it is smooth_ref.rts."""
    import smooth_em_ref as er
    import smooth_ref as sr
    from pymht_amd.models import ca
    assert np.finfo(np.longdouble).eps < 1e-18
    mats = sr.model_matrices(ca, 2.5)
    (x0, P0, z), = sr.make_batch(ca, 2.5, [60], seed=3)
    a, b = er.em(*mats, x0, P0, z, 5, dtype=np.float64), er.em(*mats, x0, P0, z, 5, dtype=np.longdouble)
    assert b["xs"].dtype == np.longdouble and b["Q"].dtype == np.longdouble
    for k in ("xs", "Ps", "Q", "R"):
        assert np.isfinite(a[k]).all() and sr.err(a[k], b[k]) < 1e-9, k
    assert 0 < sr.err(a["xs"], b["xs"])
    assert not np.array_equal(a["Q"], np.asarray(mats[1], dtype=np.float64)) and not np.array_equal(a["R"], np.asarray(mats[3], dtype=np.float64))
    zero, rts = er.em(*mats, x0, P0, z, 0), sr.rts(*mats, x0, P0, z)
    assert np.array_equal(zero["xs"], rts["xs"]) and np.array_equal(zero["Ps"], rts["Ps"])
    one = er.em(*mats, x0, P0, z[:1], 5)
    assert np.array_equal(one["xs"][0], x0) and np.array_equal(one["Ps"][0], P0) and np.array_equal(one["Q"], np.asarray(mats[1], dtype=np.float64))


def test_refusals_that_need_no_gpu():
    from pymht_amd.models import ct, pv
    from pymht_amd.smoothing import smooth_nodes, smooth_tracks_em
    track = [(np.zeros(4), pv.P0, [None, np.zeros(2)])]
    with pytest.raises(NotImplementedError, match="ct"):
        smooth_tracks_em(ct, 2.5, [(np.zeros(6), ct.P0, [None, np.zeros(2)])])
    with pytest.raises(ValueError, match="start"):
        smooth_tracks_em(pv, 2.5, track, start="pykalman")
    for bad in (-1, 65, 2.0, "5", True, None):
        with pytest.raises(ValueError, match="n_iter"):
            smooth_tracks_em(pv, 2.5, track, n_iter=bad)
    with pytest.raises(ValueError, match="em"):
        smooth_nodes(ct, 2.5, [], constantTurn=True, em=5)
    with pytest.raises(ValueError, match="em"):
        smooth_nodes(pv, 2.5, [], ais=lambda scan, mmsi: None, em=5)
    with pytest.raises(ValueError, match="n_iter"):
        smooth_nodes(pv, 2.5, [], em=-1)
