"""CPU: the constant-turn smoother's yardstick (tests/smooth_ct_ref.py) against itself in np.longdouble and against the linear reference
where the two must agree; the seam's exports and host-side arithmetic; and the device arithmetic itself (csrc/mht_smooth_ct_math.h)
compiled for the host and held to the criterion of tests/test_smooth_ct_gpu.py with the host's libm in place of the device's sin / cos."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import smooth_ct_ref as cr
import smooth_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 2.5
FACTOR = 8.0


def _accuracy_batch():
    """The batch of tests/test_smooth_ct_gpu.py::test_accuracy_against_the_longdouble_truth."""
    from pymht_amd.models import ct
    rng = np.random.default_rng(20240)
    lengths = [int(v) for v in rng.integers(2, 401, 40)]
    return ct, cr.make_batch(ct, PERIOD, lengths, seed=17, p_detect=0.8)


@pytest.fixture(scope="module")
def batch_refs():
    ct, tracks = _accuracy_batch()
    mats = cr.model_matrices(ct, PERIOD)
    truth = [cr.rts_ct(*mats, x0, P0, z, dtype=np.longdouble) for x0, P0, z in tracks]
    f64 = [cr.rts_ct(*mats, x0, P0, z, dtype=np.float64) for x0, P0, z in tracks]
    return ct, tracks, truth, f64


def test_batch_covers_the_turn_rates_and_the_coupled_covariance(batch_refs):
    ct, tracks, truth, f64 = batch_refs
    w0 = np.array([t[0][4] for t in tracks])
    a0 = np.array([t[0][5] for t in tracks])
    assert (w0 == 0.0).sum() >= 4 and ((w0 != 0) & (np.abs(w0) < 1e-9)).sum() >= 4 and (np.abs(w0) > 0.1).sum() >= 4
    assert np.abs(w0).max() <= 0.6 and (a0 != 0).sum() >= 8
    coupled = [not np.array_equal(t[1], ct.P0) for t in tracks]
    assert sum(coupled) == 20
    for (x0, P0, z), f, cpl in zip(tracks, f64, coupled):
        assert z.dtype == np.float64 and np.isnan(z[0]).all()
        seen = ~np.isnan(z).any(axis=1)
        assert np.array_equal(z[seen], z[seen].astype(np.float32).astype(np.float64))      # float32-valued measurements
        free = x0[4] + PERIOD * np.arange(len(z)) * x0[5]      # the turn rate no measurement ever corrects
        moved = float(np.max(np.abs(f["w"] - free)))
        if cpl and seen.sum() >= 2:      # the state dependence is exercised: the filtered turn rate moves with the data
            assert moved > 1e-5, "coupled P_init, but the filtered turn rate follows w_0 + k T a_0 (%.3g)" % moved
        if not cpl:      # diagonal P0: the turn block stays uncoupled
            assert moved <= 1e-12 * max(1.0, np.abs(free).max())
    assert any(np.isnan(t[2][1:]).any() for t in tracks), "no missed detection in the batch"
    assert max(float(np.abs(f["w"]).max()) for f in f64) < 0.8


def test_reference_recursion_is_self_consistent(batch_refs):
    ct, tracks, truth, f64 = batch_refs
    assert np.finfo(np.longdouble).eps < 1e-18
    assert truth[0]["xs"].dtype == np.longdouble
    e_x = max(sr.err(f["xs"], t["xs"]) for f, t in zip(f64, truth))
    e_P = max(sr.err(f["Ps"], t["Ps"]) for f, t in zip(f64, truth))
    print("float64 reference against longdouble: means %.3g covariances %.3g" % (e_x, e_P))
    assert 0 < e_x < 1e-9 and 0 < e_P < 1e-9
    tr = lambda M: np.trace(M, axis1=1, axis2=2)
    for f in f64:
        assert np.all(tr(f["Ps"]) <= tr(f["Pf"]) * (1 + 1e-9))
        assert np.array_equal(f["xs"][-1], f["xf"][-1]) and np.array_equal(f["Ps"][-1], f["Pf"][-1])
    x0, P0, z = tracks[1]
    one = cr.rts_ct(*cr.model_matrices(ct, PERIOD), x0, P0, z[:1])
    assert np.array_equal(one["xs"][0], x0) and np.array_equal(one["Ps"][0], P0)


def test_straight_tracks_agree_with_the_linear_reference(batch_refs):
    """w = 0, a = 0, diagonal P0: A_k = Phi(T, 0) at every step, so smooth_ref.rts run with ct.Phi(T, 0) (exactly representable: 1, T, 0)
    is the same recursion; the two float64 evaluations agree within their own errors against longdouble."""
    ct, tracks, truth, f64 = batch_refs
    T, Q, Cm, R = cr.model_matrices(ct, PERIOD)
    straight = [i for i, t in enumerate(tracks) if t[0][4] == 0 and t[0][5] == 0 and np.array_equal(t[1], ct.P0)]
    assert len(straight) >= 3
    for i in straight:
        x0, P0, z = tracks[i]
        lin = sr.rts(ct.Phi(PERIOD, 0.0), Q, Cm, R, x0, P0, z, dtype=np.float64)
        lin_t = sr.rts(ct.Phi(PERIOD, 0.0), Q, Cm, R, x0, P0, z, dtype=np.longdouble)
        for key in ("xs", "Ps"):
            own = sr.err(f64[i][key], truth[i][key]) + sr.err(lin[key], lin_t[key])
            assert sr.err(lin_t[key], truth[i][key]) <= 1e-17 * len(z) and sr.err(f64[i][key], lin[key]) <= own


def _host_lib(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    so = str(tmp_path_factory.mktemp("smooth_ct_host") / "libsmooth_ct_host.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "smooth_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.smooth_ct_host.restype = None
    lib.smooth_ct_host.argtypes = [C.c_double] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
    return lib


def _host_smooth(lib, model, x0, P0, z, cov=True):
    T, *mats = cr.model_matrices(model, PERIOD)
    Q, Cm, R = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in mats]
    L = len(z)
    has = sr.detected(z)
    has[0] = False
    zz = np.ascontiguousarray(np.where(has[:, None], z, 0.0))
    hz = np.ascontiguousarray(has.astype(np.uint8))
    x0, P0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(P0, dtype=np.float64)
    xs, Pp = np.full((L, 6), -7.0), np.full((L, 21), -7.0)
    lib.smooth_ct_host(T, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, L, x0.ctypes.data, P0.ctypes.data, zz.ctypes.data, hz.ctypes.data,
                       xs.ctypes.data, Pp.ctypes.data, 1 if cov else 0)
    Ps = np.empty((L, 6, 6))
    iu = np.triu_indices(6)
    Ps[:, iu[0], iu[1]] = Pp
    Ps[:, iu[1], iu[0]] = Pp
    return xs, Ps, Pp


def test_device_arithmetic_on_the_host_meets_the_accuracy_criterion(batch_refs, tmp_path_factory):
    """csrc/mht_smooth_ct_math.h compiled for the host, one track at a time: e <= 8 e_np against the longdouble truth, means and
    covariances separately, as on the device (where the device's own sin / cos take the place of the host's)."""
    ct, tracks, truth, f64 = batch_refs
    lib = _host_lib(tmp_path_factory)
    got = [_host_smooth(lib, ct, *t) for t in tracks]
    e_h = (max(sr.err(g[0], t["xs"]) for g, t in zip(got, truth)), max(sr.err(g[1], t["Ps"]) for g, t in zip(got, truth)))
    e_np = (max(sr.err(f["xs"], t["xs"]) for f, t in zip(f64, truth)), max(sr.err(f["Ps"], t["Ps"]) for f, t in zip(f64, truth)))
    print("host build of the device arithmetic: means e %.3g e_np %.3g ratio %.3g | covariances e %.3g e_np %.3g ratio %.3g"
          % (e_h[0], e_np[0], e_h[0] / e_np[0], e_h[1], e_np[1], e_h[1] / e_np[1]))
    assert e_h[0] <= FACTOR * e_np[0] and e_h[1] <= FACTOR * e_np[1]
    # means only: the same means, bit for bit, and the covariance output untouched; one node: output = input
    x0, P0, z = tracks[3]
    xs_m, _, packed = _host_smooth(lib, ct, x0, P0, z, cov=False)
    assert np.array_equal(xs_m, got[3][0]) and (packed == -7.0).all()
    xs1, Ps1, _ = _host_smooth(lib, ct, x0, P0, z[:1])
    assert np.array_equal(xs1[0], x0) and np.array_equal(Ps1[0], P0)


def test_seam_is_declared_and_exported_by_both_builds():
    from pymht_amd import _lib
    names = _lib.exported_symbols()
    assert "mht_smooth_tracks_ct" in names and "mht_smooth_ct_work_bytes" in names
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        assert hasattr(lib, "mht_smooth_tracks_ct") and hasattr(lib, "mht_smooth_ct_work_bytes"), "the %d-state build does not export the seam" % nx
        # (pure host arithmetic, no GPU) the lengths, then the filtered mean and packed covariance of every node: the linear six-state
        # smoother's workspace -- sin / cos are recomputed in the backward pass, not stored
        assert lib.mht_smooth_ct_work_bytes(2000, 400) == 8192 + 400 * (6 + 21) * 2000 * 8 == lib.mht_smooth_work_bytes(6, 2000, 400)
        assert lib.mht_smooth_ct_work_bytes(3, 5) == 256 + 5 * (6 + 21) * 3 * 8
        assert lib.mht_smooth_ct_work_bytes(-1, 5) == 0 and lib.mht_smooth_ct_work_bytes(3, -1) == 0


def test_linear_model_is_refused_before_anything_runs():
    from pymht_amd.models import pv, ca
    from pymht_amd.smoothing import smooth_tracks_ct
    with pytest.raises(ValueError, match="turn"):
        smooth_tracks_ct(pv, PERIOD, [(np.zeros(4), pv.P0, [None, np.zeros(2)])])
    with pytest.raises(ValueError, match="turn"):
        smooth_tracks_ct(ca, PERIOD, [(np.zeros(6), ca.P0, [None, np.zeros(2)])])


def test_the_keyword_defaults_to_off_everywhere():
    import inspect
    from pymht_amd import smoothing
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    for fn in (smoothing.smooth_nodes, Tracker.getSmoothTracks, Tracker._storeRun, Target.getSmoothTrack):
        assert inspect.signature(fn).parameters["constantTurn"].default is False
