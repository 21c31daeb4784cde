"""CPU: the grid score walk (csrc/mht_smooth_score_grid.h: smooth_score_grid_walk, what a lane of the kernels of
mht_smooth_score_grid.hip runs) compiled for the host next to the score walk, one (track, candidate) at a time; `noise_grid`; the Python
refusals that need no device; the sizer.

A candidate whose matrices a model can carry (power-of-two scalings of its float32 Q and R) must give the score walk's bits: the walk is
that code under another Q and R.  Any other candidate is held to the project's criterion against tests/smooth_score_ref.py evaluated
with the candidate's float64 matrices: e = max |got - truth| / (1 + |truth|) over the batch, e <= 8 max(e_np, eps64), truth the
np.longdouble evaluation, e_np the float64 evaluation's error; ll and nis separately; counts exactly."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import smooth_ref as sr
import smooth_score_grid_ref as gref
import smooth_score_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 2.5


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    so = str(tmp_path_factory.mktemp("smooth_score_grid_host") / "libsmooth_score_grid_host.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "smooth_score_grid_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.smooth_score_lin_host.restype = None
    lib.smooth_score_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 6
    lib.smooth_score_ct_host.restype = None
    lib.smooth_score_ct_host.argtypes = [C.c_double] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 5
    lib.smooth_score_grid_lin_host.restype = None
    lib.smooth_score_grid_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 2 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 5
    lib.smooth_score_grid_ct_host.restype = None
    lib.smooth_score_grid_ct_host.argtypes = [C.c_double, C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 5
    return lib


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _plots(z):
    has = sr.detected(z)
    has[0] = False
    return np.ascontiguousarray(np.where(has[:, None], z, 0.0)), np.ascontiguousarray(has.astype(np.uint8))


def host_grid(lib, model, track, Q, R, ct=False):
    """One track under every candidate through the host build of the grid walk: (ll [G], nis [G], nobs)."""
    x0, P0, z = track
    zz, hz = _plots(z)
    x0, P0, Q, R, A, Cm = _f64(x0), _f64(P0), _f64(Q), _f64(R), _f64(model.Phi(PERIOD)), _f64(model.C_RADAR)
    G = len(Q)
    ll, nis, nobs = np.full(G, -7.0), np.full(G, -7.0), np.full(1, -7, dtype=np.int32)
    tail = (len(z), x0.ctypes.data, P0.ctypes.data, zz.ctypes.data, hz.ctypes.data, G, Q.ctypes.data, R.ctypes.data, ll.ctypes.data, nis.ctypes.data,
            nobs.ctypes.data)
    if ct:
        lib.smooth_score_grid_ct_host(PERIOD, Cm.ctypes.data, *tail)
    else:
        lib.smooth_score_grid_lin_host(A.shape[0], A.ctypes.data, Cm.ctypes.data, *tail)
    return ll, nis, int(nobs[0])


def host_plain(lib, model, track, Qc, Rc, ct=False):
    """One track through the host build of the SCORE walk (smooth_score_lin_host / smooth_score_ct_host) under (Qc, Rc): (ll, nis, nobs)."""
    x0, P0, z = track
    zz, hz = _plots(z)
    x0, P0, Qc, Rc, A, Cm = _f64(x0), _f64(P0), _f64(Qc), _f64(Rc), _f64(model.Phi(PERIOD)), _f64(model.C_RADAR)
    out = np.full(5, -7.0)
    tail = (len(z), x0.ctypes.data, P0.ctypes.data, zz.ctypes.data, hz.ctypes.data)
    if ct:
        lib.smooth_score_ct_host(PERIOD, Qc.ctypes.data, Cm.ctypes.data, Rc.ctypes.data, *tail, out.ctypes.data)
    else:
        lib.smooth_score_lin_host(A.shape[0], A.ctypes.data, Qc.ctypes.data, Cm.ctypes.data, Rc.ctypes.data, *tail, None, out.ctypes.data)
    return out[0], out[1], int(out[2])


def _models():
    from pymht_amd.models import ca, ct, pv
    return {"pv": (pv, "linear"), "ca": (ca, "linear"), "ct": (ct, "ct")}


@pytest.mark.parametrize("name", ["pv", "ca", "ct"])
def test_a_representable_candidate_gives_the_bits_of_the_score_walk(lib, name):
    """The 5 x 5 grid of power-of-two scalings over smooth_score_ref's accuracy batch (33 tracks of 1 .. 60 nodes): every cell
    np.array_equal to the score walk under that candidate's matrices, nObs too; the model's own Q and R are NaN in the policy handed to
    the grid walk, so a walk that read them could not pass."""
    from pymht_amd.smoothing import noise_grid
    model, kind = _models()[name]
    tracks = (ref.linear_batch if kind == "linear" else ref.ct_batch)(model, PERIOD)[0]
    Q, R = noise_grid(model, PERIOD, gref.POW2, gref.POW2)
    assert len(Q) == 25
    for t in tracks:
        ll, nis, nobs = host_grid(lib, model, t, Q, R, ct=kind == "ct")
        plain = [host_plain(lib, model, t, Q[g], R[g], ct=kind == "ct") for g in range(25)]
        assert np.array_equal(ll, np.array([p[0] for p in plain])) and np.array_equal(nis, np.array([p[1] for p in plain]))
        assert all(p[2] == nobs for p in plain)
        assert np.isfinite(ll).all() and (nobs == 0 or len(set(ll.tolist())) > 1)
        if nobs == 0:      # nothing to explain: exactly +0.0 under every candidate
            assert not ll.any() and not nis.any() and not np.signbit(ll).any() and not np.signbit(nis).any()


@pytest.mark.parametrize("name", ["pv", "ca", "ct"])
def test_a_candidate_no_float32_holds_meets_the_accuracy_criterion(lib, name):
    """Scales {0.3, 1.7}^2 (four candidates) on the same batches against the np.longdouble reference under the candidate's float64
    matrices.  Measured, host build (g++ -O2 -mfma), the largest ratio e / max(e_np, eps64) over the four candidates, ll / nis:
        pv 1.01 / 1.00        ca 1.16 / 1.20        ct 1.01 / 1.00
    with e_np between 6.9e-15 and 2.9e-12."""
    model, kind = _models()[name]
    assert np.finfo(np.longdouble).eps < 1e-18
    tracks, Q, R, truth, f64 = gref.reference(kind, model, PERIOD)
    assert not np.array_equal(Q.astype(np.float32).astype(np.float64), Q)
    cols = [host_grid(lib, model, t, Q, R, ct=kind == "ct") for t in tracks]
    ll, nis, nobs = np.array([c[0] for c in cols]).T, np.array([c[1] for c in cols]).T, np.array([c[2] for c in cols])
    worst = gref.hold("host build of the grid walk, models/%s" % name, gref.rows_as_dicts(ll, nis, nobs), truth, f64)
    print("models/%s worst ratio ll %.3g nis %.3g" % (name, worst["ll"], worst["nis"]))


def test_an_indefinite_candidate_gives_nan_in_its_cell_only(lib):
    from pymht_amd.models import pv
    from pymht_amd.smoothing import noise_grid
    (track,) = sr.make_batch(pv, PERIOD, [12], seed=5, p_detect=1.0)
    Q, R = noise_grid(pv, PERIOD, [1.0], [1.0, 2.0, 4.0])
    R[1] = np.diag([-1e9, 1.0])
    ll, nis, nobs = host_grid(lib, pv, track, Q, R)
    assert nobs == 11 and np.isnan(ll[1]) and np.isnan(nis[1]) and np.isfinite(ll[[0, 2]]).all() and np.isfinite(nis[[0, 2]]).all()


def test_noise_grid_orders_and_scales_the_models_float32_matrices():
    from pymht_amd.models import ca, ct, pv
    from pymht_amd.smoothing import _model_x, noise_grid
    qs, rs = [0.3, 1.0, 4.0], [0.5, 1.7]
    for model, nx, turn in ((pv, 4, False), (ca, 6, False), (ct, 6, True)):
        Q, R = noise_grid(model, PERIOD, qs, rs)
        assert Q.shape == (6, nx, nx) and R.shape == (6, 2, 2) and Q.dtype == np.float64 and R.dtype == np.float64
        _, keep = _model_x(model, PERIOD, nx, turn)      # the float32 arrays the library is handed
        Q32, R32 = keep[1].astype(np.float64).reshape(nx, nx), keep[3].astype(np.float64).reshape(2, 2)
        for iq, q in enumerate(qs):
            for ir, r in enumerate(rs):
                assert np.array_equal(Q[iq * 2 + ir], q * Q32) and np.array_equal(R[iq * 2 + ir], r * R32)
        assert np.array_equal(Q[2], Q32) and np.array_equal(Q, Q.transpose(0, 2, 1))
    Q, R = noise_grid(pv, PERIOD, 2.0, np.array([1.0]))
    assert Q.shape == (1, 4, 4) and R.shape == (1, 2, 2)
    for bad in ([], [0.0], [-1.0], [np.nan], [np.inf], [1.0, 0.0]):
        with pytest.raises(ValueError, match="qScales"):
            noise_grid(pv, PERIOD, bad, [1.0])
        with pytest.raises(ValueError, match="rScales"):
            noise_grid(pv, PERIOD, [1.0], bad)


def test_refusals_that_need_no_gpu():
    from pymht_amd.models import ct, pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.smoothing import noise_grid, score_nodes_grid, score_tracks_ct_grid, score_tracks_grid
    track = [(np.zeros(4), pv.P0, [None, np.zeros(2)])]
    ct_track = [(np.zeros(6), ct.P0, [None, np.zeros(2)])]
    Q, R = noise_grid(pv, PERIOD, [1.0, 2.0], [1.0])
    Q6, R6 = noise_grid(ct, PERIOD, [1.0, 2.0], [1.0])
    with pytest.raises(NotImplementedError, match="ct"):
        score_tracks_grid(ct, PERIOD, ct_track, Q6, R6)
    with pytest.raises(ValueError, match="constant-turn"):
        score_tracks_ct_grid(pv, PERIOD, track, Q, R)
    for badQ, badR in ((Q6, R), (Q[0], R[0]), (Q, R[:1]), (Q, np.ones((2, 4))), (Q.reshape(2, 16), R)):
        with pytest.raises(ValueError, match="candidates are"):
            score_tracks_grid(pv, PERIOD, track, badQ, badR)
    with pytest.raises(ValueError, match="candidates a call"):
        score_tracks_grid(pv, PERIOD, track, Q[:0], R[:0])
    with pytest.raises(ValueError, match="candidates a call"):
        score_tracks_grid(pv, PERIOD, track, np.repeat(Q[:1], 4097, axis=0), np.repeat(R[:1], 4097, axis=0))
    skew = Q.copy()
    skew[1, 0, 2] += 1.0
    with pytest.raises(ValueError, match="symmetric"):
        score_tracks_grid(pv, PERIOD, track, skew, R)
    with pytest.raises(ValueError, match="symmetric"):
        score_tracks_grid(pv, PERIOD, track, Q, R + np.array([[0.0, 1.0], [0.0, 0.0]]))
    # nothing to score needs no device
    for score, model, q, r in ((score_tracks_grid, pv, Q, R), (score_tracks_ct_grid, ct, Q6, R6)):
        ll, nis, nobs = score(model, PERIOD, [], q, r)
        assert ll.shape == (2, 0) and nis.shape == (2, 0) and nobs.shape == (0,) and ll.dtype == np.float64 and nobs.dtype == np.int32
    tgt = Target(0.0, None, np.zeros(4), pv.P0)
    ll, nis, nobs = score_nodes_grid(pv, PERIOD, [tgt, tgt], Q, R)      # chains of one node: zeros in their columns
    assert ll.shape == (2, 2) and nis.shape == (2, 2) and not ll.any() and not nis.any() and nobs.tolist() == [0, 0]
    with pytest.raises(NotImplementedError, match="ct"):
        score_nodes_grid(ct, PERIOD, [], Q6, R6)
    with pytest.raises(ValueError, match="constant-turn"):
        score_nodes_grid(pv, PERIOD, [], Q, R, constantTurn=True)
    with pytest.raises(ValueError, match="candidates are"):
        score_nodes_grid(pv, PERIOD, [tgt], Q6, R6)


def test_the_surface_has_no_ais_switch_and_defaults_to_the_live_linear_tracks():
    from pymht_amd.tracker import Tracker
    p = inspect.signature(Tracker.getLikelihoodSurface).parameters
    assert list(p) == ["self", "qScales", "rScales", "terminated", "constantTurn"]
    assert p["terminated"].default is False and p["constantTurn"].default is False
    assert "not scored" in Tracker.getLikelihoodSurface.__doc__.lower()


def test_the_sizer():
    """The lengths and the table [G][nx (nx + 1) / 2 + 3] float64, each rounded up to 256 bytes; 0 for what the seams refuse."""
    from pymht_amd import _lib
    for nx in (4, 6):
        lib = _lib.load(nx=nx)
        size = lib.mht_score_grid_work_bytes
        assert size(4, 3, 5, 1) == 256 + 256 and size(6, 3, 5, 1) == 256 + 256      # 13 and 24 doubles
        assert size(4, 130, 300, 25) == 768 + 2816 and size(6, 130, 300, 25) == 768 + 4864      # 520 | 25 x 104 = 2600, 25 x 192 = 4800
        assert size(6, 2000, 400, 64) == 8192 + 12288 == size(6, 2000, 1, 64)      # (nothing per node)
        assert size(4, 0, 1, 4096) == 4096 * 13 * 8 and size(6, 500, 200, 4096) == 2048 + 4096 * 24 * 8
        assert all(size(nx_, n, L, 1) == lib.mht_score_work_bytes(nx_, n, L) + 256 for nx_, n, L in ((4, 1, 1), (6, 64, 9), (4, 65, 2), (6, 2000, 400)))
        for bad in ((5, 3, 5, 1), (4, -1, 5, 1), (4, 3, -1, 1), (4, 3, 5, 0), (4, 3, 5, -1), (4, 3, 5, 4097)):
            assert size(*bad) == 0, bad
