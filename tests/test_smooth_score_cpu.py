"""CPU: the score walk (csrc/mht_smooth_score.h: smooth_score_walk and smooth_score_walk_theta, what a lane of the kernels of
mht_smooth_score.hip runs) compiled for the host and held to the criterion of tests/test_smooth_score_gpu.py on that test's own
batches, one track at a time; the reference (tests/smooth_score_ref.py) against itself; and the refusals that need no GPU.

Criterion, the smoothers': e = max |got - truth| / (1 + |truth|) over the batch, e <= 8 max(e_np, eps64), truth the np.longdouble
evaluation of the reference and e_np its float64 evaluation's error; ll, nis, nisAis separately; counts exactly.  The measured ratios
are in the docstrings of the tests."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import smooth_ais_ref as ar
import smooth_ct_ref as cr
import smooth_em_ref as er
import smooth_ref as sr
import smooth_score_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 2.5
FACTOR = 8.0


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    so = str(tmp_path_factory.mktemp("smooth_score_host") / "libsmooth_score_host.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "smooth_score_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.smooth_score_lin_host.restype = None
    lib.smooth_score_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 6
    lib.smooth_score_ct_host.restype = None
    lib.smooth_score_ct_host.argtypes = [C.c_double] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 5
    lib.smooth_score_ais_host.restype = None
    lib.smooth_score_ais_host.argtypes = [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 10
    return lib


def _plots(z):
    has = sr.detected(z)
    has[0] = False
    return np.ascontiguousarray(np.where(has[:, None], z, 0.0)), np.ascontiguousarray(has.astype(np.uint8))


def _result(out, ais=False):
    assert out[2] == int(out[2]) and out[4] == int(out[4])
    d = dict(ll=out[0], nis=out[1], nobs=int(out[2]))
    if ais:
        d.update(nis_ais=out[3], nais=int(out[4]))
    return d


def host_score(lib, model, x0, P0, z, start="model", theta=False):
    """One track through smooth_score_lin_host.  theta=True: x0, P0, Q and R travel per track in the EM workspace's layout and the
    arguments in their place are poisoned."""
    Q, R, P = er.start_values(model, PERIOD, P0, start)
    A, Q, Cm, R = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in (model.Phi(PERIOD), Q, model.C_RADAR, R)]
    nx = A.shape[0]
    zz, hz = _plots(z)
    x0, P = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(P, dtype=np.float64)
    out = np.full(5, -7.0)
    th = None
    if theta:
        iu = np.triu_indices(nx)
        th = np.ascontiguousarray(np.concatenate([x0, P[iu], Q[iu], R.ravel()[[0, 1, 3]]]))
        x0, P, Q, R = [np.full_like(a, np.nan) for a in (x0, P, Q, R)]
    lib.smooth_score_lin_host(nx, A.ctypes.data, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, len(z), x0.ctypes.data, P.ctypes.data, zz.ctypes.data,
                              hz.ctypes.data, None if th is None else th.ctypes.data, out.ctypes.data)
    return _result(out)


def host_score_ct(lib, model, x0, P0, z):
    T, Q, Cm, R = cr.model_matrices(model, PERIOD)
    Q, Cm, R = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in (Q, Cm, R)]
    zz, hz = _plots(z)
    x0, P0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(P0, dtype=np.float64)
    out = np.full(5, -7.0)
    lib.smooth_score_ct_host(T, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, len(z), x0.ctypes.data, P0.ctypes.data, zz.ctypes.data, hz.ctypes.data,
                             out.ctypes.data)
    return _result(out)


def host_score_ais(lib, model, x0, P0, z, ais):
    """Inputs packed by the Python layer's own host-side code (smoothing._ais_inputs)."""
    from pymht_amd.smoothing import _ais_inputs
    A, Q, Cm, R = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in sr.model_matrices(model, PERIOD)]
    ((has_m, msg, r, leg),), legs = _ais_inputs(model, [(x0, P0, z, ais)])
    zz, hz = _plots(z)
    kind = np.ascontiguousarray(hz + 2 * has_m.astype(np.uint8))
    msg, r, leg, legs = [np.ascontiguousarray(a) for a in (msg, r, leg, legs)]
    x0, P0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(P0, dtype=np.float64)
    out = np.full(5, -7.0)
    lib.smooth_score_ais_host(A.ctypes.data, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, len(z), x0.ctypes.data, P0.ctypes.data, zz.ctypes.data,
                              hz.ctypes.data, kind.ctypes.data, msg.ctypes.data, r.ctypes.data, leg.ctypes.data, legs.ctypes.data, out.ctypes.data)
    return _result(out, ais=True)


def _hold(label, got, truth, f64, names):
    res = ref.ratios(got, truth, f64, names)
    print(label + ": " + " | ".join("%s e %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, (k, e, e_np, ratio)
    for g, t in zip(got, truth):
        assert g["nobs"] == t["nobs"] and g.get("nais", 0) == t["nais"]


def _exact_zero(r):
    assert r["ll"] == 0.0 and r["nis"] == 0.0 and r["nobs"] == 0 and not np.signbit(r["ll"]) and not np.signbit(r["nis"])


@pytest.mark.parametrize("start", ["model", "reference"])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_linear_score_walk_on_the_host_meets_the_accuracy_criterion(lib, name, start):
    """smooth_em_ref.accuracy_batch, 33 tracks of 1 .. 60 nodes.  Measured, host build (g++ -O2 -mfma), ratios e / max(e_np, eps64)
    for ll / nis, with e_np between 1.2e-14 and 3.0e-13:
        pv, start=model       1.00 / 1.00          pv, start=reference   1.00 / 1.00
        ca, start=model       1.00 / 1.00          ca, start=reference   1.11 / 1.10
    The per-track theta walk gives the same bits as the walk under the call's arguments (asserted)."""
    from pymht_amd.models import pv, ca
    model = {"pv": pv, "ca": ca}[name]
    assert np.finfo(np.longdouble).eps < 1e-18
    tracks, truth, f64 = ref.reference("linear", model, PERIOD, start)
    _, one, never, always = ref.linear_batch(model, PERIOD)
    got = [host_score(lib, model, *t, start=start) for t in tracks]
    _hold("host build of the score walk, models/%s, start=%s" % (name, start), got, truth, f64, ("ll", "nis"))
    _exact_zero(got[one])
    _exact_zero(got[never])
    assert got[always]["nobs"] == len(tracks[always][2]) - 1 and got[always]["ll"] < 0.0 < got[always]["nis"]
    for t, g in zip(tracks, got):
        assert host_score(lib, model, *t, start=start, theta=True) == g


def test_constant_turn_score_walk_on_the_host_meets_the_accuracy_criterion(lib):
    """A smooth_ct_ref.make_batch of the linear batch's lengths.  Measured, host build: ll e 2.59e-14 e_np 2.61e-14 ratio 0.99 |
    nis e 1.13e-13 e_np 1.13e-13 ratio 1.00."""
    from pymht_amd.models import ct
    tracks, truth, f64 = ref.reference("ct", ct, PERIOD)
    _, one, never, always = ref.ct_batch(ct, PERIOD)
    got = [host_score_ct(lib, ct, *t) for t in tracks]
    _hold("host build of the score walk, models/ct", got, truth, f64, ("ll", "nis"))
    _exact_zero(got[one])
    _exact_zero(got[never])
    assert got[always]["nobs"] == len(tracks[always][2]) - 1


def test_ais_score_walk_on_the_host_meets_the_accuracy_criterion(lib):
    """smooth_ais_ref.accuracy_batch, 40 tracks of 2 .. 400 nodes.  Measured, host build: ll e 1.04e-14 e_np 6.22e-15 ratio 1.67 |
    nis e 6.88e-14 e_np 6.84e-14 ratio 1.01 | nis_ais e 6.32e-14 e_np 6.25e-14 ratio 1.01."""
    model, tracks = ar.accuracy_batch()
    tracks, truth, f64 = ref.reference("ais", model, PERIOD)
    got = [host_score_ais(lib, model, *t) for t in tracks]
    _hold("host build of the score walk, AIS", got, truth, f64, ("ll", "nis", "nis_ais"))
    assert sum(g["nais"] for g in got) > 1000
    # without its messages a track is the linear walk's, bit for bit, and nothing is counted as a message
    x0, P0, z, ais = tracks[3]
    plain = host_score_ais(lib, model, x0, P0, z, [None] * len(z))
    lin = host_score(lib, model, x0, P0, z)
    assert (plain["ll"], plain["nis"], plain["nobs"]) == (lin["ll"], lin["nis"], lin["nobs"]) and plain["nais"] == 0 and plain["nis_ais"] == 0.0
    _exact_zero(host_score_ais(lib, model, x0, P0, z[:1], ais[:1]))


def test_a_model_that_is_no_covariance_gives_nan_not_a_number_that_looks_fine(lib):
    """det S <= 0: NaN in ll and nis, the count still counted."""
    from pymht_amd.models import pv

    class Broken:
        Phi, C_RADAR, Q = staticmethod(pv.Phi), pv.C_RADAR, staticmethod(pv.Q)
        R_RADAR = staticmethod(lambda: np.diag([-1e9, 1.0]))
    (x0, P0, z), = sr.make_batch(pv, PERIOD, [12], seed=5, p_detect=1.0)
    r = host_score(lib, Broken, x0, P0, z)
    assert np.isnan(r["ll"]) and np.isnan(r["nis"]) and r["nobs"] == 11


def test_reference_is_self_consistent():
    """tests/smooth_score_ref.py alone: float64 against longdouble below 1e-9; no measurement, no score; an AIS batch without messages
    is the linear score; the score's filter is smooth_ref.rts's (its last filtered state reproduces the last term)."""
    from pymht_amd.models import ca, ct, pv
    assert np.finfo(np.longdouble).eps < 1e-18
    for kind, model in (("linear", pv), ("linear", ca), ("ct", ct), ("ais", pv)):
        tracks, truth, f64 = ref.reference(kind, model, PERIOD)
        assert truth[0]["ll"].dtype == np.longdouble
        res = ref.ratios(f64, truth, f64, ("ll", "nis", "nis_ais"))
        print(kind, model.__name__, {k: v[0] for k, v in res.items()})
        for k, (e, _, _) in res.items():
            assert np.isfinite(e) and e < 1e-9, (kind, k, e)
        assert 0 < res["ll"][0] and 0 < res["nis"][0]
        assert all(t["nobs"] == f["nobs"] and t["nais"] == f["nais"] for t, f in zip(truth, f64))
    mats = sr.model_matrices(pv, PERIOD)
    for dtype in (np.float64, np.longdouble):
        for x0, P0, z in sr.make_batch(pv, PERIOD, [1, 2, 37, 150], seed=4):
            lin = ref.score(*mats, x0, P0, z, dtype=dtype)
            a = ref.score_ais(pv, PERIOD, x0, P0, z, [None] * len(z), dtype=dtype)
            assert a == lin and (lin["nobs"] > 0 or len(z) < 3)
            blind = ref.score(*mats, x0, P0, np.full_like(z, np.nan), dtype=dtype)
            assert blind["ll"] == 0 and blind["nis"] == 0 and blind["nobs"] == 0
    # the textbook figure: 2 x 2, one plot -- ln N(v; 0, S) written out
    (x0, P0, z), = sr.make_batch(pv, PERIOD, [2], seed=9, p_detect=1.0)
    A, Q, Cm, R = [np.asarray(m, dtype=np.float64) for m in mats]
    Pp = A @ P0 @ A.T + Q
    S = Cm @ Pp @ Cm.T + R
    v = z[1] - Cm @ A @ x0
    one = ref.score(*mats, x0, P0, z)
    assert one["nobs"] == 1 and abs(one["nis"] - v @ np.linalg.solve(S, v)) < 1e-9 * (1 + one["nis"])
    assert abs(one["ll"] + 0.5 * (np.log(np.linalg.det(S)) + one["nis"] + 2 * np.log(2 * np.pi))) < 1e-9 * (1 + abs(one["ll"]))


@pytest.mark.parametrize("start", ["model", "reference"])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_the_longdouble_em_trace_never_decreases(name, start):
    """EM's defining property, on the reference alone: five iterations on smooth_em_ref.accuracy_batch, every value finite, no decrease
    on any track; a one-node track has equal rows; row 0 is the score under the start values."""
    from pymht_amd.models import pv, ca
    model = {"pv": pv, "ca": ca}[name]
    tracks, truth, f64 = ref.trace_reference(model, PERIOD, start)
    _, one, never, always = er.accuracy_batch(model, PERIOD)
    _, score_truth, _ = ref.reference("linear", model, PERIOD, start)
    for i, (ll, s) in enumerate(zip(truth, score_truth)):
        assert ll.shape == (6,) and ll.dtype == np.longdouble and np.isfinite(ll).all()
        assert (np.diff(ll) >= 0).all(), (i, ll)
        assert ll[0] == s["ll"]
    assert (truth[one] == 0).all() and (truth[never] == 0).all()
    rows = ref.trace_ratios(f64, truth, f64)
    print("float64 trace against longdouble, models/%s, start=%s: " % (name, start) + " ".join("%.3g" % r[0] for r in rows))
    assert all(r[0] < 1e-9 for r in rows)
    assert any(ll[5] > ll[0] for ll in truth)


def test_refusals_that_need_no_gpu():
    from pymht_amd.models import ca, ct, pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.smoothing import score_nodes, score_tracks, score_tracks_ais, score_tracks_ct, smooth_tracks_em
    track = [(np.zeros(4), pv.P0, [None, np.zeros(2)])]
    ct_track = [(np.zeros(6), ct.P0, [None, np.zeros(2)])]
    with pytest.raises(NotImplementedError, match="ct"):
        score_tracks(ct, PERIOD, ct_track)
    with pytest.raises(ValueError, match="constant-turn"):
        score_tracks_ct(pv, PERIOD, track)
    for model, nx in ((ca, 6), (ct, 6)):
        with pytest.raises(ValueError, match="4-state linear"):
            score_tracks_ais(model, PERIOD, [(np.zeros(nx), model.P0, [None, np.zeros(2)], [None, (1.0, 1.5, np.zeros(4), True)])])
    with pytest.raises(ValueError, match="positive"):
        score_tracks_ais(pv, PERIOD, [(np.zeros(4), pv.P0, [None, np.zeros(2)], [None, (0.0, 2.5, np.zeros(4), True)])])
    assert score_tracks(pv, PERIOD, []) == [] and score_tracks_ct(ct, PERIOD, []) == [] and score_tracks_ais(pv, PERIOD, []) == []
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(TypeError, match="likelihoods"):
            smooth_tracks_em(pv, PERIOD, track, likelihoods=bad)
    with pytest.raises(NotImplementedError, match="ct"):
        smooth_tracks_em(ct, PERIOD, ct_track, likelihoods=True)
    tgt = Target(0.0, None, np.zeros(4), pv.P0)
    with pytest.raises(ValueError, match="constantTurn"):
        score_nodes(pv, PERIOD, [tgt], constantTurn=True, ais=lambda scan, mmsi: None)
    with pytest.raises(NotImplementedError, match="ct"):
        score_nodes(ct, PERIOD, [])
    with pytest.raises(ValueError, match="constant-turn"):
        score_nodes(pv, PERIOD, [], constantTurn=True)
    with pytest.raises(ValueError, match="Tracker"):
        tgt.getTrackLikelihood(PERIOD, ais=True)
    # a chain of one node has nothing to explain, and needs no device to say so
    assert score_nodes(pv, PERIOD, [tgt]) == [(0.0, 0.0, 0)] and tgt.getTrackLikelihood(PERIOD) == (0.0, 0.0, 0)
    assert score_nodes(pv, PERIOD, [tgt], ais=lambda scan, mmsi: None) == [(0.0, 0.0, 0, 0.0, 0)]


def test_the_new_keywords_default_to_off():
    from pymht_amd import smoothing
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    assert inspect.signature(smoothing.smooth_tracks_em).parameters["likelihoods"].default is False
    assert inspect.signature(smoothing.score_nodes).parameters["ais"].default is None
    for fn in (Tracker.getTrackLikelihoods, Target.getTrackLikelihood):
        p = inspect.signature(fn).parameters
        assert p["ais"].default is False and p["constantTurn"].default is False
