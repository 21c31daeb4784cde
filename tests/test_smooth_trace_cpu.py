"""CPU: the trace walk (csrc/mht_smooth_trace.h: smooth_trace_walk, what a lane of the kernels of mht_smooth_trace.hip runs) compiled for
the host and held to the criterion of tests/test_smooth_trace_gpu.py on that test's own batches, one track at a time; its sums against
the host twin of the score walk, bit for bit; the reference (tests/smooth_trace_ref.py) against itself; the host-side consistency
statistics (pymht_amd.smoothing.consistency) on the reference's traces; and the refusals that need no GPU.

Criterion, the smoothers': per output family (v, S, nis, ll, and vAis, SAis, nisAis, llAis) e = max |got - truth| / (1 + |truth|) over
the cells of the batch that are not NaN in the truth, e <= 8 max(e_np, eps64), truth the np.longdouble evaluation of the reference and
e_np its float64 evaluation's error; the NaN cells are the truth's exactly.  The measured ratios are in the docstrings of the tests."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import smooth_ct_ref as cr
import smooth_em_ref as er
import smooth_ref as sr
import smooth_score_ref as score_ref
import smooth_trace_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 2.5
FACTOR = 8.0
TAIL = 3            # rows the host arrays have behind a track's end: the walk writes them too
SENTINEL = -7.0


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(the host build of the trace walk, the host build of the score walk)"""
    gxx = shutil.which("g++") or "g++"
    out = []
    for name in ("smooth_trace_host", "smooth_score_host"):
        so = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                               os.path.join(ROOT, "tests", "hostmath", name + ".cpp"), "-o", so])
        out.append(C.CDLL(so))
    trace, score = out
    trace.smooth_trace_lin_host.restype = None
    trace.smooth_trace_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] * 2 + [C.c_void_p] * 5
    trace.smooth_trace_ct_host.restype = None
    trace.smooth_trace_ct_host.argtypes = [C.c_double] + [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p] * 5
    trace.smooth_trace_ais_host.restype = None
    trace.smooth_trace_ais_host.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 2 + [C.c_void_p] * 11
    score.smooth_score_lin_host.restype = None
    score.smooth_score_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 6
    score.smooth_score_ct_host.restype = None
    score.smooth_score_ct_host.argtypes = [C.c_double] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 5
    score.smooth_score_ais_host.restype = None
    score.smooth_score_ais_host.argtypes = [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 10
    return trace, score


def _f64(*arrays):
    return [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in arrays]


def _padded(z, rows):
    """(z [rows, 2] with zeros where there is no plot, has_z [rows]) for a track of len(z) nodes in arrays of `rows` rows"""
    has = sr.detected(z)
    has[0] = False
    zz, hz = np.zeros((rows, 2)), np.zeros(rows, dtype=np.uint8)
    zz[:len(z)] = np.where(has[:, None], np.asarray(z, dtype=np.float64), 0.0)
    hz[:len(z)] = has
    return zz, hz


def _finish(L, radar, hz, ais=None, message=None):
    """The host arrays as the Python layer's dict (pymht_amd.smoothing._trace_dict); no sentinel is left, and the rows behind the
    track's end are NaN."""
    from pymht_amd.smoothing import _trace_dict
    for a in (radar,) + (() if ais is None else (ais,)):
        assert not (a == SENTINEL).any() and np.isnan(a[L:]).all()
    return _trace_dict(radar[:L], hz[:L], None if ais is None else ais[:L], message)


def host_trace(libs, model, x0, P0, z):
    Q, R, P = er.start_values(model, PERIOD, P0, "model")
    A, Q, Cm, R, x0, P = _f64(model.Phi(PERIOD), Q, model.C_RADAR, R, x0, P)
    L, rows = len(z), len(z) + TAIL
    zz, hz = _padded(z, rows)
    radar = np.full((rows, 7), SENTINEL)
    libs[0].smooth_trace_lin_host(A.shape[0], A.ctypes.data, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, L, rows, x0.ctypes.data, P.ctypes.data,
                                  zz.ctypes.data, hz.ctypes.data, radar.ctypes.data)
    out = np.full(5, SENTINEL)
    libs[1].smooth_score_lin_host(A.shape[0], A.ctypes.data, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, L, x0.ctypes.data, P.ctypes.data,
                                  zz.ctypes.data, hz.ctypes.data, None, out.ctypes.data)
    return _finish(L, radar, hz), out


def host_trace_ct(libs, model, x0, P0, z):
    T, Q, Cm, R = cr.model_matrices(model, PERIOD)
    Q, Cm, R, x0, P0 = _f64(Q, Cm, R, x0, P0)
    L, rows = len(z), len(z) + TAIL
    zz, hz = _padded(z, rows)
    radar = np.full((rows, 7), SENTINEL)
    libs[0].smooth_trace_ct_host(T, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, L, rows, x0.ctypes.data, P0.ctypes.data, zz.ctypes.data,
                                 hz.ctypes.data, radar.ctypes.data)
    out = np.full(5, SENTINEL)
    libs[1].smooth_score_ct_host(T, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, L, x0.ctypes.data, P0.ctypes.data, zz.ctypes.data, hz.ctypes.data,
                                 out.ctypes.data)
    return _finish(L, radar, hz), out


def host_trace_ais(libs, model, x0, P0, z, ais):
    """Inputs packed by the Python layer's own host-side code (smoothing._ais_inputs)."""
    from pymht_amd.smoothing import _ais_inputs
    A, Q, Cm, R, x0, P0 = _f64(*sr.model_matrices(model, PERIOD), x0, P0)
    ((has_m, msg, r, leg),), legs = _ais_inputs(model, [(x0, P0, z, ais)])
    L, rows = len(z), len(z) + TAIL
    zz, hz = _padded(z, rows)
    kind, mm, rr, ll = hz.copy(), np.zeros((rows, 4)), np.ones(rows), np.zeros(rows, dtype=np.int32)
    kind[:L] += 2 * has_m.astype(np.uint8)
    mm[:L], rr[:L], ll[:L] = msg, r, leg
    legs = np.ascontiguousarray(legs)
    radar, aout = np.full((rows, 7), SENTINEL), np.full((rows, 16), SENTINEL)
    libs[0].smooth_trace_ais_host(A.ctypes.data, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, L, rows, x0.ctypes.data, P0.ctypes.data, zz.ctypes.data,
                                  hz.ctypes.data, kind.ctypes.data, mm.ctypes.data, rr.ctypes.data, ll.ctypes.data, legs.ctypes.data,
                                  radar.ctypes.data, aout.ctypes.data)
    out = np.full(5, SENTINEL)
    libs[1].smooth_score_ais_host(A.ctypes.data, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, L, x0.ctypes.data, P0.ctypes.data, zz.ctypes.data,
                                  hz.ctypes.data, kind.ctypes.data, mm.ctypes.data, rr.ctypes.data, ll.ctypes.data, legs.ctypes.data, out.ctypes.data)
    return _finish(L, radar, hz, aout, has_m), out


def _hold(label, got, truth, f64, names):
    res = ref.ratios(got, truth, f64, names)
    print(label + ": " + " | ".join("%s e %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert ref.same_nan(got, truth, names), "the NaN cells are not the truth's"
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, (k, e, e_np, ratio)


def _sums_are_the_score(tr, score):
    """The trace added up in node order against the host score twin's out [5] (ll, nis, nObs, nisAis, nAis): the same bits"""
    s = ref.resum(tr)
    assert tr["ll"].dtype == np.float64
    want = np.array([s["ll"], s["nis"], s["nobs"]] + ([s["nis_ais"], s["nais"]] if "message" in tr else []), dtype=np.float64)
    assert np.array_equal(want, score[:len(want)]), (want, score)


@pytest.mark.parametrize("name", ["pv", "ca"])
def test_linear_trace_walk_on_the_host_meets_the_accuracy_criterion(libs, name):
    """smooth_em_ref.accuracy_batch, 33 tracks of 1 .. 60 nodes.  Measured, host build (g++ -O2 -mfma), ratios e / max(e_np, eps64) for
    v / S / nis / ll:
        pv   1.00 / 0.51 / 1.00 / 1.00   (e_np 2.4e-12 / 3.2e-15 / 3.9e-13 / 6.6e-14)
        ca   0.91 / 2.31 / 0.75 / 1.00   (e_np 4.1e-12 / 4.9e-15 / 6.4e-13 / 1.4e-13)
    Every track's ll and nis added up in node order are the host score twin's bits, its observed nodes that twin's nObs."""
    from pymht_amd.models import pv, ca
    model = {"pv": pv, "ca": ca}[name]
    assert np.finfo(np.longdouble).eps < 1e-18
    tracks, truth, f64 = ref.reference("linear", model, PERIOD)
    _, one, never, always = er.accuracy_batch(model, PERIOD)
    both = [host_trace(libs, model, *t) for t in tracks]
    got = [b[0] for b in both]
    _hold("host build of the trace walk, models/%s" % name, got, truth, f64, ref.RADAR)
    for tr, score in both:
        _sums_are_the_score(tr, score)
    assert len(got[one]["ll"]) == 1 and not got[one]["observed"].any() and not got[never]["observed"].any()
    assert got[always]["observed"][1:].all() and not got[always]["observed"][0] and (got[always]["ll"][1:] < 0).all()
    assert all(np.array_equal(g["S"], g["S"].transpose(0, 2, 1), equal_nan=True) for g in got)


def test_constant_turn_trace_walk_on_the_host_meets_the_accuracy_criterion(libs):
    """A smooth_ct_ref.make_batch of the linear batch's lengths.  Measured, host build: v e 3.31e-12 e_np 3.31e-12 ratio 1.00 |
    S e 9.13e-14 e_np 6.75e-14 ratio 1.35 | nis e 1.36e-12 e_np 1.36e-12 ratio 1.00 | ll e 1.28e-13 e_np 1.27e-13 ratio 1.00."""
    from pymht_amd.models import ct
    tracks, truth, f64 = ref.reference("ct", ct, PERIOD)
    both = [host_trace_ct(libs, ct, *t) for t in tracks]
    _hold("host build of the trace walk, models/ct", [b[0] for b in both], truth, f64, ref.RADAR)
    for tr, score in both:
        _sums_are_the_score(tr, score)


def test_ais_trace_walk_on_the_host_meets_the_accuracy_criterion(libs):
    """smooth_ais_ref.accuracy_batch cut to at most 60 nodes a track (40 tracks).  Measured, host build, ratios for v / S / nis / ll /
    vAis / SAis / nisAis / llAis: 0.81 / 0.45 / 1.19 / 1.05 / 1.11 / 0.42 / 1.00 / 1.28 (e_np 3.1e-12 / 2.9e-14 / 5.6e-13 / 1.9e-13 /
    1.5e-12 / 1.0e-14 / 6.2e-13 / 1.0e-13).  llAis in front of ll at a node with both, the sums are the host score twin's bits; without
    its messages a track is the linear trace, bit for bit."""
    model, tracks = ref.ais_batch()
    tracks, truth, f64 = ref.reference("ais", model, PERIOD)
    assert max(len(t[2]) for t in tracks) == 60
    both = [host_trace_ais(libs, model, *t) for t in tracks]
    got = [b[0] for b in both]
    _hold("host build of the trace walk, AIS", got, truth, f64, ref.RADAR + ref.AIS)
    for tr, score in both:
        _sums_are_the_score(tr, score)
    assert sum(int(g["message"].sum()) for g in got) > 300 and any((g["message"] & g["observed"]).any() for g in got)
    assert all(np.array_equal(g["SAis"], g["SAis"].transpose(0, 2, 1), equal_nan=True) for g in got)
    x0, P0, z, ais = tracks[3]
    plain, _ = host_trace_ais(libs, model, x0, P0, z, [None] * len(z))
    lin, _ = host_trace(libs, model, x0, P0, z)
    assert all(np.array_equal(plain[k], lin[k], equal_nan=True) for k in ref.RADAR + ("observed",))
    assert not plain["message"].any() and all(np.isnan(plain[k]).all() for k in ref.AIS)


def test_a_model_that_is_no_covariance_gives_nan_at_its_nodes_and_keeps_v_and_s(libs):
    """det S <= 0 at every plot: NaN in nis and ll of the observed nodes, v and S finite there; the score twin's sums are NaN."""
    from pymht_amd.models import pv

    class Broken:
        Phi, C_RADAR, Q = staticmethod(pv.Phi), pv.C_RADAR, staticmethod(pv.Q)
        R_RADAR = staticmethod(lambda: np.diag([-1e9, 1.0]))
    (x0, P0, z), = sr.make_batch(pv, PERIOD, [12], seed=5, p_detect=1.0)
    tr, score = host_trace(libs, Broken, x0, P0, z)
    obs = tr["observed"]
    assert obs.sum() == 11 and np.isnan(tr["nis"]).all() and np.isnan(tr["ll"]).all()
    assert np.isfinite(tr["v"][obs]).all() and np.isfinite(tr["S"][obs]).all() and np.isnan(tr["v"][~obs]).all()
    assert np.isnan(score[0]) and np.isnan(score[1]) and score[2] == 11


def test_reference_is_self_consistent():
    """tests/smooth_trace_ref.py alone: float64 against longdouble below 1e-9 per family; the NaN cells agree; a trace added up in
    node order is smooth_score_ref's score in the same dtype, exactly; the textbook figure for one plot."""
    from pymht_amd.models import ca, ct, pv
    assert np.finfo(np.longdouble).eps < 1e-18
    for kind, model in (("linear", pv), ("linear", ca), ("ct", ct), ("ais", pv)):
        names = ref.RADAR + (ref.AIS if kind == "ais" else ())
        tracks, truth, f64 = ref.reference(kind, model, PERIOD)
        assert truth[0]["ll"].dtype == np.longdouble and ref.same_nan(f64, truth, names)
        res = ref.ratios(f64, truth, f64, names)
        print(kind, model.__name__, {k: v[0] for k, v in res.items()})
        assert all(np.isfinite(e) and 0 < e < 1e-9 for e, _, _ in res.values())
    mats = sr.model_matrices(pv, PERIOD)
    for dtype in (np.float64, np.longdouble):
        for x0, P0, z in sr.make_batch(pv, PERIOD, [1, 2, 37], seed=4):
            tr = ref.trace(*mats, x0, P0, z, dtype=dtype)
            assert ref.resum(tr) == score_ref.score(*mats, x0, P0, z, dtype=dtype)
            a = ref.trace_ais(pv, PERIOD, x0, P0, z, [None] * len(z), dtype=dtype)
            assert all(np.array_equal(a[k], tr[k], equal_nan=True) for k in ref.RADAR) and not a["message"].any()
    model, tracks = ref.ais_batch()
    for t in tracks[:5]:
        assert ref.resum(ref.trace_ais(model, PERIOD, *t)) == score_ref.score_ais(model, PERIOD, *t)
    (x0, P0, z), = sr.make_batch(pv, PERIOD, [2], seed=9, p_detect=1.0)
    A, Q, Cm, R = [np.asarray(m, dtype=np.float64) for m in mats]
    S = Cm @ (A @ P0 @ A.T + Q) @ Cm.T + R
    v = z[1] - Cm @ A @ x0
    one = ref.trace(*mats, x0, P0, z)
    assert np.allclose(one["v"][1], v, rtol=1e-12) and np.allclose(one["S"][1], S, rtol=1e-12) and np.isnan(one["v"][0]).all()
    assert abs(one["nis"][1] - v @ np.linalg.solve(S, v)) < 1e-9 * (1 + one["nis"][1])
    assert abs(one["ll"][1] + 0.5 * (np.log(np.linalg.det(S)) + one["nis"][1] + 2 * np.log(2 * np.pi))) < 1e-9 * (1 + abs(one["ll"][1]))


CONSISTENCY_SEED = 1


def _scaled(model, q=1.0, r=1.0):
    class Scaled:
        __name__ = "scaled"
        Phi, C_RADAR, P0 = staticmethod(model.Phi), model.C_RADAR, model.P0
        Q = staticmethod(lambda T: q * np.asarray(model.Q(T), dtype=np.float64))
        R_RADAR = staticmethod(lambda: r * np.asarray(model.R_RADAR(), dtype=np.float64))
    return Scaled


def test_consistency_tells_a_matched_filter_from_a_mistuned_one():
    """pymht_amd.smoothing.consistency on the float64 reference's traces of ONE batch simulated from models/pv's own Phi, Q, R
    (smooth_trace_ref.simulate: 40 tracks of 50 nodes, seed 1, detection probability 0.9; seeds 1 .. 15 were looked at on the CPU and
    all fifteen give the three verdicts, seed 1 with the most room).  Observed, alpha = 0.05:
        matched      nObs 1772  nisMean 1.985 in (1.908, 2.094)  outlierFraction 0.0474  rho1 -0.0093  bound 0.0350 (nPairs 1569)
        R x 4        nisMean 1.154, below the interval (rho1 0.312: the innovations of a sluggish filter are correlated too)
        Q / 100      nisMean 35.6, far above the interval; rho1 0.829, far outside its bound
    The outlier share of the matched filter lies within three binomial standard deviations of alpha for the batch's nObs."""
    from pymht_amd.models import pv
    from pymht_amd.smoothing import consistency
    alpha = 0.05
    tracks = ref.simulate(pv, PERIOD, 40, 50, CONSISTENCY_SEED)
    assert len(tracks) == 40 and all(len(t[2]) == 50 for t in tracks)

    def run(model):
        mats = sr.model_matrices(model, PERIOD)
        c = consistency([ref.trace(*mats, *t) for t in tracks], alpha=alpha)
        print({k: v for k, v in c.items()})
        return c
    matched, big_r, small_q = run(pv), run(_scaled(pv, r=4.0)), run(_scaled(pv, q=0.01))
    assert matched["nObs"] == big_r["nObs"] == small_q["nObs"] > 1500 and matched["nPairs"] > 1200
    assert matched["nisInside"] is True and matched["white"] is True
    lo, hi = matched["nisInterval"]
    assert lo < 2.0 < hi and lo + 0.25 * (hi - lo) < matched["nisMean"] < hi - 0.25 * (hi - lo)      # (with room)
    assert abs(matched["rho1"]) < 0.5 * matched["rho1Bound"]
    sigma = np.sqrt(alpha * (1 - alpha) / matched["nObs"])      # the share of nObs Bernoulli(alpha) draws
    assert abs(matched["outlierFraction"] - alpha) <= 3 * sigma
    assert big_r["nisInside"] is False and big_r["nisMean"] < big_r["nisInterval"][0]
    assert small_q["white"] is False and small_q["rho1"] > small_q["rho1Bound"]
    assert small_q["nisInside"] is False and small_q["nisMean"] > small_q["nisInterval"][1]


def test_consistency_of_degenerate_inputs_and_bad_alpha():
    from pymht_amd.smoothing import _blank_trace, consistency
    for traces in ([], [_blank_trace(1)], [_blank_trace(5, ais=True)]):
        c = consistency(traces)
        assert c["nObs"] == 0 and c["nPairs"] == 0 and c["nisInside"] is None and c["white"] is None
        assert all(np.isnan(c[k]) for k in ("nisMean", "outlierFraction", "rho1", "rho1Bound")) and np.isnan(c["nisInterval"]).all()
    # observed nodes, none of them next to another: the NIS test stands, the whiteness test has nothing to say
    from pymht_amd.models import pv
    mats = sr.model_matrices(pv, PERIOD)
    (x0, P0, z), = sr.make_batch(pv, PERIOD, [9], seed=3, p_detect=1.0)
    z[2::2] = np.nan
    tr = ref.trace(*mats, x0, P0, z)
    c = consistency([tr])
    assert c["nObs"] == 4 and c["nPairs"] == 0 and c["white"] is None and np.isnan(c["rho1"]) and np.isfinite(c["nisMean"])
    assert c["nisInside"] in (True, False) and abs(c["nisMean"] - tr["nis"][tr["observed"]].sum() / 4) < 1e-12
    # a poisoned node: NaN, not a verdict
    bad = {k: v.copy() for k, v in tr.items()}
    bad["nis"][1] = np.nan
    c = consistency([bad])
    assert c["nObs"] == 4 and np.isnan(c["nisMean"]) and c["nisInside"] is None
    for alpha in (0.0, 1.0, -0.1, 1.5, float("nan"), None, "0.05", True):
        with pytest.raises(ValueError, match="alpha"):
            consistency([tr], alpha=alpha)


def test_refusals_that_need_no_gpu():
    from pymht_amd.models import ca, ct, pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.smoothing import trace_nodes, trace_tracks, trace_tracks_ais, trace_tracks_ct
    track = [(np.zeros(4), pv.P0, [None, np.zeros(2)])]
    ct_track = [(np.zeros(6), ct.P0, [None, np.zeros(2)])]
    with pytest.raises(NotImplementedError, match="ct"):
        trace_tracks(ct, PERIOD, ct_track)
    with pytest.raises(ValueError, match="constant-turn"):
        trace_tracks_ct(pv, PERIOD, track)
    for model, nx in ((ca, 6), (ct, 6)):
        with pytest.raises(ValueError, match="4-state linear"):
            trace_tracks_ais(model, PERIOD, [(np.zeros(nx), model.P0, [None, np.zeros(2)], [None, (1.0, 1.5, np.zeros(4), True)])])
    with pytest.raises(ValueError, match="positive"):
        trace_tracks_ais(pv, PERIOD, [(np.zeros(4), pv.P0, [None, np.zeros(2)], [None, (0.0, 2.5, np.zeros(4), True)])])
    assert trace_tracks(pv, PERIOD, []) == [] and trace_tracks_ct(ct, PERIOD, []) == [] and trace_tracks_ais(pv, PERIOD, []) == []
    tgt = Target(0.0, None, np.zeros(4), pv.P0)
    with pytest.raises(ValueError, match="constantTurn"):
        trace_nodes(pv, PERIOD, [tgt], constantTurn=True, ais=lambda scan, mmsi: None)
    with pytest.raises(NotImplementedError, match="ct"):
        trace_nodes(ct, PERIOD, [])
    with pytest.raises(ValueError, match="constant-turn"):
        trace_nodes(pv, PERIOD, [], constantTurn=True)
    with pytest.raises(ValueError, match="Tracker"):
        tgt.getTrackInnovations(PERIOD, ais=True)
    # a chain of one node has nothing to explain, and needs no device to say so
    for tr, keys in ((trace_nodes(pv, PERIOD, [tgt])[0], 5), (tgt.getTrackInnovations(PERIOD), 5),
                     (trace_nodes(pv, PERIOD, [tgt], ais=lambda scan, mmsi: None)[0], 10)):
        assert len(tr) == keys and tr["v"].shape == (1, 2) and tr["S"].shape == (1, 2, 2) and not tr["observed"].any()
        assert np.isnan(tr["nis"]).all() and np.isnan(tr["ll"]).all()


def test_the_new_switches_default_to_off():
    from pymht_amd import smoothing
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    assert inspect.signature(smoothing.trace_nodes).parameters["ais"].default is None
    assert inspect.signature(smoothing.consistency).parameters["alpha"].default == 0.05
    for fn in (Tracker.getTrackInnovations, Target.getTrackInnovations, Tracker.getConsistency):
        p = inspect.signature(fn).parameters
        assert p["ais"].default is False and p["constantTurn"].default is False
    assert inspect.signature(Tracker.getConsistency).parameters["alpha"].default == 0.05
