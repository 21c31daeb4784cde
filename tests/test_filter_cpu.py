"""CPU: the filter walk (csrc/mht_smooth_filter.h: smooth_filter_walk, what a lane of the kernels of mht_smooth_filter.hip runs) compiled
for the host and held to the criterion of tests/test_filter_gpu.py on that test's own batches, one track at a time; its last node
against the host twin of the smoother walk, bit for bit; the reference (tests/filter_ref.py) against itself; and the refusals that need
no GPU.

Criterion, the smoothers': per output family (xf, Pf) e = max |got - truth| / (1 + |truth|) over the cells of the batch that are not
NaN in the truth, e <= 8 max(e_np, eps64), truth the np.longdouble evaluation of the reference and e_np its float64 evaluation's error;
the NaN cells are the truth's exactly.  The measured ratios are in the docstrings of the tests."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import filter_ref as ref
import smooth_ct_ref as cr
import smooth_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 2.5
FACTOR = 8.0
TAIL = 3            # rows the host arrays have behind a track's end: the walk writes them too
SENTINEL = -7.0
N_TRACKS = 35       # the lengths 1, 2, 60, 7, 33 seven times over


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(the host build of the filter walk, the host build of the smoother walk)"""
    gxx = shutil.which("g++") or "g++"
    out = []
    for name in ("filter_host", "smooth_host"):
        so = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                               os.path.join(ROOT, "tests", "hostmath", name + ".cpp"), "-o", so])
        out.append(C.CDLL(so))
    filt, smooth = out
    filt.filter_lin_host.restype = None
    filt.filter_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] * 2 + [C.c_void_p] * 6
    filt.filter_ct_host.restype = None
    filt.filter_ct_host.argtypes = [C.c_double] + [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p] * 6
    filt.filter_ais_host.restype = None
    filt.filter_ais_host.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 2 + [C.c_void_p] * 11
    smooth.smooth_lin_host.restype = None
    smooth.smooth_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
    smooth.smooth_ct_host.restype = None
    smooth.smooth_ct_host.argtypes = [C.c_double] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
    smooth.smooth_ais_host.restype = None
    smooth.smooth_ais_host.argtypes = [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 11 + [C.c_int32]
    return filt, smooth


def _f64(*arrays):
    return [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in arrays]


def _padded(z, rows):
    has = sr.detected(z)
    has[0] = False
    zz, hz = np.zeros((rows, 2)), np.zeros(rows, dtype=np.uint8)
    zz[:len(z)] = np.where(has[:, None], np.asarray(z, dtype=np.float64), 0.0)
    hz[:len(z)] = has
    return zz, hz


def _finish(L, n, xf, Pf, xs, Ps):
    """The host arrays as the Python layer's (xf [L, n], Pf [L, n, n]); no sentinel is left, the rows behind the track's end are NaN,
    and the last node is the smoother twin's last smoothed node, bit for bit."""
    assert not (xf == SENTINEL).any() and not (Pf == SENTINEL).any()
    assert np.isnan(xf[L:]).all() and np.isnan(Pf[L:]).all() and np.isfinite(xf[:L]).all() and np.isfinite(Pf[:L]).all()
    assert np.array_equal(xf[L - 1], xs[L - 1]) and np.array_equal(Pf[L - 1], Ps[L - 1])
    return dict(xf=xf[:L].copy(), Pf=ref.full(Pf[:L], n))


def host_filter(libs, kind, model, track):
    L, rows = len(track[2]), len(track[2]) + TAIL
    zz, hz = _padded(track[2], rows)
    if kind == "ct":
        T, Q, Cm, R = cr.model_matrices(model, PERIOD)
        Q, Cm, R, x0, P0 = _f64(Q, Cm, R, track[0], track[1])
    else:
        A, Q, Cm, R, x0, P0 = _f64(*sr.model_matrices(model, PERIOD), track[0], track[1])
    n = len(x0)
    ns = n * (n + 1) // 2
    xf, Pf = np.full((rows, n), SENTINEL), np.full((rows, ns), SENTINEL)
    xs, Ps = np.full((L, n), SENTINEL), np.full((L, ns), SENTINEL)
    p = lambda a: a.ctypes.data
    if kind == "linear":
        libs[0].filter_lin_host(n, p(A), p(Q), p(Cm), p(R), L, rows, p(x0), p(P0), p(zz), p(hz), p(xf), p(Pf))
        libs[1].smooth_lin_host(n, p(A), p(Q), p(Cm), p(R), L, p(x0), p(P0), p(zz), p(hz), p(xs), p(Ps), 1)
    elif kind == "ct":
        libs[0].filter_ct_host(T, p(Q), p(Cm), p(R), L, rows, p(x0), p(P0), p(zz), p(hz), p(xf), p(Pf))
        libs[1].smooth_ct_host(T, p(Q), p(Cm), p(R), L, p(x0), p(P0), p(zz), p(hz), p(xs), p(Ps), 1)
    else:
        from pymht_amd.smoothing import _ais_inputs
        ((has_m, msg, r, leg),), legs = _ais_inputs(model, [(x0, P0, track[2], track[3])])
        kind_a, mm, rr, ll = hz.copy(), np.zeros((rows, 4)), np.ones(rows), np.zeros(rows, dtype=np.int32)
        kind_a[:L] += 2 * has_m.astype(np.uint8)
        mm[:L], rr[:L], ll[:L] = msg, r, leg
        legs = np.ascontiguousarray(legs if len(legs) else np.zeros((1, 52)))
        libs[0].filter_ais_host(p(A), p(Q), p(Cm), p(R), L, rows, p(x0), p(P0), p(zz), p(hz), p(kind_a), p(mm), p(rr), p(ll), p(legs), p(xf), p(Pf))
        libs[1].smooth_ais_host(p(A), p(Q), p(Cm), p(R), L, p(x0), p(P0), p(zz), p(hz), p(kind_a), p(mm), p(rr), p(ll), p(legs), p(xs), p(Ps), 1)
    return _finish(L, n, xf, Pf, xs, Ps)


def _hold(label, got, truth, f64):
    res = ref.ratios(got, truth, f64, ref.NAMES)
    print(label + ": " + " | ".join("%s e %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert ref.same_nan(got, truth, ref.NAMES), "the NaN cells are not the truth's"
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, (k, e, e_np, ratio)


@pytest.mark.parametrize("kind,name", [("linear", "pv"), ("linear", "ca"), ("ct", "ct"), ("ais", "pv"), ("ais-none", "pv")])
def test_filter_walk_on_the_host_meets_the_accuracy_criterion_and_ends_in_the_smoother(libs, kind, name):
    """filter_ref.edge_batch, 35 tracks of 1, 2, 60, 7, 33 nodes in turn, every fourth never detected.  Measured, host build
    (g++ -O2 -mfma), ratios e / max(e_np, eps64) for xf / Pf:
        pv 0.98 / 0.81 (e_np 2.6e-13 / 1.2e-14)   ca 1.00 / 0.55 (7.4e-13 / 3.3e-14)   ct 1.00 / 0.54 (4.3e-13 / 2.4e-10)
        AIS 1.06 / 0.48 (3.6e-13 / 4.2e-13)        AIS without messages 1.00 / 0.25 (2.7e-13 / 5.6e-14)
    Every track's last node is the host smoother twin's last smoothed node, bit for bit; node 0 is (x_init, P_init)."""
    import importlib
    model = importlib.import_module("pymht_amd.models." + name)
    assert np.finfo(np.longdouble).eps < 1e-18
    tracks, truth, f64 = ref.reference(kind, model, PERIOD, N_TRACKS, seed=11)
    got = [host_filter(libs, kind, model, t) for t in tracks]
    _hold("host build of the filter walk, %s models/%s" % (kind, name), got, truth, f64)
    for g, t in zip(got, tracks):
        assert np.array_equal(g["xf"][0], t[0]) and np.array_equal(g["Pf"][0], t[1])
        assert np.array_equal(g["Pf"], g["Pf"].transpose(0, 2, 1))
    if kind == "ais":
        assert sum(sum(a is not None for a in t[3]) for t in tracks) > 100
    if kind == "ais-none":      # without its messages a track is the linear filter, bit for bit
        lin = [host_filter(libs, "linear", model, t[:3]) for t in tracks]
        assert all(np.array_equal(g[k], q[k]) for g, q in zip(got, lin) for k in ref.NAMES)


def test_reference_is_self_consistent():
    """tests/filter_ref.py alone: float64 against longdouble below 1e-9 per family; node 0 is the initial state; the last filtered node
    is the smoother reference's last smoothed node; a plot shrinks the predicted covariance."""
    from pymht_amd.models import ca, ct, pv
    for kind, model in (("linear", pv), ("linear", ca), ("ct", ct), ("ais", pv)):
        tracks, truth, f64 = ref.reference(kind, model, PERIOD, N_TRACKS, seed=11)
        assert truth[0]["xf"].dtype == np.longdouble and ref.same_nan(f64, truth, ref.NAMES)
        res = ref.ratios(f64, truth, f64, ref.NAMES)
        print(kind, model.__name__, {k: v[0] for k, v in res.items()})
        assert all(np.isfinite(e) and 0 < e < 1e-9 for e, _, _ in res.values())
        assert all(np.array_equal(f["xf"][0], t[0]) and np.array_equal(f["Pf"][0], t[1]) for f, t in zip(f64, tracks))
    import smooth_ais_ref as ar
    for dtype in (np.float64, np.longdouble):      # the forward halves of the smoother references, bit for bit
        pairs = [(ref.run("linear", ca, PERIOD, t, dtype), sr.rts(*sr.model_matrices(ca, PERIOD), *t, dtype=dtype)) for t in ref.edge_batch("linear", ca, PERIOD, 5, 3)]
        pairs += [(ref.run("ct", ct, PERIOD, t, dtype), cr.rts_ct(*cr.model_matrices(ct, PERIOD), *t, dtype=dtype)) for t in ref.edge_batch("ct", ct, PERIOD, 5, 3)]
        pairs += [(ref.run("ais", pv, PERIOD, t, dtype), ar.rts_ais(pv, PERIOD, *t, dtype=dtype)) for t in ref.edge_batch("ais", pv, PERIOD, 5, 3)]
        assert all(f[k].dtype == dtype and np.array_equal(f[k], s[k]) for f, s in pairs for k in ref.NAMES)
    mats = sr.model_matrices(pv, PERIOD)
    (x0, P0, z), = sr.make_batch(pv, PERIOD, [20], seed=4, p_detect=1.0)
    f, s = ref.filter_lin(*mats, x0, P0, z), sr.rts(*mats, x0, P0, z)
    assert np.array_equal(f["xf"][-1], s["xs"][-1]) and np.array_equal(f["Pf"][-1], s["Ps"][-1])
    assert sorted(f) == ["Pf", "xf"] and f["xf"].shape == (20, 4) and f["Pf"].shape == (20, 4, 4)
    A, Q = [np.asarray(m, dtype=np.float64) for m in mats[:2]]
    assert all(np.trace(f["Pf"][k]) < np.trace(A @ f["Pf"][k - 1] @ A.T + Q) for k in range(1, 20))
    assert np.array_equal(ref.full(np.arange(10.0), 4)[1], [1, 4, 5, 6])


def test_refusals_that_need_no_gpu():
    from pymht_amd.models import ca, ct, pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.smoothing import filter_nodes, filter_tracks, filter_tracks_ais, filter_tracks_ct
    track = [(np.zeros(4), pv.P0, [None, np.zeros(2)])]
    ct_track = [(np.zeros(6), ct.P0, [None, np.zeros(2)])]
    with pytest.raises(NotImplementedError, match="ct"):
        filter_tracks(ct, PERIOD, ct_track)
    with pytest.raises(ValueError, match="constant-turn"):
        filter_tracks_ct(pv, PERIOD, track)
    for model, nx in ((ca, 6), (ct, 6)):
        with pytest.raises(ValueError, match="4-state linear"):
            filter_tracks_ais(model, PERIOD, [(np.zeros(nx), model.P0, [None, np.zeros(2)], [None, (1.0, 1.5, np.zeros(4), True)])])
    with pytest.raises(ValueError, match="positive"):
        filter_tracks_ais(pv, PERIOD, [(np.zeros(4), pv.P0, [None, np.zeros(2)], [None, (0.0, 2.5, np.zeros(4), True)])])
    assert filter_tracks(pv, PERIOD, []) == [] and filter_tracks_ct(ct, PERIOD, []) == [] and filter_tracks_ais(pv, PERIOD, []) == []
    tgt = Target(0.0, None, np.arange(4.0), pv.P0)
    with pytest.raises(ValueError, match="constantTurn"):
        filter_nodes(pv, PERIOD, [tgt], constantTurn=True, ais=lambda scan, mmsi: None)
    with pytest.raises(NotImplementedError, match="ct"):
        filter_nodes(ct, PERIOD, [])
    with pytest.raises(ValueError, match="constant-turn"):
        filter_nodes(pv, PERIOD, [], constantTurn=True)
    with pytest.raises(ValueError, match="Tracker"):
        tgt.getFilteredTrack(PERIOD, ais=True)
    # a chain of one node was never filtered: its initial state, and no device is needed to say so
    for xf, Pf in (filter_nodes(pv, PERIOD, [tgt])[0], tgt.getFilteredTrack(PERIOD)):
        assert xf.shape == (1, 4) and Pf.shape == (1, 4, 4) and np.array_equal(xf[0], np.arange(4.0)) and np.array_equal(Pf[0], pv.P0)


def test_the_new_switches_default_to_off_and_the_docstrings_say_what_the_covariances_are():
    from pymht_amd import smoothing
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    assert inspect.signature(smoothing.filter_nodes).parameters["ais"].default is None
    assert inspect.signature(Tracker.getFilteredTracks).parameters["terminated"].default is False
    for fn in (Tracker.getFilteredTracks, Target.getFilteredTrack):
        p = inspect.signature(fn).parameters
        assert p["ais"].default is False and p["constantTurn"].default is False
    for fn in (smoothing.filter_tracks, smoothing.filter_nodes, Tracker.getFilteredTracks, Target.getFilteredTrack):
        doc = " ".join(fn.__doc__.split())
        assert "float64 filter" in doc and "bit for bit" in doc and "forest" in doc, fn
