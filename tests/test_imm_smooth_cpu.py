"""CPU: the IMM smoother's walk (csrc/mht_imm_smooth.h: imm_smooth_walk, what the lanes of the kernels of mht_imm_smooth.hip run)
compiled for the host with the modes in lock step (tests/hostmath/imm_smooth_host.cpp) and held to the criterion of
tests/test_imm_smooth_gpu.py on that test's own batches, one track at a time; its bit properties against the host twins of the smoother
and of the IMM filter; the reference (tests/imm_smooth_ref.py) against smooth_ref and imm_ref and on a simulated manoeuvre; and the
refusals that need no GPU.

Criterion, the smoothers': per output family (mus, muf, xs, Ps, ll) e = max |got - truth| / (1 + |truth|) over the cells of the batch
that are not NaN in the truth, e <= 8 max(e_np, eps64), truth the np.longdouble evaluation of the reference and e_np its float64
evaluation's error; the NaN cells are the truth's exactly and nObs is exact."""
import ctypes as C
import importlib
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import filter_ref as fr
import imm_ref as ir
import imm_smooth_ref as ref
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
    """(the host build of the IMM smoother's walk, of the IMM filter's walk, of the smoothers' walk)"""
    gxx = shutil.which("g++") or "g++"
    out = []
    for name in ("imm_smooth_host", "imm_host", "smooth_host"):
        so = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                               os.path.join(ROOT, "tests", "hostmath", name + ".cpp"), "-o", so])
        out.append(C.CDLL(so))
    ims, imm, smo = out
    ims.imm_smooth_lin_host.restype = None
    ims.imm_smooth_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 2 + [C.c_int32] * 2 + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 9
    ims.imm_smooth_ct_host.restype = None
    ims.imm_smooth_ct_host.argtypes = [C.c_double, C.c_void_p] + [C.c_int32] * 2 + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 9
    imm.imm_lin_host.restype = None
    imm.imm_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 2 + [C.c_int32] * 2 + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 8
    imm.imm_ct_host.restype = None
    imm.imm_ct_host.argtypes = [C.c_double, C.c_void_p] + [C.c_int32] * 2 + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 8
    smo.smooth_lin_host.restype = None
    smo.smooth_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
    smo.smooth_ct_host.restype = None
    smo.smooth_ct_host.argtypes = [C.c_double] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
    return ims, imm, smo


def _model(name):
    return importlib.import_module("pymht_amd.models." + name)


def _f64(*arrays):
    return [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in arrays]


def _padded(z, rows):
    has = sr.detected(z)
    has[0] = False
    zz, hz = np.zeros((rows, 2)), np.zeros(rows, dtype=np.uint8)
    zz[:len(z)] = np.where(has[:, None], np.asarray(z, dtype=np.float64), 0.0)
    hz[:len(z)] = has
    return zz, hz


p = lambda a: a.ctypes.data


def host_smooth(libs, kind, model, track, modes, filtered=False):
    """One track through the host twin of the smoother (filtered: of the IMM filter, its dict in the smoother's names): the dict of
    imm_smooth_ref.imm_smooth.  No sentinel is left and the rows behind the track's end are NaN."""
    Qs, Rs, Pi, mu0 = _f64(*modes)
    L, rows, r = len(track[2]), len(track[2]) + TAIL, len(Qs)
    zz, hz = _padded(track[2], rows)
    trans, Cm = ir.transition_and_C(kind, model, PERIOD)
    Cm, x0, P0 = _f64(Cm, track[0], track[1])
    n = len(x0)
    ns = n * (n + 1) // 2
    mus, muf, x, P, out = (np.full((rows, r), SENTINEL), np.full((rows, r), SENTINEL), np.full((rows, n), SENTINEL), np.full((rows, ns), SENTINEL),
                           np.full(2, SENTINEL))
    outs = (p(mus), p(x), p(P)) + (() if filtered else (p(muf),)) + (p(out),)
    if kind == "ct":
        fn = libs[1].imm_ct_host if filtered else libs[0].imm_smooth_ct_host
        fn(trans, p(Cm), L, rows, p(x0), p(P0), p(zz), p(hz), r, p(Qs), p(Rs), p(Pi), p(mu0), *outs)
    else:
        A, = _f64(trans)
        fn = libs[1].imm_lin_host if filtered else libs[0].imm_smooth_lin_host
        fn(n, p(A), p(Cm), L, rows, p(x0), p(P0), p(zz), p(hz), r, p(Qs), p(Rs), p(Pi), p(mu0), *outs)
    if filtered:
        muf = mus
    for a in (mus, muf, x, P, out):
        assert not (a == SENTINEL).any()
        assert a is out or np.isnan(a[L:]).all()
    return dict(mus=mus[:L].copy(), muf=muf[:L].copy(), xs=x[:L].copy(), Ps=fr.full(P[:L], n), ll=np.asarray(out[0]), nobs=int(out[1]))


def host_rts(libs, kind, model, track, Q):
    """One track through the host twin of the plain smoother under the model's matrices with Q in place of its own: (xs [L, n], Ps [L, n, n])"""
    L = len(track[2])
    zz, hz = _padded(track[2], L)
    x0, P0, Q = _f64(track[0], track[1], Q)
    n = len(x0)
    xs, Ps = np.empty((L, n)), np.empty((L, n * (n + 1) // 2))
    if kind == "ct":
        T, _, Cm, R = cr.model_matrices(model, PERIOD)
        Cm, R = _f64(Cm, R)
        libs[2].smooth_ct_host(T, p(Q), p(Cm), p(R), L, p(x0), p(P0), p(zz), p(hz), p(xs), p(Ps), 1)
    else:
        A, _, Cm, R = _f64(*sr.model_matrices(model, PERIOD))
        libs[2].smooth_lin_host(n, p(A), p(Q), p(Cm), p(R), L, p(x0), p(P0), p(zz), p(hz), p(xs), p(Ps), 1)
    return xs, fr.full(Ps, n)


def hold(label, got, truth, f64):
    """The criterion over a batch; prints the measured ratios"""
    res = ref.ratios(got, truth, f64, ref.NAMES)
    print(label + ": " + " | ".join("%s e %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert ref.same_nan(got, truth, ref.NAMES), "the NaN cells are not the truth's"
    assert [g["nobs"] for g in got] == [t["nobs"] for t in truth]
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, (k, e, e_np, ratio)


CASES = [("linear", "pv", 1), ("linear", "pv", 2), ("linear", "pv", 3), ("linear", "pv", 4), ("linear", "pv", "blocked"), ("linear", "ca", 4),
         ("ct", "ct", 2)]


@pytest.mark.parametrize("kind,name,key", CASES)
def test_walk_on_the_host_meets_the_accuracy_criterion_and_ends_on_the_filter(libs, kind, name, key):
    """filter_ref.edge_batch, 35 tracks of 1, 2, 60, 7, 33 nodes in turn, every fourth never detected, under imm_ref.SETUPS[key].  The
    twin meets the criterion against tests/imm_smooth_ref.py (the ratios are printed); its muf, ll, nObs are the IMM filter twin's
    bits, and at the last node so are mus, xs, Ps; the rows of mus add up to 1."""
    model = _model(name)
    assert np.finfo(np.longdouble).eps < 1e-18
    tracks, truth, f64 = ref.reference(kind, model, PERIOD, N_TRACKS, 11, key)
    modes = ir.setup(model, PERIOD, key)
    got = [host_smooth(libs, kind, model, t, modes) for t in tracks]
    hold("host build of the IMM smoother's walk, %s models/%s, modes %s" % (kind, name, key), got, truth, f64)
    for g, t in zip(got, tracks):
        f = host_smooth(libs, kind, model, t, modes, filtered=True)
        assert np.array_equal(g["muf"], f["muf"]) and np.array_equal(g["ll"], f["ll"]) and g["nobs"] == f["nobs"]
        assert all(np.array_equal(g[k][-1], f[k][-1]) for k in ("mus", "xs", "Ps"))
        assert np.abs(g["mus"].sum(axis=1) - 1.0).max() < 1e-12
    if key == "blocked":      # nobody enters mode 1, at any node >= 1, in hindsight either
        assert all((g["mus"][1:, 1] == 0.0).all() for g in got)


@pytest.mark.parametrize("kind,name", [("linear", "pv"), ("linear", "ca"), ("ct", "ct")])
def test_one_mode_is_the_smoother_bit_for_bit(libs, kind, name):
    """Pi = [[1]]: every weight is exactly 1 and every difference exactly 0.  The reference's states are smooth_ref.rts' (rts_ct's)
    bits; the twin's are the smoother twin's, and mus is exactly 1."""
    model = _model(name)
    tracks = fr.edge_batch(kind, model, PERIOD, N_TRACKS, 11)
    modes = ir.setup(model, PERIOD, 1)
    for t in tracks:
        one = ref.run(kind, model, PERIOD, t, 1)
        want = cr.rts_ct(*cr.model_matrices(model, PERIOD), *t) if kind == "ct" else sr.rts(*sr.model_matrices(model, PERIOD), *t)
        assert np.array_equal(one["xs"], want["xs"]) and np.array_equal(one["Ps"], want["Ps"]) and (one["mus"] == 1.0).all()
        got = host_smooth(libs, kind, model, t, modes)
        xs, Ps = host_rts(libs, kind, model, t, modes[0][0])
        assert np.array_equal(got["xs"], xs) and np.array_equal(got["Ps"], Ps) and (got["mus"] == 1.0).all() and (got["muf"] == 1.0).all()


def test_identity_chain_from_a_certain_mode_is_the_smoother_under_that_mode(libs):
    """r = 2, Pi = I, mu0 = (0, 1), Q = (Q, 16 Q) on imm_ref.manoeuvre_batch, where both modes stay finite: xs, Ps are the plain
    smoother's bits under 16 Q and mus = (0, 1) at every node, in the reference and in the twin -- mode 0 has probability 0 and never
    produces a 0 * inf."""
    from pymht_amd.models import pv
    Qs, Rs = ir.modes(pv, PERIOD, (1.0, 16.0))
    modes = (Qs, Rs, np.eye(2), np.array([0.0, 1.0]))
    A, _, Cm, R = sr.model_matrices(pv, PERIOD)
    for t in ir.manoeuvre_batch(pv, PERIOD, 12, 60, seed=5):
        one = ref.imm_smooth(A, Cm, *modes, *t)
        want = sr.rts(A, Qs[1], Cm, R, *t)
        assert np.array_equal(one["xs"], want["xs"]) and np.array_equal(one["Ps"], want["Ps"])
        got = host_smooth(libs, "linear", pv, t, modes)
        xs, Ps = host_rts(libs, "linear", pv, t, Qs[1])
        assert np.array_equal(got["xs"], xs) and np.array_equal(got["Ps"], Ps)
        for d in (one, got):
            assert (d["mus"][:, 0] == 0.0).all() and (d["mus"][:, 1] == 1.0).all()


def test_reference_forward_pass_is_the_filter_reference():
    """imm_smooth_ref.forward restates imm_ref.imm: muf, ll, nObs and the last node are its bits."""
    from pymht_amd.models import pv
    for key in (2, 3, "blocked"):
        for t in fr.edge_batch("linear", pv, PERIOD, 10, 11):
            a, b = ref.run("linear", pv, PERIOD, t, key), ir.run("linear", pv, PERIOD, t, key)
            assert np.array_equal(a["muf"], b["mu"]) and np.array_equal(a["ll"], b["ll"]) and a["nobs"] == b["nobs"]
            assert np.array_equal(a["mus"][-1], b["mu"][-1]) and np.array_equal(a["xs"][-1], b["x"][-1]) and np.array_equal(a["Ps"][-1], b["P"][-1])


@pytest.fixture(scope="module")
def manoeuvre():
    from pymht_amd.models import pv
    tracks, truth = ref.manoeuvre_batch_with_truth(pv, PERIOD)
    return tracks, truth, [ref.run("linear", pv, PERIOD, t, 2) for t in tracks]


def test_reference_finds_the_manoeuvre_in_hindsight(manoeuvre):
    """imm_ref.manoeuvre_batch(pv, 2.5) -- 40 tracks of 60 nodes, 64 Q on nodes 20 .. 39 -- under SETUPS[2]: the mean smoothed
    probability of the loud mode is >= 0.9 at nodes 25, 30, 35 and <= 0.1 at 5, 10, 15, 45, 50, 55, and at each of them on the right
    side of the filter's mean."""
    from pymht_amd.models import pv
    tracks, truth, res = manoeuvre
    same = ir.manoeuvre_batch(pv, PERIOD)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2], equal_nan=True) for a, b in zip(tracks, same))
    mus = np.mean([r["mus"][:, 1] for r in res], axis=0)
    muf = np.mean([r["muf"][:, 1] for r in res], axis=0)
    print("loud mode, smoothed / filtered: " + "  ".join("%d: %.3f / %.3f" % (k, mus[k], muf[k]) for k in (5, 10, 15, 25, 30, 35, 45, 50, 55)))
    for k in (25, 30, 35):
        assert mus[k] >= 0.9 and mus[k] >= muf[k], (k, mus[k], muf[k])
    for k in (5, 10, 15, 45, 50, 55):
        assert mus[k] <= 0.1 and mus[k] <= muf[k], (k, mus[k], muf[k])


def test_reference_beats_the_single_level_smoothers(manoeuvre):
    """Position RMSE over nodes 1 .. L - 1 against the true states on the same batch: the IMM smoother's is <= 0.85 x the RTS
    smoother's at 1 x Q and <= the RTS smoother's at 16 x Q."""
    from pymht_amd.models import pv
    tracks, truth, res = manoeuvre
    A, Q, Cm, R = sr.model_matrices(pv, PERIOD)
    Q32 = ir.modes(pv, PERIOD, (1.0,))[0][0]
    rmse = lambda xs: float(np.sqrt(np.mean([((x[1:, :2] - s[1:, :2]) ** 2).sum(axis=1) for x, s in zip(xs, truth)])))
    e_imm = rmse([r["xs"] for r in res])
    e_1 = rmse([sr.rts(A, Q32, Cm, R, *t)["xs"] for t in tracks])
    e_16 = rmse([sr.rts(A, 16.0 * Q32, Cm, R, *t)["xs"] for t in tracks])
    print("position RMSE: IMM smoother %.3f, RTS at 1 x Q %.3f, at 16 x Q %.3f" % (e_imm, e_1, e_16))
    assert e_imm <= 0.85 * e_1 and e_imm <= e_16


@pytest.mark.parametrize("name", ["pv", "ca"])
def test_reference_covariances_are_positive_definite_and_probabilities_add_up(name):
    """Setups 2, 3, 4 and blocked on the manoeuvre batch: every smoothed covariance is positive definite, every row of mus adds up to 1
    within 1e-12."""
    model = _model(name)
    tracks = ir.manoeuvre_batch(model, PERIOD, 8, 60, seed=5)
    for key in (2, 3, 4, "blocked"):
        for t in tracks:
            got = ref.run("linear", model, PERIOD, t, key)
            assert np.abs(got["mus"].sum(axis=1) - 1.0).max() <= 1e-12
            assert np.linalg.eigvalsh(got["Ps"]).min() > 0.0, (name, key)


def test_refusals_that_need_no_gpu_and_the_signatures():
    from pymht_amd import smoothing
    from pymht_amd.models import ct, pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    Q, R, Pi, mu0 = smoothing.imm_modes(pv, PERIOD, (1.0, 16.0))
    track = [(np.zeros(4), pv.P0, [None, np.zeros(2)])]
    for args in ((Q[:, :3, :3], R, Pi), (Q, R[:1], Pi), (Q, R, np.eye(3)), (Q, R, [[0.5, 0.6], [0.5, 0.5]])):
        with pytest.raises(ValueError):
            smoothing.imm_smooth_tracks(pv, PERIOD, track, *args)
    with pytest.raises(ValueError, match="mu0"):
        smoothing.imm_smooth_tracks(pv, PERIOD, track, Q, R, Pi, mu0=[0.5, 0.6])
    with pytest.raises(NotImplementedError, match="ct"):
        smoothing.imm_smooth_tracks(ct, PERIOD, [(np.zeros(6), ct.P0, [None, np.zeros(2)])], Q, R, Pi)
    with pytest.raises(ValueError, match="constant-turn"):
        smoothing.imm_smooth_tracks_ct(pv, PERIOD, track, Q, R, Pi)
    assert smoothing.imm_smooth_tracks(pv, PERIOD, [], Q, R, Pi) == []
    for fn, sib in ((smoothing.imm_smooth_tracks, smoothing.imm_tracks), (smoothing.imm_smooth_tracks_ct, smoothing.imm_tracks_ct),
                    (smoothing.imm_smooth_nodes, smoothing.imm_nodes), (Tracker.getSmoothModeProbabilities, Tracker.getModeProbabilities),
                    (Target.getSmoothModeProbabilities, Target.getModeProbabilities)):
        assert inspect.signature(fn) == inspect.signature(sib), fn
    assert inspect.signature(Tracker.getSmoothTracks).parameters["imm"].default is None
    # a chain of one node was never filtered, let alone smoothed: mu0 and its initial state, and no device is needed to say so
    tgt = Target(0.0, None, np.arange(4.0), pv.P0)
    one, = smoothing.imm_smooth_nodes(pv, PERIOD, [tgt], Q, R, Pi, mu0=[0.25, 0.75])
    assert sorted(one) == ["P", "logLikelihood", "mu", "muFiltered", "nObs", "x"]
    assert np.array_equal(one["mu"], [[0.25, 0.75]]) and np.array_equal(one["muFiltered"], [[0.25, 0.75]])
    assert np.array_equal(one["x"], [np.arange(4.0)]) and np.array_equal(one["P"], [pv.P0]) and one["logLikelihood"] == 0.0 and one["nObs"] == 0
    d = tgt.getSmoothModeProbabilities(PERIOD)
    assert np.array_equal(d["mu"], [[0.5, 0.5]]) and d["nObs"] == 0
    with pytest.raises(ValueError, match="constant-turn"):
        tgt.getSmoothModeProbabilities(PERIOD, constantTurn=True)
