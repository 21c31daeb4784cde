"""CPU: the interacting-multiple-model walk (csrc/mht_imm.h: imm_walk, what the lanes of the kernels of mht_imm.hip run) compiled for
the host with the modes in lock step (tests/hostmath/imm_host.cpp) and held to the criterion of tests/test_imm_gpu.py on that test's own
batches, one track at a time; with one mode against the host twins of the filter and the score, bit for bit; the reference
(tests/imm_ref.py) against filter_ref, against the score of independent modes and on a simulated manoeuvre; and the refusals that need
no GPU.

Criterion, the smoothers': per output family (mu, x, P, ll) e = max |got - truth| / (1 + |truth|) over the cells of the batch that are
not NaN in the truth, e <= 8 max(e_np, eps64), truth the np.longdouble evaluation of the reference and e_np its float64 evaluation's
error; the NaN cells are the truth's exactly and nObs is exact.  The measured ratios are in the docstrings of the tests."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import filter_ref as fr
import imm_ref as ref
import smooth_ct_ref as cr
import smooth_ref as sr
import smooth_score_ref as scr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 2.5
FACTOR = 8.0
TAIL = 3            # rows the host arrays have behind a track's end: the walk writes them too
SENTINEL = -7.0
N_TRACKS = 35       # the lengths 1, 2, 60, 7, 33 seven times over


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(the host build of the IMM walk, of the filter walk, of the score walk)"""
    gxx = shutil.which("g++") or "g++"
    out = []
    for name in ("imm_host", "filter_host", "smooth_score_host"):
        so = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                               os.path.join(ROOT, "tests", "hostmath", name + ".cpp"), "-o", so])
        out.append(C.CDLL(so))
    imm, filt, score = out
    imm.imm_lin_host.restype = None
    imm.imm_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 2 + [C.c_int32] * 2 + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 8
    imm.imm_ct_host.restype = None
    imm.imm_ct_host.argtypes = [C.c_double, C.c_void_p] + [C.c_int32] * 2 + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 8
    filt.filter_lin_host.restype = None
    filt.filter_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] * 2 + [C.c_void_p] * 6
    score.smooth_score_lin_host.restype = None
    score.smooth_score_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 6
    return imm, filt, score


def _f64(*arrays):
    return [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in arrays]


def _padded(z, rows):
    has = sr.detected(z)
    has[0] = False
    zz, hz = np.zeros((rows, 2)), np.zeros(rows, dtype=np.uint8)
    zz[:len(z)] = np.where(has[:, None], np.asarray(z, dtype=np.float64), 0.0)
    hz[:len(z)] = has
    return zz, hz


def host_imm(libs, kind, model, track, modes):
    """One track through the host twin: the dict of imm_ref.imm.  No sentinel is left and the rows behind the track's end are NaN."""
    Qs, Rs, Pi, mu0 = _f64(*modes)
    L, rows, r = len(track[2]), len(track[2]) + TAIL, len(Qs)
    zz, hz = _padded(track[2], rows)
    trans, Cm = ref.transition_and_C(kind, model, PERIOD)
    Cm, x0, P0 = _f64(Cm, track[0], track[1])
    n = len(x0)
    ns = n * (n + 1) // 2
    mu, x, P, out = np.full((rows, r), SENTINEL), np.full((rows, n), SENTINEL), np.full((rows, ns), SENTINEL), np.full(2, SENTINEL)
    p = lambda a: a.ctypes.data
    if kind == "ct":
        libs[0].imm_ct_host(trans, p(Cm), L, rows, p(x0), p(P0), p(zz), p(hz), r, p(Qs), p(Rs), p(Pi), p(mu0), p(mu), p(x), p(P), p(out))
    else:
        A, = _f64(trans)
        libs[0].imm_lin_host(n, p(A), p(Cm), L, rows, p(x0), p(P0), p(zz), p(hz), r, p(Qs), p(Rs), p(Pi), p(mu0), p(mu), p(x), p(P), p(out))
    for a in (mu, x, P, out):
        assert not (a == SENTINEL).any()
    assert np.isnan(mu[L:]).all() and np.isnan(x[L:]).all() and np.isnan(P[L:]).all()
    return dict(mu=mu[:L].copy(), x=x[:L].copy(), P=fr.full(P[:L], n), ll=np.asarray(out[0]), nobs=int(out[1]))


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
def test_imm_walk_on_the_host_meets_the_accuracy_criterion(libs, kind, name, key):
    """filter_ref.edge_batch, 35 tracks of 1, 2, 60, 7, 33 nodes in turn, every fourth never detected, under imm_ref.SETUPS[key] (three
    modes: zeros in Pi; "blocked": a mode that is never entered and keeps its own state).  Measured, host build (g++ -O2 -mfma), ratios
    e / max(e_np, eps64) for mu / x / P / ll:
        pv r=1 0 / 0.98 / 0.81 / 1.00       pv r=2 0.91 / 0.59 / 0.49 / 0.68    pv r=3 0.85 / 0.72 / 0.81 / 1.35
        pv r=4 1.00 / 1.50 / 1.25 / 1.00    pv blocked 0 / 0.98 / 0.81 / 1.00   ca r=4 1.80 / 1.74 / 0.71 / 0.65
        ct r=2 0.65 / 0.75 / 0.53 / 1.13
    (e_np 1.4e-13 .. 4.4e-13 for mu, 2.6e-13 .. 1.2e-12 for x, 1.2e-14 .. 4.0e-12 for P -- 8.6e-10 under the constant-turn model --
    and 1.7e-14 .. 4.7e-14 for ll; with one mode, and with the blocked one, mu is exact.)
    Node 0 is (mu0, x_init, P_init); the rows of mu add up to 1."""
    import importlib
    model = importlib.import_module("pymht_amd.models." + name)
    assert np.finfo(np.longdouble).eps < 1e-18
    tracks, truth, f64 = ref.reference(kind, model, PERIOD, N_TRACKS, 11, key)
    modes = ref.setup(model, PERIOD, key)
    got = [host_imm(libs, kind, model, t, modes) for t in tracks]
    hold("host build of the IMM walk, %s models/%s, modes %s" % (kind, name, key), got, truth, f64)
    for g, t in zip(got, tracks):
        assert np.array_equal(g["mu"][0], modes[3]) and np.array_equal(g["x"][0], t[0]) and np.array_equal(g["P"][0], t[1])
        assert np.abs(g["mu"].sum(axis=1) - 1.0).max() < 1e-12
        assert len(t[2]) > 1 or (float(g["ll"]) == 0.0 and g["nobs"] == 0)
    if key == "blocked":      # the mode nobody enters has probability exactly 0 from node 1 on
        assert all((g["mu"][1:, 1] == 0.0).all() for g in got)


@pytest.mark.parametrize("name", ["pv", "ca"])
def test_one_mode_is_the_filter_and_the_score_bit_for_bit(libs, name):
    """Pi = [[1]]: every weight is exactly 1 and every difference exactly 0.  The reference's x, P are filter_ref.filter_lin's bits; the
    twin's are the filter twin's, and its ll, nObs the score twin's -- the same expressions in the same order."""
    import importlib
    model = importlib.import_module("pymht_amd.models." + name)
    tracks = fr.edge_batch("linear", model, PERIOD, N_TRACKS, 11)
    modes = ref.setup(model, PERIOD, 1)
    A, Q, Cm, R = _f64(*sr.model_matrices(model, PERIOD))
    assert np.array_equal(modes[0][0], Q) and np.array_equal(modes[1][0], R)      # (scale 1 is the model itself)
    n = A.shape[0]
    ns = n * (n + 1) // 2
    p = lambda a: a.ctypes.data
    for t in tracks:
        one, lin = ref.run("linear", model, PERIOD, t, 1), fr.run("linear", model, PERIOD, t)
        assert np.array_equal(one["x"], lin["xf"]) and np.array_equal(one["P"], lin["Pf"]) and (one["mu"] == 1.0).all()
        got = host_imm(libs, "linear", model, t, modes)
        L, rows = len(t[2]), len(t[2]) + TAIL
        zz, hz = _padded(t[2], rows)
        x0, P0 = _f64(t[0], t[1])
        xf, Pf, out = np.empty((rows, n)), np.empty((rows, ns)), np.empty(5)
        libs[1].filter_lin_host(n, p(A), p(Q), p(Cm), p(R), L, rows, p(x0), p(P0), p(zz), p(hz), p(xf), p(Pf))
        libs[2].smooth_score_lin_host(n, p(A), p(Q), p(Cm), p(R), L, p(x0), p(P0), p(zz), p(hz), None, p(out))
        assert np.array_equal(got["x"], xf[:L]) and np.array_equal(got["P"], fr.full(Pf[:L], n)) and (got["mu"] == 1.0).all()
        assert float(got["ll"]) == out[0] and got["nobs"] == int(out[2])


def test_reference_with_an_identity_chain_is_the_score_of_independent_modes():
    """Pi = I: the modes do not interact, ll = logsumexp_j(ln mu0_j + ll_j) and the last mu is the softmax of the same terms, ll_j
    smooth_score_ref.score under mode j.  Measured in float64 with scales (0.25, 1, 16) and mu0 = (0.5, 0.3, 0.2): 3.5e-16 relative in
    ll, 2.4e-14 absolute in mu; 1e-10 is allowed -- this guards the algebra, where a wrong formula is off by 1e-2, not the rounding."""
    from pymht_amd.models import pv
    Qs, Rs = ref.modes(pv, PERIOD, (0.25, 1.0, 16.0))
    mu0 = np.array([0.5, 0.3, 0.2])
    A, _, Cm, _ = sr.model_matrices(pv, PERIOD)
    worst_ll = worst_mu = 0.0
    for t in fr.edge_batch("linear", pv, PERIOD, N_TRACKS, 11):
        got = ref.imm(A, Cm, Qs, Rs, np.eye(3), mu0, *t)
        terms = np.log(mu0) + np.array([scr.score(A, Qs[j], Cm, Rs[j], *t)["ll"] for j in range(3)])
        top = terms.max()
        want = top + np.log(np.exp(terms - top).sum())
        worst_ll = max(worst_ll, abs(float(got["ll"]) - want) / (1.0 + abs(want)))
        worst_mu = max(worst_mu, np.abs(got["mu"][-1] - np.exp(terms - want)).max())
    print("identity chain: ll %.3g relative, mu %.3g absolute" % (worst_ll, worst_mu))
    assert worst_ll < 1e-10 and worst_mu < 1e-10


def test_reference_finds_the_manoeuvre():
    """40 simulated pv tracks of 60 nodes (seed 5), process noise 64 Q on nodes 20 .. 39 and Q elsewhere; modes (Q, 64 Q), stay 0.95.
    Per track the mean probability of the loud mode over nodes 25 .. 39 is at least 0.79 (asked: > 0.5) and over the quiet stretches
    5 .. 19 and 45 .. 59 at most 0.09 (asked: < 0.2)."""
    from pymht_amd.models import pv
    from pymht_amd.smoothing import imm_modes
    Q, R, Pi, mu0 = imm_modes(pv, PERIOD, (1.0, 64.0), stay=0.95)
    assert np.array_equal(Q, ref.modes(pv, PERIOD, (1.0, 64.0))[0]) and np.array_equal(Pi, ref.sticky(2))
    loud, quiet = [], []
    for t in ref.manoeuvre_batch(pv, PERIOD, 40, 60, seed=5):
        mu = ref.imm(pv.Phi(PERIOD), pv.C_RADAR, Q, R, Pi, mu0, *t)["mu"][:, 1]
        loud.append(mu[25:40].mean())
        quiet.append(max(mu[5:20].mean(), mu[45:60].mean()))
    print("loud stretch: min %.3f; quiet stretches: max %.3f" % (min(loud), max(quiet)))
    assert min(loud) > 0.5 and max(quiet) < 0.2


def test_reference_poison_and_shapes():
    """A mode whose R is no covariance (indefinite: det S < 0 at every plot, the poison of tests/test_smooth_score_grid_gpu.py) makes ll
    NaN on a track with a plot and leaves a never-detected one at exactly 0.0.  (R = -R is no such poison for this model: S = C P C' - R
    is isotropic, both its eigenvalues change sign together and det S stays positive.)"""
    from pymht_amd.models import pv
    Qs, Rs = ref.modes(pv, PERIOD, (1.0, 16.0))
    Rs[1] = np.diag([-1e9, 1.0])
    tracks = fr.edge_batch("linear", pv, PERIOD, 8, 11)
    for i, t in enumerate(tracks):
        got = ref.imm(pv.Phi(PERIOD), pv.C_RADAR, Qs, Rs, ref.sticky(2), [0.5, 0.5], *t)
        L = len(t[2])
        assert got["mu"].shape == (L, 2) and got["x"].shape == (L, 4) and got["P"].shape == (L, 4, 4)
        if got["nobs"] == 0:
            assert float(got["ll"]) == 0.0
        else:
            assert np.isnan(float(got["ll"]))
    assert sum(ref.imm(pv.Phi(PERIOD), pv.C_RADAR, Qs, Rs, ref.sticky(2), [0.5, 0.5], *t)["nobs"] > 0 for t in tracks) >= 3


def test_refusals_that_need_no_gpu():
    from pymht_amd.models import ca, ct, pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.smoothing import imm_modes, imm_nodes, imm_tracks, imm_tracks_ct
    for bad in ((), (1.0, -1.0), (1.0, np.nan), (1.0, 2.0, 3.0, 4.0, 5.0)):
        with pytest.raises(ValueError):
            imm_modes(pv, PERIOD, bad)
    with pytest.raises(ValueError, match="rScales|modes"):
        imm_modes(pv, PERIOD, (1.0, 2.0), rScales=(1.0,))
    for bad in (0.0, 1.5, -0.1, True, "0.9"):
        with pytest.raises(ValueError, match="stay"):
            imm_modes(pv, PERIOD, (1.0, 16.0), stay=bad)
    Q, R, Pi, mu0 = imm_modes(ca, PERIOD, (1.0, 4.0, 16.0), rScales=(1.0, 2.0, 1.0), stay=0.9)
    assert Q.shape == (3, 6, 6) and R.shape == (3, 2, 2) and np.allclose(Pi.sum(axis=1), 1.0) and np.array_equal(np.diag(Pi), [0.9] * 3)
    assert np.array_equal(Pi[0, 1:], [(1.0 - 0.9) / 2] * 2) and np.array_equal(mu0, np.full(3, 1.0 / 3)) and np.array_equal(R[1], 2.0 * R[0])
    assert np.array_equal(imm_modes(pv, PERIOD, (1.0,))[2], [[1.0]]) and np.array_equal(imm_modes(pv, PERIOD, (1.0,), stay=1.0)[3], [1.0])
    Q, R, Pi, mu0 = imm_modes(pv, PERIOD, (1.0, 16.0))
    track = [(np.zeros(4), pv.P0, [None, np.zeros(2)])]
    skew = Q.copy()
    skew[1, 0, 1] += 1.0
    for args in ((skew, R, Pi), (Q[:, :3, :3], R, Pi), (Q, R[:1], Pi), (np.tile(Q, (3, 1, 1))[:5], np.tile(R, (3, 1, 1))[:5], np.eye(5)),
                 (Q, R, np.eye(3)), (Q, R, [[0.5, 0.6], [0.5, 0.5]]), (Q, R, [[1.5, -0.5], [0.5, 0.5]]), (Q, R, [[np.nan, 1.0], [0.5, 0.5]])):
        with pytest.raises(ValueError):
            imm_tracks(pv, PERIOD, track, *args)
    for bad in ([0.5, 0.6], [1.0], [1.5, -0.5]):
        with pytest.raises(ValueError, match="mu0"):
            imm_tracks(pv, PERIOD, track, Q, R, Pi, mu0=bad)
    with pytest.raises(NotImplementedError, match="ct"):
        imm_tracks(ct, PERIOD, [(np.zeros(6), ct.P0, [None, np.zeros(2)])], Q, R, Pi)
    with pytest.raises(ValueError, match="constant-turn"):
        imm_tracks_ct(pv, PERIOD, track, Q, R, Pi)
    per, ll, nobs = imm_tracks(pv, PERIOD, [], Q, R, Pi)
    assert per == [] and ll.shape == (0,) and nobs.shape == (0,) and nobs.dtype == np.int32
    # a chain of one node was never filtered: mu0 and its initial state, and no device is needed to say so
    tgt = Target(0.0, None, np.arange(4.0), pv.P0)
    (one,), ll, nobs = imm_nodes(pv, PERIOD, [tgt], Q, R, Pi, mu0=[0.25, 0.75])
    assert np.array_equal(one[0], [[0.25, 0.75]]) and np.array_equal(one[1], [np.arange(4.0)]) and np.array_equal(one[2], [pv.P0])
    assert ll.tolist() == [0.0] and nobs.tolist() == [0]
    d = tgt.getModeProbabilities(PERIOD)
    assert sorted(d) == ["P", "logLikelihood", "mu", "nObs", "x"] and np.array_equal(d["mu"], [[0.5, 0.5]]) and d["logLikelihood"] == 0.0 and d["nObs"] == 0
    with pytest.raises(NotImplementedError, match="ct"):
        imm_nodes(ct, PERIOD, [], Q, R, Pi)
    with pytest.raises(ValueError, match="constant-turn"):
        tgt.getModeProbabilities(PERIOD, constantTurn=True)


def test_the_defaults_are_said_not_to_be_tuned_and_the_product_does_not_import_the_oracle():
    from pymht_amd import smoothing
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    for fn in (Tracker.getModeProbabilities, Target.getModeProbabilities):
        p = inspect.signature(fn).parameters
        assert p["qScales"].default == (1.0, 16.0) and p["stay"].default == 0.95 and p["constantTurn"].default is False
        assert "not tuned" in " ".join(fn.__doc__.split()).lower()
    assert inspect.signature(Tracker.getModeProbabilities).parameters["terminated"].default is False
    assert smoothing.IMM_MAX_MODES == 4
    pkg = os.path.join(ROOT, "pymht_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(base, f)).read()
                assert not re.search(r"^\s*(import|from)\s+(oracle|mht_oracle|m_of_n_oracle|refimport)\b", text, re.M), f
