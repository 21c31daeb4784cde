"""CPU: the trial manoeuvres (csrc/mht_trial.h: trial_track, trial_candidate, trial_cell and the fold, what a lane of the kernels of
mht_trial.hip runs) compiled for the host and held to the criterion of tests/test_trial_gpu.py against tests/trial_ref.py; the
properties of the manoeuvre; and the refusals that need no GPU.

Criterion, the project's: per output family e = max |got - truth| / (1 + |truth|) over the cells that are not NaN in the truth,
e <= 8 max(e_np, eps64), truth the reference's np.longdouble evaluation (pc: mpmath at 30 digits, the rule's 64 nodes) and e_np its
float64 evaluation's error; the NaN cells and the exact zeros of pc are the truth's exactly; tpc, an arg max, is held through
encounter_ref.hold_tpc (test_encounter_cpu.hold does all of this and is used as it is).  The measured figures are in the docstrings."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import encounter_ref as eref
import trial_ref as ref
from test_encounter_cpu import FACTOR, RADIUS, hold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.03125e10      # (a value no case here produces)
DT = 5.0


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    so = str(tmp_path_factory.mktemp("trial_host") / "libtrial_host.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "trial_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.trial_manoeuvres_host.restype = C.c_int
    lib.trial_manoeuvres_host.argtypes = [C.c_int32] * 4 + [C.c_double] * 2 + [C.c_void_p] * 6 + [C.c_double] + [C.c_void_p] * 4
    lib.trial_host_work_doubles.restype = C.c_int64
    lib.trial_host_work_doubles.argtypes = [C.c_int32] * 3
    lib.trial_fold_host.restype = None
    lib.trial_fold_host.argtypes = [C.c_int32] + [C.c_void_p] * 2
    return lib


def host_trial(lib, x, P, Phi, Q, K, dt, R, own, Sown, w, cand):
    """The twin on x [n, N], P [n, N, N]: (trial_ref's dict of [G, n] arrays, summary [4, G], pos [K + 1, 2, n + G], S [K + 1, 3, n + G]);
    every cell of the table, of the summary and of the trajectories is written."""
    n, N = x.shape
    cand = np.ascontiguousarray(cand, dtype=np.float64)
    G = len(cand)
    xp, Pp = eref.pack(x, P)
    Phi, Q = np.ascontiguousarray(Phi, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    own, Sown = np.ascontiguousarray(own, dtype=np.float64), np.ascontiguousarray(Sown, dtype=np.float64)
    out, summary = np.full((5, G, n), SENTINEL), np.full((4, G), SENTINEL)
    work = np.full(int(lib.trial_host_work_doubles(n, G, K)), SENTINEL)
    rc = lib.trial_manoeuvres_host(N, n, G, K, dt, R, Phi.ctypes.data, Q.ctypes.data, xp.ctypes.data, Pp.ctypes.data, own.ctypes.data, Sown.ctypes.data,
                                   w, cand.ctypes.data, out.ctypes.data, summary.ctypes.data, work.ctypes.data)
    assert rc == 0
    traj = work[:5 * (K + 1) * (n + G)]
    assert not (out == SENTINEL).any() and not (summary == SENTINEL).any() and not (traj == SENTINEL).any()
    return eref.seam_dict(out), summary, traj[:2 * (K + 1) * (n + G)].reshape(K + 1, 2, n + G), traj[2 * (K + 1) * (n + G):].reshape(K + 1, 3, n + G)


def check_summary(summary, table):
    """summary [4, G] is bit for bit the NumPy fold of the table it came with: nanmax / nanmin, the lowest index on ties, NaN and -1 for
    a row without a figure"""
    want = ref.fold(table["pc"], table["dcpa"])
    for f, name in enumerate(ref.SUMMARY):
        assert np.array_equal(summary[f], want[name].astype(np.float64), equal_nan=True), (name, summary[f], want[name])
    return want


_mp_case = {}


def mp_case(N):
    """The case pc and tpc are held to mpmath on, shared with tests/test_trial_gpu.py and computed once: trial_ref.make_scene of
    models/pv (N = 4, S_own = 0) or models/ca (N = 6, S_own set), 52 tracks, the five candidates, K = 3, dt = 5, R = 80 -- 250 cells
    of four steps.  Returns (x, P, own, Sown, Phi, Q, K, truth, f64, e_np of pc)."""
    if N not in _mp_case:
        from pymht_amd.models import ca, pv
        model = pv if N == 4 else ca
        K = 3
        x, P, own, Sown = ref.make_scene(model, 52, seed=3, own_cov=N == 6)
        Phi, Q = eref.model_matrices(model, DT)
        args = (x, P, Phi, Q, K, DT, RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES)
        truth, f64 = ref.manoeuvres(*args, truth=True), ref.manoeuvres(*args)
        e_np = eref.ratios([f64], [truth], [f64], ("pc",))["pc"][1]
        _mp_case[N] = (x, P, own, Sown, Phi, Q, K, truth, f64, e_np)
    return _mp_case[N]


_cases = {}


def cell_case(N, K, n):
    """trial_ref.make_scene of models/pv (S_own = 0) or models/ca (S_own set), n tracks, the five candidates, dt = 5, R = 80, evaluated
    once for both test files (the truth's pc is the float64 rule's on the longdouble d_k, Sigma_k): (x, P, own, Sown, Phi, Q, truth, f64)"""
    if (N, K, n) not in _cases:
        from pymht_amd.models import ca, pv
        model = pv if N == 4 else ca
        x, P, own, Sown = ref.make_scene(model, n, seed=3, own_cov=N == 6)
        Phi, Q = eref.model_matrices(model, DT)
        args = (x, P, Phi, Q, K, DT, RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES)
        _cases[N, K, n] = (x, P, own, Sown, Phi, Q, ref.manoeuvres(*args, truth=True, pc_mp=False), ref.manoeuvres(*args))
    return _cases[N, K, n]


def check_special_columns(got, summary, Sown, K):
    """What the special tracks of encounter_ref.make_batch look like in any evaluation of the table"""
    for e in (eref.NAN_X, eref.NAN_P):
        assert all(np.isnan(got[name][:, e]).all() for name in ref.NAMES), e
    a, b = eref.TWINS
    assert all(np.array_equal(got[name][:, a], got[name][:, b]) for name in ("tcpa", "dcpa"))      # (the same states; their P differ)
    for e in eref.ZERO_P:
        if not np.any(Sown):      # Sigma_0 = 0: pc, tpc and md2 are NaN, the CPA stays
            assert np.isnan(got["pc"][:, e]).all() and np.isnan(got["md2"][:, e]).all() and np.isnan(got["tpc"][:, e]).all()
        else:
            assert np.isfinite(got["pc"][:, e]).all()
        assert np.isfinite(got["dcpa"][:, e]).all() and np.isfinite(got["tcpa"][:, e]).all()
    assert not np.isin(summary[1], [eref.NAN_X, eref.NAN_P]).any() and not np.isin(summary[3], [eref.NAN_X, eref.NAN_P]).any()
    if K * DT >= 20.0:      # the own ship stands on into the twins at t = 20: of the two equal columns the lower has the row's smallest dcpa
        assert summary[3, 0] == a and summary[2, 0] < 1e-6, summary[:, 0]


@pytest.mark.parametrize("N", [4, 6])
def test_pc_and_tpc_on_the_host_against_mpmath(lib, N):
    """mp_case(N): every figure of the twin against the truth, pc's from mpmath.  Measured, host build (g++ -O2 -mfma), ratios
    e / max(e_np, eps64) for tcpa / dcpa / md2 / pc:
        N 4   1 / 1 / 1 / 1   (e_np 2.5e-14 / 2.5e-15 / 1.7e-15 / 7.6e-16), 166 of the 240 cells with pc > 0
        N 6   1 / 1 / 1 / 1   (e_np 5.1e-14 / 9.7e-16 / 8.7e-16 / 3.3e-16), 247 of 250
    -- the twin and the float64 reference do the same operations in the same order."""
    assert np.finfo(np.longdouble).eps < 1e-18
    x, P, own, Sown, Phi, Q, K, truth, f64, e_np = mp_case(N)
    got, summary, _, _ = host_trial(lib, x, P, Phi, Q, K, DT, RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES)
    hold("host build, trial mpmath case N %d" % N, got, truth, f64, DT)
    assert int(np.sum(truth["pc"] > 0)) >= 20 and int(np.sum((truth["pc"] > 1e-3) & (truth["pc"] < 0.999))) >= 4
    hold("float64 reference, trial mpmath case N %d" % N, f64, truth, f64, DT)
    check_summary(summary, got)


@pytest.mark.parametrize("N,K,n", [(4, 1, 70), (4, 7, 300), (6, 1, 300), (6, 7, 70)])
def test_manoeuvres_on_the_host_meet_the_accuracy_criterion(lib, N, K, n):
    """cell_case: 70 tracks (one partly filled tile a candidate) and 300 (two tiles: the fold across tiles runs), K 1 and 7, the five
    candidates -- stand on, 40 degrees to port, 40 to starboard after 5 s, half speed, a delay beyond the horizon.  tcpa, dcpa and md2
    against the longdouble truth, pc against the float64 reference with e_np from mp_case; the candidates' trajectories against the
    longdouble ones under the same criterion; the special tracks; the summary is the NumPy fold of the twin's own table bit for bit; a
    permutation of the candidates permutes the rows bit for bit; the candidate whose delay lies beyond the horizon has the stand-on
    candidate's row bit for bit.  Measured, host build, ratios for tcpa / dcpa / md2 / pc / the candidates' positions:
        N 4 K 1 n 70    0.47 / 1 / 1 / 0.13 / 0.69      N 4 K 7 n 300   1 / 1 / 1 / 1.01 / 0.85
        N 6 K 1 n 300   1 / 1 / 1 / 1.69 / 0.40         N 6 K 7 n 70    1 / 1 / 1 / 0.88 / 0.90"""
    x, P, own, Sown, Phi, Q, truth, f64 = cell_case(N, K, n)
    got, summary, pos, S = host_trial(lib, x, P, Phi, Q, K, DT, RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES)
    hold("host build, trial N %d K %d n %d" % (N, K, n), got, truth, f64, DT, pc_scale=mp_case(N)[9])
    check_special_columns(got, summary, Sown, K)
    check_summary(summary, got)
    G = len(ref.CANDIDATES)
    want, mine = ref.candidate_path(own, Sown, ref.TURN_RATE, ref.CANDIDATES, K, DT, np.longdouble), ref.candidate_path(own, Sown, ref.TURN_RATE, ref.CANDIDATES, K, DT)
    path = lambda p, s: dict(pos=np.asarray(p), S=np.asarray(s))
    res = eref.ratios([path(np.moveaxis(pos[:, :, n:], 1, 2), np.moveaxis(S[:, :, n:], 1, 2))], [path(*want)], [path(*mine)], ("pos", "S"))
    print("candidate paths N %d K %d: " % (N, K) + " | ".join("%s e %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert all(np.isfinite(e) and ratio <= FACTOR for e, _, ratio in res.values())
    assert all(np.array_equal(got[k][4], got[k][0], equal_nan=True) for k in ref.NAMES)
    order = np.array([3, 0, 4, 2, 1])
    back, bsum, _, _ = host_trial(lib, x, P, Phi, Q, K, DT, RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES[order])
    assert all(np.array_equal(back[k], got[k][order], equal_nan=True) for k in ref.NAMES) and np.array_equal(bsum, summary[:, order], equal_nan=True)
    assert G == 5 and got["pc"].shape == (G, n)


@pytest.mark.parametrize("N", [4, 6])
def test_stand_on_candidate_is_the_linear_own_ship(lib, N):
    """(a) dpsi = 0, f = 1, at any delay: the own ship as a linear entry 0 of encounter_ref.encounters (first = 1), under the criterion
    with that reference's longdouble truth and float64 error.  With Q = 0 and no covariance on the own ship's velocity, so that the
    linear entry's position covariance stays S_own as the manoeuvre's does (a Q would grow it).  The twin evaluates k dt v0 in closed
    form where the linear entry accumulates.  Measured: ratios 1 / 1 / 1 / 0.44 (N 4) and 1 / 1 / 1 / 0.31 (N 6), the three delays
    alike."""
    from pymht_amd.models import ca, pv
    model = pv if N == 4 else ca
    K = 6
    x, P, own, Sown = ref.make_scene(model, 70, seed=5)
    Phi, Q = eref.model_matrices(model, DT)[0], np.zeros((N, N))
    xo, Po = np.zeros(N), np.zeros((N, N))
    xo[:4] = own
    Po[0, 0], Po[0, 1], Po[1, 0], Po[1, 1] = Sown[0], Sown[1], Sown[1], Sown[2]
    xs, Ps = np.vstack([xo, x]), np.concatenate([Po[None], P])
    cut = lambda d: {k: v[..., 1:] for k, v in d.items()}
    truth, f64 = cut(eref.encounters(xs, Ps, Phi, Q, K, DT, RADIUS, first=1, truth=True, pc_mp=False)), cut(eref.encounters(xs, Ps, Phi, Q, K, DT, RADIUS, first=1))
    cand = np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 12.5], [0.0, 1.0, 1000.0]])
    got, _, _, _ = host_trial(lib, x, P, Phi, Q, K, DT, RADIUS, own, Sown, ref.TURN_RATE, cand)
    for g in range(len(cand)):
        hold("stand-on candidate %d against the linear own ship, N %d" % (g, N), {k: got[k][g:g + 1] for k in ref.NAMES}, truth, f64, DT, pc_scale=mp_case(N)[9])


def test_mirrored_scene_gives_the_same_figures(lib):
    """(b) y -> -y for the own ship and every track (the covariances' cross terms change sign) and dpsi -> -dpsi: the figures of the
    mirrored scene are held to the truth of the scene itself, under the criterion."""
    from pymht_amd.models import ca
    N, K, n = 6, 7, 70
    x, P, own, Sown, Phi, Q, truth, f64 = cell_case(N, K, n)
    flip = np.array([1.0, -1.0] * (N // 2))
    xm, Pm = x * flip, P * np.outer(flip, flip)
    ownm, Sm = own * np.array([1.0, -1.0, 1.0, -1.0]), Sown * np.array([1.0, -1.0, 1.0])
    cm = ref.CANDIDATES * np.array([-1.0, 1.0, 1.0])
    got, summary, _, _ = host_trial(lib, xm, Pm, Phi, Q, K, DT, RADIUS, ownm, Sm, ref.TURN_RATE, cm)
    hold("mirrored scene", got, truth, f64, DT, pc_scale=mp_case(N)[9])
    check_summary(summary, got)
    assert ca.P0.shape == (N, N)


def test_path_is_continuous_at_the_joints():
    """(c) p(t) at t0 from the stand-on branch and from the arc, and at te from the arc and from the straight run, in np.longdouble:
    equal to a few longdouble roundings of the path's scale; and the speed on the straight run is f |v0| on the course turned by dpsi."""
    L = np.longdouble
    own = np.array([120.0, -340.0, 6.0, 3.0])
    eps = float(np.finfo(L).eps)
    for cand in ([0.7, 1.0, 12.5], [-0.7, 0.5, 3.0], [np.pi, 1.3, 0.0], [-2.5, 0.0, 40.0], [0.0, 0.8, 7.0], [1e-9, 1.0, 5.0]):
        t0, te, (stand_on, arc, straight) = ref.path_branches(own, ref.TURN_RATE, cand)
        scale = 1 + float(np.abs(stand_on(t0)).max()) + float(te) * 10.0
        assert np.abs(stand_on(t0) - arc(t0)).max() <= 16 * eps * scale, cand
        assert np.abs(arc(te) - straight(te)).max() <= 16 * eps * scale, cand
        v = (straight(te + 10) - straight(te)) / L(10)
        want = L(cand[1]) * np.array([np.cos(L(cand[0])) * L(6) - np.sin(L(cand[0])) * L(3), np.sin(L(cand[0])) * L(6) + np.cos(L(cand[0])) * L(3)])
        assert np.abs(v - want).max() <= 1e-15, cand
    # and the float64 restatement is that path, at times on every branch
    K, dt = 12, 2.5
    cand = np.array([[0.7, 1.0, 12.5], [-0.7, 0.5, 3.0], [np.pi, 1.3, 0.0], [0.0, 0.8, 7.0]])
    pos, _ = ref.candidate_path(own, np.zeros(3), ref.TURN_RATE, cand, K, dt)
    for g, c in enumerate(cand):
        t0, te, br = ref.path_branches(own, ref.TURN_RATE, c)
        for k in range(K + 1):
            t = L(k) * L(dt)
            want = br[0 if t <= t0 else 1 if t <= te else 2](t)
            assert np.abs(pos[k, g] - want).max() <= 1e-12 * (1 + float(np.abs(want).max())), (c, k)


def test_head_on_scene_prefers_the_alteration(lib):
    """(d) The own ship at 10 m/s east, a target 1000 m ahead at 10 m/s west, 60 s in 12 steps, radius 50, w = 0.05 rad/s.  Of the grid
    (stand on; 20, 40 and 60 degrees to either side; half speed) the stand-on candidate has the largest pc, and the 60 degree
    alterations have a larger dcpa and a smaller pc than it; to either side the wider turn has the larger dcpa and no larger a pc.
    Inequalities only."""
    from pymht_amd.models import pv
    x = np.array([[1000.0, 0.0, -10.0, 0.0], [400.0, 3000.0, 0.0, 2.0]])
    P = np.tile(np.asarray(pv.P0, dtype=np.float64), (2, 1, 1))
    Phi, Q = eref.model_matrices(pv, 5.0)
    deg = np.pi / 180.0
    cand = np.array([[0.0, 1.0, 0.0]] + [[s * a * deg, 1.0, 0.0] for a in (20.0, 40.0, 60.0) for s in (1.0, -1.0)] + [[0.0, 0.5, 0.0]])
    got, summary, _, _ = host_trial(lib, x, P, Phi, Q, 12, 5.0, 50.0, [0.0, 0.0, 10.0, 0.0], np.zeros(3), 0.05, cand)
    pc, dcpa = got["pc"][:, 0], got["dcpa"][:, 0]
    print("head-on: pc", pc, "dcpa", dcpa)
    assert (pc[0] > pc[1:]).all() and int(np.argmax(summary[0])) == 0
    assert (dcpa[5:7] > dcpa[0]).all() and (pc[5:7] < pc[0]).all()
    for side in ([0, 1, 3, 5], [0, 2, 4, 6]):
        assert (np.diff(dcpa[side]) > 0).all() and (np.diff(pc[side]) <= 0).all()
    assert (summary[1] == 0).all() and (summary[3] == 0).all()
    from pymht_amd import evaluation
    assert evaluation.trial_best(summary[0], summary[2]) in (5, 6)


def test_fold_is_total_and_skips_nan(lib):
    """The fold over figures with ties, NaN and infinities, forwards and backwards: the same bits, and NumPy's nanmax / nanmin with the
    lowest index; nothing but NaN gives NaN and -1."""
    rng = np.random.default_rng(2)
    for m, kind in ((1, "nan"), (7, "nan"), (300, "mixed"), (300, "ties"), (5, "inf")):
        fig = rng.integers(0, 4, (m, 2)).astype(np.float64) if kind == "ties" else rng.normal(size=(m, 2))
        if kind == "nan":
            fig[:] = np.nan
        if kind in ("mixed", "ties"):
            fig[rng.random((m, 2)) < 0.3] = np.nan
        if kind == "inf":
            fig[1], fig[3] = np.inf, -np.inf
        res = np.full((2, 4), SENTINEL)
        lib.trial_fold_host(m, np.ascontiguousarray(fig).ctypes.data, res.ctypes.data)
        want = ref.fold(fig[None, :, 0], fig[None, :, 1])
        assert np.array_equal(res[0], res[1], equal_nan=True), kind
        assert np.array_equal(res[0], [want["pcMax"][0], want["pcArg"][0], want["dcpaMin"][0], want["dcpaArg"][0]], equal_nan=True), (kind, res[0], want)


def test_refusals_that_need_no_gpu_and_what_the_docstrings_say(lib):
    """(e) What the seam refuses, on the twin: nothing is written.  evaluation.trial_manoeuvres: ValueError for every argument that does
    not fit, before a device is needed; no track gives [G, 0] arrays.  evaluation.trial_best's order.  Tracker.getTrialManoeuvres'
    signature -- turnRate without a default -- and docstring; the model goes through evaluation.encounter_model, which refuses a
    constant-turn tracker."""
    from pymht_amd import evaluation
    from pymht_amd.models import ct, pv
    from pymht_amd.tracker import Tracker
    a = np.zeros(512)
    p = a.ctypes.data
    nan, inf = float("nan"), float("inf")
    ok = dict(nx=4, n=2, G=2, K=3, dt=1.0, R=1.0, w=0.1)
    for bad in (dict(nx=5), dict(K=0), dict(K=65), dict(G=0), dict(G=4097), dict(n=-1), dict(dt=0.0), dict(dt=nan), dict(dt=inf), dict(R=0.0), dict(R=-1.0),
                dict(R=inf), dict(w=0.0), dict(w=-0.1), dict(w=nan), dict(w=inf)):
        kw = dict(ok)
        kw.update(bad)
        assert lib.trial_manoeuvres_host(kw["nx"], kw["n"], kw["G"], kw["K"], kw["dt"], kw["R"], p, p, p, p, p, p, kw["w"], p, p, p, p) == -1, bad
    for c in ([4.0, 1.0, 0.0], [-3.2, 1.0, 0.0], [0.1, -0.5, 0.0], [0.1, 1.0, -1.0], [inf, 1.0, 0.0], [0.1, inf, 0.0], [0.1, 1.0, inf]):
        cand = np.array([[0.0, 1.0, 0.0], c])
        assert lib.trial_manoeuvres_host(4, 2, 2, 3, 1.0, 1.0, p, p, p, p, p, p, 0.1, cand.ctypes.data, p, p, p) == -1, c
    assert (a == 0).all()
    x, P = np.zeros((3, 4)), np.tile(np.eye(4), (3, 1, 1))
    Phi, Q = eref.model_matrices(pv, 2.5)
    good = dict(x=x, P=P, Phi=Phi, Q=Q, steps=4, dt=2.5, radius=50.0, own=[0.0, 0.0, 1.0, 0.0], candidates=[[0.0, 1.0, 0.0], [0.5, 1.0, 0.0]], turnRate=0.05)
    for bad in (dict(x=np.zeros((3, 5))), dict(x=np.zeros(4)), dict(P=np.zeros((3, 4, 3))), dict(P=np.zeros((2, 4, 4))), dict(Phi=np.eye(6)), dict(Q=np.eye(3)),
                dict(steps=0), dict(steps=65), dict(steps=2.5), dict(steps=True), dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(radius=0.0), dict(radius=inf),
                dict(Phi=np.full((4, 4), nan)), dict(turnRate=0.0), dict(turnRate=-1.0), dict(turnRate=nan), dict(turnRate=inf), dict(turnRate=None),
                dict(own=[0.0, 0.0]), dict(own=[0.0, 0.0, 1.0, inf]), dict(own=np.zeros(6)), dict(ownCovariance=np.eye(3)), dict(ownCovariance=[[1.0, 0.5], [0.2, 1.0]]),
                dict(ownCovariance=[[inf, 0.0], [0.0, 1.0]]), dict(candidates=[]), dict(candidates=[0.0, 1.0, 0.0]), dict(candidates=[[0.0, 1.0]]),
                dict(candidates=np.zeros((4097, 3))), dict(candidates=[[3.2, 1.0, 0.0]]), dict(candidates=[[0.1, -1.0, 0.0]]), dict(candidates=[[0.1, 1.0, -2.0]]),
                dict(candidates=[[0.1, inf, 0.0]])):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError, match="trial_manoeuvres"):
            evaluation.trial_manoeuvres(**kw)
    # no track: empty arrays, no device
    out = evaluation.trial_manoeuvres(**dict(good, x=x[:0], P=P[:0]))
    assert sorted(out) == sorted(ref.NAMES + ref.SUMMARY + ("candidates",))
    assert all(out[k].shape == (2, 0) for k in ref.NAMES) and all(out[k].shape == (2,) for k in ref.SUMMARY)
    assert np.isnan(out["pcMax"]).all() and np.isnan(out["dcpaMin"]).all() and out["pcArg"].dtype == np.int64 and (out["pcArg"] == -1).all() and (out["dcpaArg"] == -1).all()
    assert np.array_equal(out["candidates"], good["candidates"])
    assert evaluation.TRIAL_MAX_CANDIDATES == 4096 and "#define MHT_TRIAL_MAX_CANDIDATES 4096" in open(os.path.join(ROOT, "include", "mht_amd.h")).read()
    # best: the smallest pcMax, then the largest dcpaMin, then the lowest index; a NaN pcMax is not eligible
    assert evaluation.trial_best([0.3, 0.1, 0.1, nan, 0.1], [5.0, 7.0, 9.0, 99.0, 9.0]) == 2
    assert evaluation.trial_best([nan, 0.2, 0.2], [1.0, nan, 1.0]) == 2 and evaluation.trial_best([nan, nan], [1.0, 2.0]) is None
    # the Tracker's entry point: its signature, and the constant-turn refusal
    sig = inspect.signature(Tracker.getTrialManoeuvres).parameters
    assert list(sig) == ["self", "horizon", "radius", "ownShip", "courseChanges", "turnRate", "speedFactors", "delay", "ownCovariance", "steps"]
    assert sig["turnRate"].default is inspect.Parameter.empty and sig["speedFactors"].default == (1.0,) and sig["delay"].default == 0.0
    assert sig["ownCovariance"].default is None and sig["steps"].default is None
    assert "encounter_model" in inspect.getsource(Tracker.getTrialManoeuvres)
    doc = " ".join(Tracker.getTrialManoeuvres.__doc__.split())
    assert "AIS-aided filter's state is NOT used" in doc and "NotImplementedError" in doc and "counter-clockwise" in doc
    with pytest.raises(NotImplementedError, match="ct"):
        evaluation.encounter_model(ct, 2.5)
    sig = inspect.signature(evaluation.trial_manoeuvres).parameters
    assert list(sig) == ["x", "P", "Phi", "Q", "steps", "dt", "radius", "own", "candidates", "turnRate", "ownCovariance", "device", "ctx"]
