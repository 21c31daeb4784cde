"""GPU: the device trial manoeuvres (`mht_trial_manoeuvres`, include/mht_amd.h; pymht_amd.evaluation.trial_manoeuvres) and the drop-in
path on top (Tracker.getTrialManoeuvres), against tests/trial_ref.py.

The criterion is the project's (tests/test_trial_cpu.py states it and holds the host twin of the same header to it), per output family:
with the np.longdouble evaluation of the reference as the truth -- pc: mpmath at 30 digits with the rule's own 64 nodes --
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
and e_dev <= 8 * max(e_np, eps64); the NaN cells and the zeros of pc by the rule are the truth's exactly; tpc, an arg max, is held by
encounter_ref.hold_tpc.  On the tables too large for mpmath pc is held to the float64 reference with e_np from the mpmath case.  The
summary is held bit for bit to the NumPy fold of the device's own table.  Every test prints the device's own ratios -- measured on an
MI355X, tcpa / dcpa / md2 / pc:
    cells N 4   K 1, n 70: 0.47 / 1 / 1 / 0.13     K 7, n 300: 1 / 1 / 1 / 1.01   (e_np 1.3e-13 / 2.3e-14 / 1.2e-15; pc's 7.6e-16 from the mpmath case)
    cells N 6   K 1, n 300: 1 / 1 / 1 / 1.69       K 7, n 70: 1 / 1 / 1 / 0.75    (e_np 1.0e-14 / 3.0e-14 / 4.0e-16; pc's 3.3e-16)
    against mpmath           N 4: 1 / 1 / 1 / 1      N 6: 1 / 1 / 1 / 1
    getTrialManoeuvres       1 / 1 / 1 / 0.051
both builds alike -- and tools/trial_cost.py writes them into profiles/trial_cost.txt.  Nothing here is larger than 300 tracks, 5
candidates and 7 steps.  The shapes at which the kernels go round their grid-stride loops are
held in tests/test_encounter_strides_gpu.py."""
import numpy as np
import pytest

import encounter_ref as eref
import trial_ref as ref
from test_encounter_cpu import RADIUS, hold
from test_encounter_gpu import guard_untouched, guarded_work
from test_trial_cpu import DT, cell_case, check_special_columns, check_summary, mp_case

pytestmark = pytest.mark.gpu

SENTINEL = -7.03125e10


@pytest.fixture(scope="module")
def ctxs():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (pymht_amd has no CPU fallback)")
    from pymht_amd.device import Context
    c = {4: Context(0, nx=4), 6: Context(0, nx=6)}
    yield c
    for v in c.values():
        v.close()


def _raw(ctx, x, P, Phi, Q, K, dt, R, own, Sown, w, cand, nulls=(), nx=None, n=None, G=None, short=0, guard=0):
    """One call of the seam on x [n, N], P [n, N, N], the outputs preset to SENTINEL: (return code, out [5, G, n], summary [4, G]).
    guard > 0: that many bytes of a pattern lie behind the sizer's figure and must be the pattern after the call."""
    import torch
    dev = ctx.device
    N = x.shape[1]
    cand = np.ascontiguousarray(cand, dtype=np.float64)
    n = len(x) if n is None else n
    G = len(cand) if G is None else G
    xp, Pp = eref.pack(x, P)
    host = dict(Phi=np.ascontiguousarray(Phi, dtype=np.float64), Q=np.ascontiguousarray(Q, dtype=np.float64), own=np.ascontiguousarray(own, dtype=np.float64),
                Sown=np.ascontiguousarray(Sown, dtype=np.float64), cand=cand)
    arrays = dict(x=torch.from_numpy(xp).to(dev), P=torch.from_numpy(Pp).to(dev))
    arrays["out"] = torch.full((5, len(cand), len(x)), SENTINEL, dtype=torch.float64, device=dev)
    arrays["summary"] = torch.full((4, len(cand)), SENTINEL, dtype=torch.float64, device=dev)
    need = int(ctx.lib.mht_trial_work_bytes(len(x), len(cand), min(max(K, 1), 64)))
    arrays["work"] = guarded_work(need, guard, dev)
    ptr = lambda k: None if k in nulls else host[k].ctypes.data if k in host else arrays[k].data_ptr()
    torch.cuda.synchronize(dev)
    rc = ctx.lib.mht_trial_manoeuvres(ctx.handle, N if nx is None else nx, n, G, K, dt, R, ptr("Phi"), ptr("Q"), ptr("x"), ptr("P"), ptr("own"), ptr("Sown"), w,
                                      ptr("cand"), ptr("out"), ptr("summary"), ptr("work"), need - short)
    torch.cuda.synchronize(dev)
    assert guard_untouched(arrays["work"], need), "the call wrote behind the work buffer the sizer asks for"
    return rc, arrays["out"].cpu().numpy(), arrays["summary"].cpu().numpy()


@pytest.mark.parametrize("N,K,n,lib_nx", [(4, 1, 70, 4), (4, 7, 300, 4), (4, 1, 70, 6), (4, 7, 300, 6), (6, 1, 300, 6), (6, 7, 70, 6), (6, 1, 300, 4), (6, 7, 70, 4)])
def test_cell_cases_meet_the_accuracy_criterion_and_every_cell_is_written(ctxs, N, K, n, lib_nx):
    """The cases of tests/test_trial_cpu.py: 70 tracks -- a row straddles a wavefront, the tile of 256 lanes is partly filled -- and
    300, two tiles a candidate, so that the fold across tiles runs; K 1 and 7; G = 5: stand on, 40 degrees to port, 40 to starboard
    after 5 s, half speed, a delay beyond the horizon; the tracks hold a NaN in x, a NaN in P, P = 0 and identical states.  Table and
    summary preset to a sentinel, none left; the cells under the criterion; the summary bit for bit the NumPy fold of the device's own
    table; a permutation of the candidates permutes rows and summary bit for bit."""
    assert np.finfo(np.longdouble).eps < 1e-18
    x, P, own, Sown, Phi, Q, truth, f64 = cell_case(N, K, n)
    rc, out, summary = _raw(ctxs[lib_nx], x, P, Phi, Q, K, DT, RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES)
    assert rc == 0 and not (out == SENTINEL).any() and not (summary == SENTINEL).any()
    got = eref.seam_dict(out)
    hold("trial cells N %d K %d n %d, %d-state build" % (N, K, n, lib_nx), got, truth, f64, DT, pc_scale=mp_case(N)[9])
    check_special_columns(got, summary, Sown, K)
    check_summary(summary, got)
    assert np.array_equal(out[:, 4], out[:, 0], equal_nan=True)      # (a delay beyond the horizon: stand on)
    order = np.array([3, 0, 4, 2, 1])
    rc, back, bsum = _raw(ctxs[lib_nx], x, P, Phi, Q, K, DT, RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES[order])
    assert rc == 0 and np.array_equal(back, out[:, order], equal_nan=True) and np.array_equal(bsum, summary[:, order], equal_nan=True)


@pytest.mark.parametrize("N,lib_nx", [(4, 4), (4, 6), (6, 6), (6, 4)])
def test_pc_and_tpc_against_mpmath(ctxs, N, lib_nx):
    """mp_case(N) of tests/test_trial_cpu.py -- 52 tracks, the five candidates, K = 3; mpmath's truth computed once for both files --
    every figure under the criterion, e_np the float64 reference's own error there; a NaN candidate and a dead row."""
    x, P, own, Sown, Phi, Q, K, truth, f64, e_np = mp_case(N)
    rc, out, summary = _raw(ctxs[lib_nx], x, P, Phi, Q, K, DT, RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES)
    assert rc == 0 and not (out == SENTINEL).any() and not (summary == SENTINEL).any()
    hold("trial against mpmath N %d, %d-state build" % (N, lib_nx), eref.seam_dict(out), truth, f64, DT)
    check_summary(summary, eref.seam_dict(out))
    # a NaN in a candidate: its row is NaN and its summary NaN, -1; the other rows are what they were
    cand = ref.CANDIDATES.copy()
    cand[1, 2], cand[3, 0] = np.nan, np.nan
    rc, part, psum = _raw(ctxs[lib_nx], x, P, Phi, Q, K, DT, RADIUS, own, Sown, ref.TURN_RATE, cand)
    assert rc == 0 and np.isnan(part[:, [1, 3]]).all() and np.array_equal(part[:, [0, 2, 4]], out[:, [0, 2, 4]], equal_nan=True)
    assert np.isnan(psum[[0, 2]][:, [1, 3]]).all() and (psum[[1, 3]][:, [1, 3]] == -1).all() and np.array_equal(psum[:, [0, 2, 4]], summary[:, [0, 2, 4]])
    # a NaN in the own ship or in its covariance: everything is NaN
    for o, s in ((np.array([own[0], np.nan, own[2], own[3]]), Sown), (own, np.array([1.0, np.nan, 1.0]))):
        rc, dead, dsum = _raw(ctxs[lib_nx], x, P, Phi, Q, K, DT, RADIUS, o, s, ref.TURN_RATE, ref.CANDIDATES)
        assert rc == 0 and np.isnan(dead).all() and np.isnan(dsum[[0, 2]]).all() and (dsum[[1, 3]] == -1).all()


def test_raw_abi_errors_and_the_call_behind_them(ctxs):
    """A bad nx, K, G, n, R, dt or w, a candidate out of range or infinite, an infinite own ship, a null array, a work buffer one byte
    short: MHT_E_INVALID with the sentinels untouched; a call without tracks is MHT_OK and launches nothing; the sizer."""
    from pymht_amd import _lib
    ctx = ctxs[4]
    x, P, own, Sown, Phi, Q, _, _ = cell_case(4, 1, 70)
    x, P = x[:6], P[:6]
    nan, inf = float("nan"), float("inf")
    bad_cand = lambda row: np.vstack([ref.CANDIDATES[:2], [row]])
    for kw in (dict(nx=5), dict(nx=3), dict(K=0), dict(K=65), dict(K=-1), dict(G=0), dict(G=-1), dict(G=4097), dict(n=-1), dict(R=0.0), dict(R=-1.0), dict(R=nan),
               dict(R=inf), dict(dt=0.0), dict(dt=-2.0), dict(dt=nan), dict(dt=inf), dict(w=0.0), dict(w=-0.05), dict(w=nan), dict(w=inf),
               dict(cand=bad_cand([3.2, 1.0, 0.0])), dict(cand=bad_cand([-3.2, 1.0, 0.0])), dict(cand=bad_cand([0.1, -0.5, 0.0])), dict(cand=bad_cand([0.1, 1.0, -1.0])),
               dict(cand=bad_cand([inf, 1.0, 0.0])), dict(cand=bad_cand([0.1, inf, 0.0])), dict(cand=bad_cand([0.1, 1.0, inf])), dict(own=[0.0, inf, 1.0, 1.0]),
               dict(Sown=[1.0, 0.0, inf]), dict(nulls=("Phi",)), dict(nulls=("Q",)), dict(nulls=("x",)), dict(nulls=("P",)), dict(nulls=("own",)), dict(nulls=("Sown",)),
               dict(nulls=("cand",)), dict(nulls=("out",)), dict(nulls=("summary",)), dict(nulls=("work",)), dict(short=1)):
        rc, out, summary = _raw(ctx, x, P, Phi, Q, kw.get("K", 3), kw.get("dt", DT), kw.get("R", RADIUS), kw.get("own", own), kw.get("Sown", Sown),
                                kw.get("w", ref.TURN_RATE), kw.get("cand", ref.CANDIDATES), nulls=kw.get("nulls", ()), nx=kw.get("nx"), n=kw.get("n"), G=kw.get("G"),
                                short=kw.get("short", 0))
        assert rc == _lib.MHT_E_INVALID and ctx.lib.mht_last_error() and (out == SENTINEL).all() and (summary == SENTINEL).all(), kw
    assert ctx.lib.mht_trial_manoeuvres(ctx.handle, 4, 0, 5, 3, DT, RADIUS, None, None, None, None, None, None, 0.05, None, None, None, None, 0) == _lib.MHT_OK
    for lib in (ctxs[4].lib, ctxs[6].lib):
        up = lambda b: (b + 255) // 256 * 256      # (the trajectories, the partials, the staging for six states, the candidates)
        size = lambda n, G, K: up(8 * (5 * (K + 1) * (n + G) + 4 * G * ((n + 255) // 256) + 27 * (n + G) + 3 * G))
        assert lib.mht_trial_work_bytes(70, 5, 7) == size(70, 5, 7) and lib.mht_trial_work_bytes(300, 5, 1) == size(300, 5, 1)
        assert lib.mht_trial_work_bytes(2000, 64, 24) == size(2000, 64, 24) and lib.mht_trial_work_bytes(1, 4096, 64) == size(1, 4096, 64)
        assert lib.mht_trial_work_bytes(0, 5, 3) == 0 and lib.mht_trial_work_bytes(-1, 5, 3) == 0 and lib.mht_trial_work_bytes(5, 0, 3) == 0
        assert lib.mht_trial_work_bytes(5, 4097, 3) == 0 and lib.mht_trial_work_bytes(5, 5, 0) == 0 and lib.mht_trial_work_bytes(5, 5, 65) == 0
    rc, out, summary = _raw(ctx, x, P, Phi, Q, 3, DT, RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES)
    assert rc == _lib.MHT_OK and not (out == SENTINEL).any() and not (summary == SENTINEL).any()


def test_module_function_gives_the_seams_bits(ctxs):
    """evaluation.trial_manoeuvres on a Context and on a device ordinal: the raw call's table and summary, the indices as int64"""
    from pymht_amd import evaluation
    x, P, own, Sown, Phi, Q, _, _ = cell_case(6, 7, 70)
    rc, out, summary = _raw(ctxs[6], x, P, Phi, Q, 7, DT, RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES)
    assert rc == 0
    cov = np.array([[Sown[0], Sown[1]], [Sown[1], Sown[2]]])
    for kw in (dict(ctx=ctxs[6]), dict(device=0), dict(ctx=ctxs[4])):
        res = evaluation.trial_manoeuvres(x, P, Phi, Q, 7, DT, RADIUS, own, ref.CANDIDATES, ref.TURN_RATE, ownCovariance=cov, **kw)
        assert sorted(res) == sorted(ref.NAMES + ref.SUMMARY + ("candidates",))
        assert all(np.array_equal(res[k], out[f], equal_nan=True) for f, k in enumerate(ref.NAMES))
        assert all(np.array_equal(res[k], summary[f], equal_nan=True) for f, k in enumerate(ref.SUMMARY))
        assert res["pcArg"].dtype == np.int64 and res["dcpaArg"].dtype == np.int64 and np.array_equal(res["candidates"], ref.CANDIDATES)


def test_tracker_trial_manoeuvres_of_a_short_run():
    """Four targets initiated from known states, five scans of their true positions plus unit noise (no clutter).  The own ship runs
    head-on into target 0, 40 s away; getTrialManoeuvres over 60 s, radius 50, course changes 0, +-60 degrees and speed factors 1 and
    0.5 after a delay of 5 s: the figures are trial_ref's on the tracker's own getFilteredTracks() last rows, under the criterion with
    mpmath's pc; standing on at full speed has a larger pcMax, against target 0, than either 60 degree alteration at full speed; `best`
    is evaluation.trial_best of the summary, one of the alterations, with a smaller pcMax and a larger dcpaMin than standing on."""
    from pymht_amd import evaluation
    from pymht_amd.models import pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    period, t0, horizon, radius, w = 2.5, 1000.0, 60.0, 50.0, 0.05
    x0 = np.array([[0.0, 0.0, -5.0, 0.0], [2000.0, 2000.0, 6.0, 3.0], [-2000.0, 1800.0, -7.0, 2.0], [-1900.0, -2100.0, -3.0, -8.0]])
    rng = np.random.default_rng(8)
    trk = Tracker(pv, period, 2e-6, 1e-4, P_d=0.9, N=3, eta2=5.99, useInitiator=False)
    try:
        for s in x0:
            trk.initiateTarget(Target(t0, None, s.copy(), pv.P0))
        for k in range(1, 6):
            z = x0[:, :2] + x0[:, 2:] * (k * period) + rng.normal(size=(4, 2))
            trk.addMeasurementList(MeasurementList(t0 + k * period, z))
        last = [(xf[-1], Pf[-1]) for xf, Pf in trk.getFilteredTracks()]
        assert len(last) == 4
        x, P = np.array([a for a, _ in last]), np.array([b for _, b in last])
        target = int(np.argmin(np.hypot(*(x[:, :2] - (x0[0, :2] + x0[0, 2:] * 5 * period)).T)))
        own = np.array([x[target, 0] - 400.0, x[target, 1], 5.0, 0.0])      # closing at 10 m/s from 400 m
        cov = np.diag([4.0, 9.0])
        deg60 = np.pi / 3
        got = trk.getTrialManoeuvres(horizon, radius, own, [0.0, deg60, -deg60], w, speedFactors=(1.0, 0.5), delay=5.0, ownCovariance=cov, steps=12)
        cand = np.array([[a, f, 5.0] for a in (0.0, deg60, -deg60) for f in (1.0, 0.5)])
        assert sorted(got) == sorted(ref.NAMES + ref.SUMMARY + ("candidates", "ids", "best")) and np.array_equal(got["candidates"], cand)
        assert len(got["ids"]) == 4 and len(set(got["ids"])) == 4 and got["pc"].shape == (6, 4)
        Phi, Q = eref.model_matrices(pv, 5.0)
        args = (x, P, Phi, Q, 12, 5.0, radius, own, [4.0, 0.0, 9.0], w, cand)
        truth, f64 = ref.manoeuvres(*args, truth=True), ref.manoeuvres(*args)
        hold("getTrialManoeuvres", {k: got[k] for k in ref.NAMES}, truth, f64, 5.0)
        want = ref.fold(got["pc"], got["dcpa"])
        assert all(np.array_equal(got[k], want[k], equal_nan=True) for k in ref.SUMMARY)
        print("pcMax", got["pcMax"], "dcpaMin", got["dcpaMin"], "best", got["best"])
        assert (got["pcMax"][0] > got["pcMax"][[2, 4]]).all() and got["pcArg"][0] == target and got["dcpaArg"][0] == target
        assert got["best"] == evaluation.trial_best(got["pcMax"], got["dcpaMin"]) and got["best"] in (2, 3, 4, 5)
        assert got["pcMax"][got["best"]] < got["pcMax"][0] and got["dcpaMin"][got["best"]] > got["dcpaMin"][0]
        default = trk.getTrialManoeuvres(horizon, radius, own, [0.0], w)      # steps = 24, dt = 2.5, one candidate: stand on
        assert default["pc"].shape == (1, 4) and default["best"] == 0 and np.array_equal(default["candidates"], [[0.0, 1.0, 0.0]])
        for bad in (dict(horizon=0.0), dict(radius=-1.0), dict(steps=65), dict(steps=0), dict(ownShip=np.zeros(3)), dict(ownCovariance=np.eye(3)), dict(turnRate=0.0),
                    dict(turnRate=float("nan")), dict(courseChanges=[4.0]), dict(courseChanges=[]), dict(speedFactors=[-1.0]), dict(delay=-1.0), dict(delay=float("inf"))):
            kw = dict(horizon=horizon, radius=radius, ownShip=own, courseChanges=[0.0, 0.5], turnRate=w)
            kw.update(bad)
            with pytest.raises(ValueError, match="getTrialManoeuvres"):
                trk.getTrialManoeuvres(**kw)
    finally:
        trk.close()


def test_tracker_without_tracks_makes_no_device_call():
    from pymht_amd.models import pv
    from pymht_amd.tracker import Tracker
    trk = Tracker(pv, 2.5, 2e-6, 1e-4, P_d=0.9, N=3, eta2=5.99, useInitiator=False)
    try:
        none = trk.getTrialManoeuvres(30.0, 50.0, [0.0, 0.0, 1.0, 1.0], [0.0, 0.5], 0.05)
        assert none["ids"] == [] and none["best"] is None and all(none[k].shape == (2, 0) for k in ref.NAMES) and (none["pcArg"] == -1).all()
    finally:
        trk.close()
