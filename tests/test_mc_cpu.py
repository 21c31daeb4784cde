"""CPU: the Monte-Carlo encounter engine's host twin (tests/hostmath/mc_host.cpp, csrc/mht_mc.h compiled for the CPU) against the NumPy
restatement tests/mc_ref.py, which states the borderline rule every comparison of counts here uses; against the closed-form pc of the
Gaussian rule where there is one; and pymht_amd.evaluation's host side (mc_own_paths, every ValueError of mc_encounters) without a
device.

Against the closed form (scene A, seed 12345, S = 4096): |within / S - pck| <= 4 sqrt(max(pck (1 - pck), 1 / S) / S) in every cell where
trial_ref.manoeuvres' pck is finite.  The seed is fixed, so this is a deterministic statement about this draw: the test prints the
largest ratio per path (a prototype of this layout gave 2.50 and 2.55), and four sigma is the margin over that -- a ratio far above it
means the sampler is wrong."""
import numpy as np
import pytest

import encounter_ref as eref
import mc_ref as ref
import trial_ref as tref


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return ref.build_twin(tmp_path_factory.mktemp("mc_twin"))


def _pv():
    from pymht_amd.models import pv
    return pv, *eref.model_matrices(pv, ref.DT)


def test_philox_known_answers_and_normals(twin):
    kat = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for ctr, key, want in kat:
        out = np.zeros(4, dtype=np.uint32)
        twin.mc_philox_host(*ctr, *key, out.ctypes.data)
        assert " ".join("%08x" % v for v in out) == want
        assert " ".join("%08x" % int(v[0]) for v in ref.philox(*ctr, *key)) == want
    for N in (4, 6):
        for p in range(4):
            z = np.full(6, np.nan)
            twin.mc_normals_host(N, p, 3, 5, 12345, z.ctypes.data)
            want = ref.normals(N, np.array([p]), 3, 5, 12345)[:, 0]
            assert np.all(np.abs(z[:N] - want) <= 4 * np.spacing(np.abs(want))), (N, p, z, want)
            assert np.all(np.abs(z[:N]) <= 6.8)
    assert np.sqrt(-2.0 * np.log(ref.uniform(np.uint32(0)))) < 6.8      # the cut of the tails


def test_scene_a_counts_nan_entries_and_a_zero_covariance(twin):
    sc = ref.scene_a()
    got, want = ref.call_twin(twin, sc), ref.reference(sc, "a")
    differ = ref.hold_counts("scene A", got, want)
    print("scene A: %d borderline pairs of %d, %d cells differ" % (int(want["borderWithin"].sum()), want["pairs"], differ))
    assert differ == 0 and not any((got[k] == ref.SENTINEL).any() for k in ("within", "ever", "valid"))
    for e in (eref.NAN_X, eref.NAN_P):
        assert got["status"][e] == 1 and got["valid"][e] == 0 and not got["within"][:, :, e].any() and not got["ever"][:, e].any()
    scored = np.setdiff1d(np.arange(70), [eref.NAN_X, eref.NAN_P])
    assert (got["status"][scored] == 0).all() and (got["valid"][scored] == sc["S"]).all()
    for e in eref.ZERO_P:      # an exactly known state: every particle starts at the same point, where the Gaussian rule gives NaN
        assert set(got["within"][:, 0, e].tolist()) <= {0, sc["S"]}
    assert (got["ever"] >= got["within"].max(axis=1)).all()
    assert int(((got["within"] > 0) & (got["within"] < sc["S"])).sum()) >= 60


def test_scene_a_agrees_with_the_closed_form_within_four_sigma(twin):
    sc = ref.scene_a()
    got = ref.call_twin(twin, sc)
    pck = tref.manoeuvres(sc["x"], sc["P"], sc["Phi"], sc["Q"], sc["K"], sc["dt"], sc["R"], sc["x"][0, :4], np.zeros(3), tref.TURN_RATE, ref.CANDIDATES,
                          pc_mp=False)["pck"]      # [K + 1, G, n]
    S = float(sc["S"])
    pck = np.transpose(pck, (1, 0, 2))
    finite = np.isfinite(pck)
    assert (got["status"][finite.any(axis=(0, 1))] == 0).all()
    ratio = np.abs(got["within"] / S - pck) / np.sqrt(np.fmax(pck * (1.0 - pck), 1.0 / S) / S)
    informative = int((finite & (pck > 1e-3) & (pck < 0.999)).sum())
    print("largest ratio per path: %s, %d informative cells of %d" % ([round(float(np.nanmax(ratio[g][finite[g]])), 2) for g in range(2)], informative, int(finite.sum())))
    assert informative >= 60
    assert (ratio[finite] <= 4.0).all(), float(np.nanmax(ratio[finite]))


def test_ever_sees_a_passage_between_two_steps(twin):
    pv, Phi, _ = _pv()
    x = np.array([[-100.0, 10.0, 40.0, 0.0]])
    own = np.zeros((1, 2, 2))
    sc = ref.scene(x, np.zeros((1, 4, 4)), [0, 1], [1.0], Phi, np.zeros((4, 4)), own, K=1, S=128)
    got, want = ref.call_twin(twin, sc), ref.reference(sc)
    assert ref.hold_counts("passage", got, want) == 0
    assert got["ever"].tolist() == [[128]] and not got["within"].any() and got["status"].tolist() == [0]


def _mixture_scene(weights, x_second=5000.0, n=2, **kw):
    pv, Phi, Q = _pv()
    x = np.zeros((n + 1, 4))
    x[1:n, 0] = x_second
    x[n] = [300.0, 300.0, 1.0, 1.0]
    P = np.tile(np.asarray(pv.P0, dtype=np.float64), (n + 1, 1, 1))
    own = np.zeros((1, ref.K + 1, 2))
    return ref.scene(x, P, [0, n, n + 1], list(weights) + [1.0], Phi, Q, own, **kw)


def test_mixture_picks_components_by_their_weights(twin):
    sc = _mixture_scene((0.25, 0.75))
    got, want = ref.call_twin(twin, sc), ref.reference(sc)
    assert ref.hold_counts("mixture", got, want) == 0
    u = ref.pick_uniform(np.arange(sc["S"], dtype=np.uint64), 0, sc["seed"])
    assert got["within"][0, 0, 0] == int((u < 0.25).sum()) and 0 < got["within"][0, 0, 0] < sc["S"]
    never = ref.call_twin(twin, _mixture_scene((0.0, 1.0)))      # a weight of 0 is never picked: nobody starts inside the disc
    assert never["within"][0, 0, 0] == 0 and never["status"].tolist() == [0, 0]
    last = ref.call_twin(twin, _mixture_scene((1.0, 0.0)))
    assert last["within"][0, 0, 0] == sc["S"]
    # a target of one component: the counts of the same component alone at the same target index, bit for bit
    one = _mixture_scene((1.0, 0.0))
    alone = ref.scene(one["x"][[0, 2]], one["P"][[0, 2]], [0, 1, 2], [1.0, 1.0], one["Phi"], one["Q"], one["own"])
    assert ref.same_counts(ref.call_twin(twin, alone), last)


def test_a_target_of_67_components(twin):
    rng = np.random.default_rng(67)
    pv, Phi, Q = _pv()
    n = 67
    x = np.zeros((n + 1, 4))
    x[:n, :2] = rng.uniform(-150, 150, (n, 2))
    x[:n, 2:] = rng.uniform(-5, 5, (n, 2))
    x[n] = [40.0, -30.0, 1.0, 2.0]
    P = np.tile(np.asarray(pv.P0, dtype=np.float64), (n + 1, 1, 1))
    w = np.append(rng.uniform(0.0, 1.0, n), 1.0)
    w[[3, 40]] = 0.0
    sc = ref.scene(x, P, [0, n, n + 1], w, Phi, Q, np.zeros((2, ref.K + 1, 2)), S=1024)
    got, want = ref.call_twin(twin, sc), ref.reference(sc)
    assert ref.hold_counts("67 components", got, want) == 0 and 0 < got["within"][0, 0, 0] < 1024


def test_three_chunks_three_paths_three_targets(twin):
    """mc_ref.scene_stride: the reference alone satisfies the case's conditions, and the twin's counts are the reference's"""
    sc = ref.scene_stride()
    got, want = ref.call_twin(twin, sc), ref.reference(sc)
    ref.check_stride_counts(want)
    assert ref.hold_counts("strides", got, want) == 0
    ref.check_stride_counts(got)


def test_scene_c_constant_turn(twin):
    sc = ref.scene_c()
    got, want = ref.call_twin(twin, sc), ref.reference(sc, "c")
    differ = ref.hold_counts("scene C", got, want)
    live = int(((got["within"] > 0) & (got["within"] < sc["S"])).sum())
    print("scene C: %d borderline pairs, %d cells differ, %d cells with 0 < count < S" % (int(want["borderWithin"].sum()), differ, live))
    assert differ == 0 and live >= 40 and (got["ever"] >= got["within"].max(axis=1)).all()
    assert got["status"][eref.NAN_X] == 1 and got["status"][eref.NAN_P] == 1


def test_constant_turn_without_noise_is_the_circular_arc(twin):
    """P = 0, Q = 0, w = 0.05: the positions against the closed form in np.longdouble, by the project's criterion -- the error at most 8
    times the float64 NumPy evaluation's (tests/mc_ref.step iterated), with a floor of one eps of the path's extent."""
    L = np.longdouble
    K, dt, w = 24, 5.0, 0.05
    x0 = np.array([100.0, -50.0, 6.0, 3.0, w, 0.0])
    out = np.zeros((K + 1, 6))
    assert twin.mc_path_host(6, 1, K, dt, None, np.zeros((6, 6)).ctypes.data, x0.ctypes.data, 7, 0, 0, out.ctypes.data) == 0
    X, mine = x0[:, None].copy(), [x0[:2].copy()]
    for _ in range(K):
        X = ref.step(X, np.zeros((6, 1)), None, np.zeros((6, 6)), dt, True)
        mine.append(X[:2, 0].copy())
    t = L(dt) * np.arange(K + 1).astype(L)
    sw, cw = np.sin(L(w) * t) / L(w), (1 - np.cos(L(w) * t)) / L(w)
    truth = np.stack([L(x0[0]) + sw * L(x0[2]) - cw * L(x0[3]), L(x0[1]) + cw * L(x0[2]) + sw * L(x0[3])], axis=1)
    e_twin, e_np = float(np.abs(out[:, :2].astype(L) - truth).max()), float(np.abs(np.array(mine).astype(L) - truth).max())
    print("arc: twin %.3g, NumPy %.3g" % (e_twin, e_np))
    assert e_twin <= 8 * max(e_np, ref.EPS * float(np.abs(truth).max()))
    assert np.all(out[:, 4] == w) and np.all(out[:, 5] == 0.0)


def test_constant_turn_at_rate_zero_is_the_linear_walk(twin):
    from pymht_amd.models import ct
    c = ref.scene_c()
    x, P, Q = c["x"].copy(), c["P"].copy(), c["Q"].copy()
    x[:, 4:] = 0.0
    P[:, 4:, :] = P[:, :, 4:] = 0.0
    Q[4:, :] = Q[:, 4:] = 0.0
    turn = ref.scene(x, P, c["first"], np.ones(len(x)), c["Phi"], Q, c["own"], ct=True, S=1024)
    line = dict(turn, ct=False, Phi=np.asarray(ct.Phi(ref.DT, 0.0), dtype=np.float64))
    a, b = ref.call_twin(twin, turn), ref.call_twin(twin, line)
    assert ref.same_counts(a, b) and a["within"].any()


def test_factor(twin):
    from pymht_amd.models import ct
    x, P = eref.make_batch(_pv()[0], 70, seed=3)
    for e in range(70):
        if e in (eref.NAN_X, eref.NAN_P):
            continue
        L = np.zeros((4, 4))
        assert twin.mc_factor_host(4, 0, np.ascontiguousarray(P[e]).ctypes.data, L.ctypes.data) == 0
        assert np.array_equal(L, ref.factor(P[e])[0])
        assert np.abs(L @ L.T - P[e]).max() <= 64 * ref.EPS * max(P[e].diagonal().max(), 1e-300)
    Q = np.ascontiguousarray(np.asarray(ct.Q(5.0), dtype=np.float32).astype(np.float64))
    L = np.zeros((6, 6))
    assert twin.mc_factor_host(6, 1, Q.ctypes.data, L.ctypes.data) == 0
    assert int((L.diagonal() == 0).sum()) == 3 and np.array_equal(L, ref.factor(Q, own=True)[0])
    assert np.abs(L @ L.T - Q).max() <= 2.0 ** -20 * Q.diagonal().max()
    assert twin.mc_factor_host(6, 0, Q.ctypes.data, L.ctypes.data) == 2      # (the components' rule calls this Q indefinite: csrc/mht_mc.h)
    bad = np.diag([1.0, -1.0, 1.0, 1.0])
    L4 = np.zeros((4, 4))
    assert twin.mc_factor_host(4, 0, bad.ctypes.data, L4.ctypes.data) == 2 and ref.factor(bad)[1] == 2
    pv, Phi, Qpv = _pv()
    sc = ref.scene(np.zeros((2, 4)), np.array([bad, np.eye(4)]), [0, 1, 2], [1.0, 1.0], Phi, Qpv, np.zeros((1, 2, 2)), K=1, S=64)
    got = ref.call_twin(twin, sc)
    assert got["status"].tolist() == [2, 0] and got["valid"].tolist() == [0, 64] and not got["within"][:, :, 0].any() and got["within"][0, 0, 1] == 64


def test_the_split_of_a_targets_particles(twin):
    out = np.zeros(2, dtype=np.int32)
    for T, S in ((1, 64), (1, 320), (1, 65536), (70, 4096), (500, 65536), (1024, 1 << 20), (5000, 4096), (3, 1 << 20)):
        twin.mc_chunks_host(T, S, out.ctypes.data)
        chunks, slab = int(out[0]), int(out[1])
        assert (chunks, slab) == ref.chunks(T, S)
        assert slab % 256 == 0 and (chunks - 1) * slab < S <= chunks * slab and (T >= 1024) <= (chunks == 1)


def test_own_paths_are_the_trial_manoeuvres_paths_bit_for_bit():
    from pymht_amd import evaluation
    own = np.array([-400.0, 35.0, 6.0, 3.0])
    for K, dt in ((7, 5.0), (24, 2.5), (1, 60.0)):
        want = np.ascontiguousarray(tref.candidate_path(own, np.zeros(3), tref.TURN_RATE, tref.CANDIDATES, K, dt)[0].transpose(1, 0, 2))
        got = evaluation.mc_own_paths(own, tref.CANDIDATES, tref.TURN_RATE, K, dt)
        assert got.dtype == np.float64 and got.shape == (len(tref.CANDIDATES), K + 1, 2) and got.tobytes() == want.tobytes()
    assert np.isnan(evaluation.mc_own_paths(own, [[np.nan, 1.0, 0.0], [0.0, 1.0, 0.0]], 0.05, 3, 5.0)[0]).all()


def test_every_value_error_is_raised_without_a_device(monkeypatch):
    from pymht_amd import evaluation

    def no_device(*a, **kw):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(evaluation, "Context", no_device)
    pv, Phi, Q = _pv()
    x, P = np.zeros((3, 4)), np.tile(np.eye(4), (3, 1, 1))
    own = np.zeros((2, 5, 2))
    good = dict(x=x, P=P, target=[0, 0, 1], weight=[1.0, 2.0, 1.0], Phi=Phi, Q=Q, steps=4, dt=5.0, radius=50.0, ownPaths=own)
    bad = [dict(x=np.zeros((3, 5))), dict(P=P[:2]), dict(Phi=np.eye(6)), dict(Q=np.full((4, 4), np.nan)), dict(steps=0), dict(steps=65), dict(steps=2.0),
           dict(dt=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(particles=100), dict(particles=32), dict(particles=(1 << 20) + 64), dict(particles=64.0),
           dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5), dict(transition="ct"), dict(transition="arc"), dict(ownPaths=np.zeros((2, 4, 2))),
           dict(ownPaths=np.zeros((65, 5, 2))), dict(ownPaths=np.zeros((0, 5, 2))), dict(ownPaths=np.full((2, 5, 2), np.nan)), dict(target=[0, 0]),
           dict(target=[0.0, 0.0, 1.0]), dict(weight=[1.0, 2.0]), dict(weight=[1.0, -2.0, 1.0]), dict(weight=[0.0, 0.0, 1.0]), dict(weight=[1.0, np.inf, 1.0]),
           dict(weight=[1.0, np.nan, 1.0])]
    for change in bad:
        with pytest.raises(ValueError, match="mc_encounters"):
            evaluation.mc_encounters(**dict(good, **change))
    with pytest.raises(ValueError, match="target 7"):
        evaluation.mc_encounters(**dict(good, target=[7, 7, 1], weight=[0.0, 0.0, 1.0]))
    none = evaluation.mc_encounters(np.zeros((0, 4)), np.zeros((0, 4, 4)), np.zeros(0, dtype=np.int64), np.zeros(0), Phi, Q, 4, 5.0, 50.0, own)
    assert none["within"].shape == (2, 5, 0) and none["ever"].shape == (2, 0) and none["pcMax"].shape == (2, 0) and none["pEver"].shape == (2, 0)
    assert none["valid"].shape == (0,) and none["status"].shape == (0,) and len(none["targets"]) == 0 and none["first"].tolist() == [0]
    for call in (lambda: evaluation.mc_own_paths([0.0, 0.0, 1.0], tref.CANDIDATES, 0.05, 4, 5.0), lambda: evaluation.mc_own_paths(np.zeros(4), tref.CANDIDATES, 0.0, 4, 5.0),
                 lambda: evaluation.mc_own_paths(np.zeros(4), tref.CANDIDATES, 0.05, 0, 5.0), lambda: evaluation.mc_own_paths(np.zeros(4), [[4.0, 1.0, 0.0]], 0.05, 4, 5.0)):
        with pytest.raises(ValueError, match="mc_own_paths"):
            call()


def test_the_hosts_figures():
    """pc, pcMax with the EARLIEST largest, pEver, the standard errors with their floor of one particle, NaN where valid is 0"""
    from pymht_amd import evaluation
    within = np.array([[[0, 10], [32, 10], [32, 10], [5, 10]]], dtype=np.uint32)      # [1, 4, 2]
    d = evaluation.mc_derive(within, np.array([[40, 10]], dtype=np.uint32), np.array([64, 0], dtype=np.uint32), 2.5)
    assert d["pc"][0, :, 0].tolist() == [0.0, 0.5, 0.5, 5 / 64] and np.isnan(d["pc"][0, :, 1]).all()
    assert d["pcMax"][0, 0] == 0.5 and d["tpc"][0, 0] == 2.5 and np.isnan(d["pcMax"][0, 1]) and np.isnan(d["tpc"][0, 1])
    assert d["pEver"][0, 0] == 40 / 64 and np.isnan(d["pEver"][0, 1]) and np.isnan(d["sePEver"][0, 1])
    assert d["sePcMax"][0, 0] == np.sqrt(0.25 / 64) and d["sePEver"][0, 0] == np.sqrt((40 / 64) * (24 / 64) / 64)
    assert evaluation.mc_standard_error(np.array([0.0, 1.0]), np.array([64, 64]))[0] == 1.0 / 64
