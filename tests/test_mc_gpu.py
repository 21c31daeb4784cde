"""GPU: the Monte-Carlo encounter engine on the device (`mht_mc_encounters`, include/mht_amd.h; csrc/mht_mc.hip) against its host twin
(tests/hostmath/mc_host.cpp, the same header compiled for the CPU) under the borderline rule of tests/mc_ref.py -- the generator is
integer only, so only the device's sin, cos and log can move a particle, and only a borderline one across the radius; the scenes have
none, so the counts are expected to be EQUAL and every test prints how many cells differed --, the seam's refusals, and the drop-in
path Tracker.getMonteCarloEncounters on a models/pv and a models/ct tracker.  Nothing here is larger than 70 targets and 4 096
particles, except one target with 65 536."""
import numpy as np
import pytest

import encounter_ref as eref
import mc_ref as ref
from test_encounter_gpu import guard_untouched, guarded_work

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return ref.build_twin(tmp_path_factory.mktemp("mc_twin"))


def _raw(ctx, sc, nulls=(), short=0, guard=0, **over):
    """One call of the seam on a scene of tests/mc_ref.py, the outputs preset to a sentinel and the work buffer to a pattern: (return code,
    dict of the outputs).  guard > 0: that many bytes of the pattern lie behind the sizer's figure and must be the pattern after the call."""
    import torch
    dev = ctx.device
    N, T, G = sc["x"].shape[1], len(sc["first"]) - 1, len(sc["own"])
    xp, Pp = eref.pack(sc["x"], sc["P"])
    host = dict(Phi=np.ascontiguousarray(sc["Phi"]), Q=np.ascontiguousarray(sc["Q"]))
    first = np.ascontiguousarray(over.pop("first", sc["first"]), dtype=np.int32)
    arrays = dict(x=torch.from_numpy(xp).to(dev), P=torch.from_numpy(Pp).to(dev), first=torch.from_numpy(first).to(dev),
                  cdf=torch.from_numpy(sc["cdf"]).to(dev), own=torch.from_numpy(sc["own"]).to(dev))
    o = ref.outputs(G, sc["K"], T)
    for k in ("within", "ever", "valid", "status"):
        arrays[k] = torch.from_numpy(o[k].view(np.int32)).to(dev)
    a = dict(nx=N, transition=1 if sc["ct"] else 0, nComp=len(sc["x"]), T=T, G=G, K=sc["K"], S=sc["S"], seed=sc["seed"], dt=sc["dt"], R=sc["R"])
    a.update(over)
    need = int(ctx.lib.mht_mc_work_bytes(N, len(sc["x"]), T, G, sc["K"], sc["S"]))
    assert need > 0
    arrays["work"] = guarded_work(need, guard, dev)
    ptr = lambda k: None if k in nulls else host[k].ctypes.data if k in host else arrays[k].data_ptr()
    torch.cuda.synchronize(dev)
    rc = ctx.lib.mht_mc_encounters(None if "ctx" in nulls else ctx.handle, a["nx"], a["transition"], a["nComp"], a["T"], a["G"], a["K"], a["S"], a["seed"], a["dt"], a["R"],
                                   ptr("Phi"), ptr("Q"), ptr("x"), ptr("P"), ptr("first"), ptr("cdf"), ptr("own"), ptr("within"), ptr("ever"), ptr("valid"),
                                   ptr("status"), ptr("work"), need - short)
    torch.cuda.synchronize(dev)
    assert guard_untouched(arrays["work"], need), "the call wrote behind the work buffer the sizer asks for"
    out = {k: arrays[k].cpu().numpy().view(o[k].dtype) for k in ("within", "ever", "valid", "status")}
    return rc, out


def _untouched(out):
    return all((out[k] == ref.SENTINEL).all() for k in ("within", "ever", "valid")) and (out["status"] == -7).all()


def _hold(label, got, want, sc):
    """The device's counts against the twin's: equal, or -- a last-bit difference of sin, cos or log -- within the reference's
    borderline particles per cell.  Prints and returns the number of cells that differ."""
    assert not any((got[k] == ref.SENTINEL).any() for k in ("within", "ever", "valid")) and not (got["status"] == -7).any(), (label, "a sentinel is left")
    differ = 0
    if not ref.same_counts(got, want):
        border = ref.reference(sc)
        differ = ref.hold_counts(label, got, dict(border, **{k: want[k] for k in ("within", "ever", "valid", "status")}))
    print("%s: %d cells differ from the twin's" % (label, differ))
    return differ


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("name", ["a", "c"])
def test_scenes_a_and_c_equal_the_twin_and_no_sentinel_is_left(ctxs, twin, name, lib_nx):
    sc = ref.scene_a() if name == "a" else ref.scene_c()
    rc, got = _raw(ctxs[lib_nx], sc)
    assert rc == 0
    want = ref.call_twin(twin, sc)
    assert _hold("scene %s, %d-state build" % (name.upper(), lib_nx), got, want, sc) == 0
    assert got["status"][eref.NAN_X] == 1 and got["status"][eref.NAN_P] == 1 and (got["ever"] >= got["within"].max(axis=1)).all()
    assert int(((got["within"] > 0) & (got["within"] < sc["S"])).sum()) >= 40


STRIDES = "3 chunks, G=3, K=5, T=3 (the strides of a workgroup's slab)"


def _shape_scene(kind):
    a, c = ref.scene_a(), ref.scene_c()
    pick = lambda sc, idx, **kw: ref.scene(sc["x"][idx], sc["P"][idx], np.arange(len(idx) + 1), np.ones(len(idx)), sc["Phi"], sc["Q"],
                                           kw.pop("own", sc["own"]), ct=sc["ct"], **kw)
    few = [0, 12, 20, 50]
    if kind == "S=64":
        return pick(a, few, S=64)
    if kind == "S=320":
        return pick(c, few, S=320)
    if kind == "T=1, S=65536":
        return pick(a, [12], S=65536)
    if kind == "T=70 (the factor launch past a wavefront)":
        return dict(a, S=256)
    if kind == "K=1":
        return pick(c, few, K=1, own=np.ascontiguousarray(c["own"][:, :2]), S=512)
    if kind in ("K=64", "G=64"):
        sc = a if kind == "K=64" else c
        G, K = (2, 64) if kind == "K=64" else (64, 5)
        cand = np.array([[0.02 * (g - G // 2), 1.0 - 0.005 * g, 2.0 * (g % 3)] for g in range(G)])
        return pick(sc, few, K=K, dt=1.0, own=ref.own_paths(sc["x"][12, :4], cand, K, 1.0), S=256)
    if kind == "G=1":
        return pick(a, few, own=np.ascontiguousarray(a["own"][:1]), S=512)
    if kind == STRIDES:
        return ref.scene_stride()
    rng = np.random.default_rng(67)
    if kind == "67 components":
        n = 67
        x, P = np.tile(a["x"][12], (n + 2, 1)), np.tile(a["P"][12], (n + 2, 1, 1))
        x[:n, :2] += rng.uniform(-120, 120, (n, 2))
        w = np.append(rng.uniform(0, 1, n), [1.0, 1.0])
        w[[5, 66]] = 0.0
        return ref.scene(x, P, [0, n, n + 1, n + 2], w, a["Phi"], a["Q"], ref.own_paths(a["x"][12, :4], ref.CANDIDATES, ref.K, ref.DT), S=1024)
    assert kind == "a NaN first component among good ones"
    x, P = np.tile(c["x"][12], (7, 1)), np.tile(c["P"][12], (7, 1, 1))
    x[:, :2] += rng.uniform(-60, 60, (7, 2))
    x[2, 3] = np.nan
    return ref.scene(x, P, [0, 2, 5, 7], np.ones(7), c["Phi"], c["Q"], ref.own_paths(c["x"][12, :4], ref.CANDIDATES, ref.K, ref.DT), ct=True, S=512)


@pytest.mark.parametrize("kind", ["S=64", "S=320", "T=1, S=65536", "T=70 (the factor launch past a wavefront)", "K=1", "K=64", "G=1", "G=64", "67 components",
                                  "a NaN first component among good ones", STRIDES])
def test_shapes_at_which_the_kernels_take_another_path(ctxs, twin, kind):
    sc = _shape_scene(kind)
    want = ref.call_twin(twin, sc)
    for lib_nx in (4, 6):
        rc, got = _raw(ctxs[lib_nx], sc)
        assert rc == 0, kind
        assert _hold("%s, %d-state build" % (kind, lib_nx), got, want, sc) == 0
    if kind == STRIDES:
        ref.check_stride_counts(want)
    if kind.startswith("a NaN"):
        assert want["status"].tolist() == [0, 1, 0] and want["valid"].tolist() == [512, 0, 512] and not want["within"][:, :, 1].any()
    assert want["within"].any() and (want["ever"] >= want["within"].max(axis=1)).all()


def test_one_seed_one_result_whatever_the_split(ctxs, twin):
    a = ref.scene_a()
    ctx = ctxs[4]
    rc1, one = _raw(ctx, a)
    rc2, two = _raw(ctx, a)
    assert rc1 == 0 and rc2 == 0 and ref.same_counts(one, two)
    rc3, other = _raw(ctx, dict(a, seed=a["seed"] + 1))
    assert rc3 == 0 and not np.array_equal(other["within"], one["within"]) and np.array_equal(other["status"], one["status"])
    # target 0 alone is cut into 16 chunks of 256 particles, among the 69 others into 8 of 512: the same counts
    alone = ref.scene(a["x"][:1], a["P"][:1], [0, 1], [1.0], a["Phi"], a["Q"], a["own"])
    assert ref.chunks(1, a["S"]) == (16, 256) and ref.chunks(70, a["S"]) == (8, 512)
    rc4, solo = _raw(ctx, alone)
    assert rc4 == 0 and np.array_equal(solo["within"][:, :, 0], one["within"][:, :, 0]) and np.array_equal(solo["ever"][:, 0], one["ever"][:, 0])
    assert solo["within"].any()


def test_the_seam_refuses_and_writes_nothing(ctxs):
    from pymht_amd import _lib
    a = ref.scene_a()
    sc = ref.scene(a["x"][:6], a["P"][:6], [0, 2, 3, 6], np.ones(6), a["Phi"], a["Q"], a["own"], S=128)
    for lib_nx in (4, 6):
        ctx = ctxs[lib_nx]
        rc, out = _raw(ctx, sc)
        assert rc == 0 and not _untouched(out)
        cases = [dict(nulls=(k,)) for k in ("ctx", "Phi", "Q", "x", "P", "first", "cdf", "own", "within", "ever", "valid", "status", "work")]
        cases += [dict(short=1), dict(S=100), dict(S=32), dict(S=(1 << 20) + 64), dict(G=65), dict(G=0), dict(K=0), dict(K=65), dict(nx=5), dict(transition=1),
                  dict(transition=2), dict(T=0), dict(T=7), dict(dt=0.0), dict(R=float("nan")), dict(first=[0, 3, 2, 6]), dict(first=[0, 2, 2, 6]),
                  dict(first=[1, 2, 3, 6]), dict(first=[0, 2, 3, 5])]
        for case in cases:
            rc, out = _raw(ctx, sc, **case)
            assert rc == _lib.MHT_E_INVALID and _untouched(out), (lib_nx, case, rc)
        indefinite = dict(sc, Q=np.diag([1.0, -1.0, 1.0, 1.0]))
        rc, out = _raw(ctx, indefinite)
        assert rc == _lib.MHT_E_INVALID and _untouched(out)
        assert b"positive semidefinite" in ctx.lib.mht_last_error()
        for bad in ((5, 6, 3, 2, 7, 128), (4, 0, 1, 2, 7, 128), (4, 6, 7, 2, 7, 128), (4, 6, 3, 65, 7, 128), (4, 6, 3, 2, 0, 128), (4, 6, 3, 2, 7, 100)):
            assert ctx.lib.mht_mc_work_bytes(*bad) == 0, bad


def _weights(cnllr, target):
    w = np.zeros(len(cnllr))
    for t in np.unique(target):
        at = np.flatnonzero(target == t)
        w[at] = np.exp(-(cnllr[at] - cnllr[at].min()))
    return w


def _scans(model, six):
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    from pymht_amd.utils.scenario import make_scenario
    sc = make_scenario(T=3, radius=300.0, lambda_phi=2e-5, n_scans=12, P_d=0.7, seed=3)
    trk = Tracker(model, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=3, eta2=5.99, useInitiator=False)
    for x0 in sc["x0"]:
        x = np.append(x0, [0.0, 0.0]) if six else x0.copy()
        trk.initiateTarget(Target(sc["t0"], None, x, model.P0, status="preinitialized") if six else Target(sc["t0"], None, x, model.P0))
    for zk, tk in zip(sc["scans"], sc["times"]):
        trk.addMeasurementList(MeasurementList(float(tk), zk))
    return trk


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_tracker_hands_its_leaves_to_the_engine(name):
    from pymht_amd import evaluation, models
    model = getattr(models, name)
    six = name == "ct"
    trk = _scans(model, six)
    try:
        lb = trk.leafBatch()
        assert trk.nTargets >= 2 and len(lb["x"]) > trk.nTargets, "the scene keeps no second hypothesis"
        own = np.array([lb["x"][0, 0] - 300.0, lb["x"][0, 1] + 40.0, 8.0, 0.0])
        deg = np.pi / 180.0
        kw = dict(particles=1024, seed=5, courseChanges=[0.0, 40.0 * deg], turnRate=0.05, steps=12)
        got = trk.getMonteCarloEncounters(60.0, 60.0, own, **kw)
        widen = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64)
        Phi, Q = (widen(model.Phi(5.0, 0.0)), widen(model.Q(5.0))) if six else eref.model_matrices(model, 5.0)
        paths = evaluation.mc_own_paths(own, got["candidates"], 0.05, 12, 5.0)
        P = np.asarray(lb["P"], dtype=np.float64)
        flat = dict(particles=1024, seed=5, transition="ct" if six else "linear", ctx=trk._ctx)
        want = evaluation.mc_encounters(lb["x"], P, lb["target"], _weights(lb["cnllr"], lb["target"]), Phi, Q, 12, 5.0, 60.0, paths, **flat)
        for k in ("within", "ever", "valid", "status", "pc", "pcMax", "tpc", "pEver", "sePcMax", "sePEver", "cdf", "first"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), k
        assert (got["status"] == 0).all() and (got["valid"] == 1024).all() and got["within"].shape == (2, 13, trk.nTargets)
        assert got["ids"] == [int(i) for i in trk._tbl_["id"]] and np.array_equal(got["leafIds"], lb["ID"]) and got["ever"].any()
        assert np.array_equal(got["pEverMax"], got["pEver"].max(axis=1)) and got["best"] == int(np.argmin(got["pEverMax"]))
        assert (got["pEver"] >= got["pcMax"]).all()
        sel = trk._selected_leaves(lb, list(trk.getTrackNodes()))
        assert (sel >= 0).all()
        best = trk.getMonteCarloEncounters(60.0, 60.0, own, hypotheses=False, **kw)
        only = evaluation.mc_encounters(lb["x"][sel], P[sel], lb["target"][sel], np.ones(len(sel)), Phi, Q, 12, 5.0, 60.0, paths, **flat)
        assert all(np.array_equal(best[k], only[k]) for k in ("within", "ever", "valid", "status")) and np.array_equal(best["leafIds"], lb["ID"][sel])
        if six:      # the constant-turn tracker answers here, and the Gaussian rule still refuses it
            with pytest.raises(NotImplementedError):
                trk.getEncounters(60.0, 60.0, own)
        else:
            gh = trk.getGlobalHypotheses(k=8)
            joint = trk.getMonteCarloEncounters(60.0, 60.0, own, weights=gh["leafProbability"], **kw)
            assert (joint["status"] == 0).all() and joint["within"].shape == got["within"].shape
            with pytest.raises(ValueError, match="target"):
                trk.getMonteCarloEncounters(60.0, 60.0, own, weights=np.full(len(lb["x"]), np.nan), **kw)
    finally:
        trk.close()
