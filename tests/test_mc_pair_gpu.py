"""GPU: the pair engine on the device (`mht_mc_pair_encounters`, include/mht_amd.h; csrc/mht_mc_pair.hip) against its host twin
(tests/hostmath/mc_pair_host.cpp, the same header compiled for the CPU) under the borderline rule of tests/mc_pair_ref.py -- the
generator is integer only, so only the device's sin, cos and log can move a particle, and only a borderline one across the radius; the
scenes have none, so the counts are expected to be EQUAL and every test prints how many cells differed --, the seam's refusals, and the
drop-in path Tracker.getMonteCarloPairEncounters on a models/pv and a models/ct tracker.  The outputs are preset to a sentinel.  Nothing
here is larger than 2 415 pairs of 1 024 particles, except one pair with 65 536."""
import numpy as np
import pytest

import encounter_ref as eref
import mc_pair_ref as pref
import mc_ref as ref
from test_encounter_gpu import guard_untouched, guarded_work
from test_mc_gpu import _scans, _weights

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
    return pref.build_twin(tmp_path_factory.mktemp("mc_pair_twin"))


def _raw(ctx, sc, pairs, nulls=(), short=0, guard=0, **over):
    """One call of the seam on a scene of tests/mc_ref.py and pairs [n, 2], the outputs preset to a sentinel and the work buffer to a pattern:
    (return code, outputs).  guard > 0: that many bytes of the pattern lie behind the sizer's figure and must be the pattern after the call."""
    import torch
    dev = ctx.device
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    N, T, n = sc["x"].shape[1], len(sc["first"]) - 1, len(pairs)
    xp, Pp = eref.pack(sc["x"], sc["P"])
    host = dict(Phi=np.ascontiguousarray(sc["Phi"]), Q=np.ascontiguousarray(sc["Q"]))
    first = np.ascontiguousarray(over.pop("first", sc["first"]), dtype=np.int32)
    arrays = dict(x=torch.from_numpy(xp).to(dev), P=torch.from_numpy(Pp).to(dev), first=torch.from_numpy(first).to(dev),
                  cdf=torch.from_numpy(sc["cdf"]).to(dev), pairs=torch.from_numpy(pairs).to(dev))
    o = pref.outputs(sc["K"], n)
    for k in pref.COUNTS:
        arrays[k] = torch.from_numpy(o[k].view(np.int32)).to(dev)
    a = dict(nx=N, transition=1 if sc["ct"] else 0, nComp=len(sc["x"]), T=T, nPair=n, K=sc["K"], S=sc["S"], seed=sc["seed"], dt=sc["dt"], R=sc["R"])
    a.update(over)
    need = int(ctx.lib.mht_mc_pair_work_bytes(N, len(sc["x"]), T, n, sc["K"], sc["S"]))
    assert need > 0 and need == pref.work_bytes(N, len(sc["x"]), T, n, sc["K"], sc["S"])
    arrays["work"] = guarded_work(need, guard, dev)
    ptr = lambda k: None if k in nulls else host[k].ctypes.data if k in host else arrays[k].data_ptr()
    torch.cuda.synchronize(dev)
    rc = ctx.lib.mht_mc_pair_encounters(None if "ctx" in nulls else ctx.handle, a["nx"], a["transition"], a["nComp"], a["T"], a["nPair"], a["K"], a["S"], a["seed"],
                                        a["dt"], a["R"], ptr("Phi"), ptr("Q"), ptr("x"), ptr("P"), ptr("first"), ptr("cdf"), ptr("pairs"), ptr("within"),
                                        ptr("firstAt"), ptr("ever"), ptr("valid"), ptr("status"), ptr("work"), need - short)
    torch.cuda.synchronize(dev)
    assert guard_untouched(arrays["work"], need), "the call wrote behind the work buffer the sizer asks for"
    return rc, {k: arrays[k].cpu().numpy().view(o[k].dtype) for k in pref.COUNTS}


def _hold(label, got, want, sc, pairs):
    """The device's counts against the twin's: equal, or -- a last-bit difference of sin, cos or log -- within the reference's
    borderline particles per cell.  Prints and returns the number of cells that differ."""
    assert not any((got[k] == pref.SENTINEL).any() for k in ("within", "firstAt", "ever", "valid")) and not (got["status"] == -7).any(), (label, "a sentinel is left")
    differ = 0
    if not pref.same_counts(got, want):
        border = pref.encounters(sc, pairs)
        differ = pref.hold_counts(label, got, dict(border, **{k: want[k] for k in pref.COUNTS}))
    print("%s: %d cells differ from the twin's" % (label, differ))
    pref.check_invariants(got)
    return differ


@pytest.fixture(scope="module")
def scene_a_1024(twin):
    sc = dict(ref.scene_a(), S=1024)
    pairs = pref.all_pairs(70)
    return sc, pairs, pref.call_twin(twin, sc, pairs)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_all_pairs_of_scene_a_equal_the_twin(ctxs, scene_a_1024, lib_nx):
    sc, pairs, want = scene_a_1024
    assert ref.chunks(len(pairs), sc["S"]) == (1, 1024)      # one chunk, four trips of the loop
    rc, got = _raw(ctxs[lib_nx], sc, pairs)
    assert rc == 0
    assert _hold("scene A, all pairs, %d-state build" % lib_nx, got, want, sc, pairs) == 0
    touched = np.isin(pairs, [eref.NAN_X, eref.NAN_P]).any(axis=1)
    assert np.array_equal(got["status"] == 1, touched) and int(touched.sum()) == 137 and (got["status"][~touched] == 0).all()
    assert int(((got["ever"] > 0) & (got["ever"] < sc["S"])).sum()) >= 1000 and int((got["firstAt"][1:] > 0).sum()) >= 1000


def test_64_pairs_of_scene_c_in_16_chunks(ctxs, twin):
    sc = ref.scene_c()
    pairs = pref.all_pairs(70)[np.arange(64) * 37 % 2415]
    assert ref.chunks(64, sc["S"]) == (16, 256)
    want = pref.call_twin(twin, sc, pairs)
    for lib_nx in (4, 6):
        rc, got = _raw(ctxs[lib_nx], sc, pairs)
        assert rc == 0
        assert _hold("scene C, 64 pairs, %d-state build" % lib_nx, got, want, sc, pairs) == 0
    assert (want["status"] == 1).any() and int(((want["ever"] > 0) & (want["ever"] < sc["S"])).sum()) >= 20


FEW = [[27, 62], [56, 54], [1, 12], [13, 41]]      # (pairs that come inside at every step of scenes A and C, and not with every particle)
OWN0 = np.zeros((1, ref.K + 1, 2))      # (a scene of tests/mc_ref.py carries own paths; they do not enter a pair's counts)
KINDS = ["S=64", "S=320", "nPair=1, S=65536", "nPair=1030", "K=1", "K=63", "K=64", "67 components", "a NaN first component next to a good pair",
         "both orders and a duplicate"]


def _shape_scene(kind):
    a, c = ref.scene_a(), ref.scene_c()
    if kind == "S=64":
        return dict(a, S=64), FEW
    if kind == "S=320":
        return dict(c, S=320), FEW
    if kind == "nPair=1, S=65536":
        return dict(a, S=65536), [[62, 27]]
    if kind == "nPair=1030":
        return dict(c, S=256), pref.all_pairs(70)[:1030]
    if kind in ("K=1", "K=63", "K=64"):
        K = int(kind[2:])
        return dict(c if K == 63 else a, K=K, dt=35.0 / K, S=1024), FEW
    rng = np.random.default_rng(67)
    if kind == "67 components":
        n = 67
        x, P = np.tile(a["x"][12], (n + 2, 1)), np.tile(a["P"][12], (n + 2, 1, 1))
        x[:n, :2] += rng.uniform(-120, 120, (n, 2))
        x[n + 1, :2] += [60.0, -40.0]
        w = np.append(rng.uniform(0, 1, n), [1.0, 1.0])
        w[[5, 66]] = 0.0
        return ref.scene(x, P, [0, n, n + 1, n + 2], w, a["Phi"], a["Q"], OWN0, S=1024), [[0, 1], [2, 0], [1, 2]]
    if kind.startswith("a NaN"):
        x, P = np.tile(c["x"][12], (7, 1)), np.tile(c["P"][12], (7, 1, 1))
        x[:, :2] += rng.uniform(-60, 60, (7, 2))
        x[2, 3] = np.nan
        return ref.scene(x, P, [0, 2, 5, 7], np.ones(7), c["Phi"], c["Q"], OWN0, ct=True, S=512), [[0, 1], [0, 2], [2, 1]]
    assert kind == "both orders and a duplicate"
    return dict(a, S=512), [[27, 62], [62, 27], [27, 62], [54, 56], [56, 54]]


@pytest.mark.parametrize("kind", KINDS)
def test_shapes_at_which_the_kernels_take_another_path(ctxs, twin, kind):
    sc, pairs = _shape_scene(kind)
    pairs = np.asarray(pairs, dtype=np.int32)
    if sc["K"] != ref.K:      # (Phi and Q of the scene's own step)
        from pymht_amd.models import ct, pv
        if sc["ct"]:
            sc = dict(sc, Q=np.asarray(ct.Q(sc["dt"]), dtype=np.float32).astype(np.float64))
        else:
            Phi, Q = eref.model_matrices(pv, sc["dt"])
            sc = dict(sc, Phi=Phi, Q=Q)
    want = pref.call_twin(twin, sc, pairs)
    for lib_nx in (4, 6):
        rc, got = _raw(ctxs[lib_nx], sc, pairs)
        assert rc == 0, kind
        assert _hold("%s, %d-state build" % (kind, lib_nx), got, want, sc, pairs) == 0
    assert want["within"].any() and want["ever"].any() and want["firstAt"][1:].any()
    if kind == "S=320":
        assert ref.chunks(4, 320) == (2, 256)      # a last chunk of 64
    if kind == "nPair=1, S=65536":
        assert ref.chunks(1, 65536) == (256, 256)
    if kind == "K=64":
        assert want["within"].shape == (65, 4) and want["within"][64].any() and want["firstAt"][64].any()      # the 65th word of a lane's two
    if kind.startswith("a NaN"):
        assert want["status"].tolist() == [1, 0, 1] and want["valid"].tolist() == [0, 512, 0] and not want["within"][:, [0, 2]].any()
    if kind.startswith("both"):
        assert all(np.array_equal(want[k][..., 0], want[k][..., j]) for k in pref.COUNTS for j in (1, 2))
        assert all(np.array_equal(want[k][..., 3], want[k][..., 4]) for k in pref.COUNTS)


def test_one_seed_one_result_whatever_the_split(ctxs, scene_a_1024):
    sc, pairs, _ = scene_a_1024
    ctx = ctxs[4]
    sub = pairs[np.arange(600) * 11 % 2415]
    rc1, one = _raw(ctx, sc, sub)
    rc2, two = _raw(ctx, sc, sub)
    assert rc1 == 0 and rc2 == 0 and pref.same_counts(one, two)
    rc3, other = _raw(ctx, dict(sc, seed=sc["seed"] + 1), sub)
    assert rc3 == 0 and not np.array_equal(other["within"], one["within"]) and np.array_equal(other["status"], one["status"])
    # a pair alone is cut into 4 chunks of 256 particles, among 599 others into 2 of 512: the same counts
    j = int(np.flatnonzero((one["ever"] > 0) & (one["ever"] < sc["S"]))[3])
    assert ref.chunks(1, sc["S"]) == (4, 256) and ref.chunks(600, sc["S"]) == (2, 512)
    rc4, solo = _raw(ctx, sc, sub[j:j + 1])
    assert rc4 == 0 and all(np.array_equal(solo[k][..., 0], one[k][..., j]) for k in pref.COUNTS) and solo["within"].any()


def test_the_seam_refuses_and_writes_nothing(ctxs):
    from pymht_amd import _lib
    a = ref.scene_a()
    sc = ref.scene(a["x"][:6], a["P"][:6], [0, 2, 3, 6], np.ones(6), a["Phi"], a["Q"], OWN0, S=128)
    good = [[0, 1], [2, 1], [0, 2]]
    for lib_nx in (4, 6):
        ctx = ctxs[lib_nx]
        rc, out = _raw(ctx, sc, good)
        assert rc == 0 and not pref.untouched(out)
        cases = [dict(nulls=(k,)) for k in ("ctx", "Phi", "Q", "x", "P", "first", "cdf", "pairs", "within", "firstAt", "ever", "valid", "status", "work")]
        cases += [dict(short=1), dict(S=100), dict(S=32), dict(S=(1 << 20) + 64), dict(K=0), dict(K=65), dict(nPair=0), dict(nPair=(1 << 20) + 1), dict(nx=5),
                  dict(transition=1), dict(transition=2), dict(T=0), dict(T=7), dict(dt=0.0), dict(R=float("nan")), dict(first=[0, 3, 2, 6]),
                  dict(first=[0, 2, 2, 6]), dict(first=[1, 2, 3, 6]), dict(first=[0, 2, 3, 5])]
        for case in cases:
            rc, out = _raw(ctx, sc, good, **case)
            assert rc == _lib.MHT_E_INVALID and pref.untouched(out), (lib_nx, case, rc)
        for bad in ([[0, 1], [-1, 1], [0, 2]], [[0, 1], [2, 3], [0, 2]], [[0, 1], [2, 1], [1, 1]], [[3, 0], [2, 1], [0, 2]]):
            rc, out = _raw(ctx, sc, bad)
            assert rc == _lib.MHT_E_INVALID and pref.untouched(out), (lib_nx, bad, rc)
            assert b"pair" in ctx.lib.mht_last_error()
        indefinite = dict(sc, Q=np.diag([1.0, -1.0, 1.0, 1.0]))
        rc, out = _raw(ctx, indefinite, good)
        assert rc == _lib.MHT_E_INVALID and pref.untouched(out)
        assert b"positive semidefinite" in ctx.lib.mht_last_error()
        for bad in ((5, 6, 3, 2, 7, 128), (4, 0, 1, 2, 7, 128), (4, 6, 7, 2, 7, 128), (4, 6, 3, 0, 7, 128), (4, 6, 3, 2, 0, 128), (4, 6, 3, 2, 7, 100)):
            assert ctx.lib.mht_mc_pair_work_bytes(*bad) == 0, bad


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_tracker_hands_its_leaves_to_the_pair_engine(name):
    from pymht_amd import evaluation, models
    model = getattr(models, name)
    six = name == "ct"
    trk = _scans(model, six)
    try:
        lb = trk.leafBatch()
        T = trk.nTargets
        assert T == 3 and len(lb["x"]) > T, "the scene keeps no second hypothesis"
        kw = dict(particles=1024, seed=5, steps=12)
        radius = 400.0      # (the three targets start 300 m apart at least: a radius at which pairs do meet)
        got = trk.getMonteCarloPairEncounters(60.0, radius, **kw)
        widen = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64)
        Phi, Q = (widen(model.Phi(5.0, 0.0)), widen(model.Q(5.0))) if six else eref.model_matrices(model, 5.0)
        P = np.asarray(lb["P"], dtype=np.float64)
        flat = dict(particles=1024, seed=5, transition="ct" if six else "linear", ctx=trk._ctx)
        every = pref.all_pairs(T).astype(np.int64)
        w = _weights(lb["cnllr"], lb["target"])
        want = evaluation.mc_pair_encounters(lb["x"], P, lb["target"], w, Phi, Q, 12, 5.0, radius, every, **flat)
        names = ("within", "firstAt", "ever", "valid", "status", "pc", "pcMax", "tpc", "pEver", "sePcMax", "sePEver", "pEverBy", "pairs", "cdf", "first")
        for k in names:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), k
        assert (got["status"] == 0).all() and (got["valid"] == 1024).all() and got["within"].shape == (13, 3) and got["firstAt"].shape == (13, 3)
        assert got["ever"].any() and np.array_equal(got["pEverBy"][-1], got["pEver"]) and (got["firstAt"].sum(axis=0) == got["ever"]).all()
        ids = [int(i) for i in trk._tbl_["id"]]
        assert got["ids"].tolist() == [[ids[a], ids[b]] for a, b in every] and np.array_equal(got["leafIds"], lb["ID"])
        order = sorted(range(3), key=lambda j: (-got["pEver"][j], j))
        assert got["ranking"].tolist() == order and got["worst"] == order[0]
        # the selected leaves alone
        sel = trk._selected_leaves(lb, list(trk.getTrackNodes()))
        assert (sel >= 0).all()
        best = trk.getMonteCarloPairEncounters(60.0, radius, hypotheses=False, **kw)
        only = evaluation.mc_pair_encounters(lb["x"][sel], P[sel], lb["target"][sel], np.ones(len(sel)), Phi, Q, 12, 5.0, radius, every, **flat)
        assert all(np.array_equal(best[k], only[k]) for k in pref.COUNTS) and np.array_equal(best["leafIds"], lb["ID"][sel])
        # a screen: a subset, with the same figures for the pairs it keeps
        cuts = [c for c in np.linspace(10.0, 3000.0, 300) if 1 <= len(evaluation.mc_pair_screen(lb["x"], lb["target"], w, 60.0, float(c))) < 3]
        assert cuts, "no distance keeps one or two of the three pairs"
        cut = float(cuts[0])
        part = trk.getMonteCarloPairEncounters(60.0, radius, screen=cut, **kw)
        kept = [every.tolist().index(p) for p in part["pairs"].tolist()]
        assert 1 <= len(kept) < 3 and np.array_equal(part["pairs"], evaluation.mc_pair_screen(lb["x"], lb["target"], w, 60.0, cut))
        for k in names[:12]:
            assert np.array_equal(part[k], got[k][..., kept], equal_nan=True), k
        given = trk.getMonteCarloPairEncounters(60.0, radius, pairs=[[2, 0], [0, 2]], **kw)
        assert all(np.array_equal(given[k][..., 0], got[k][..., 1]) and np.array_equal(given[k][..., 1], got[k][..., 1]) for k in pref.COUNTS)
        assert given["ranking"].tolist() == [0, 1] and given["ids"].tolist() == [[ids[2], ids[0]], [ids[0], ids[2]]]
        with pytest.raises(ValueError, match="getMonteCarloPairEncounters"):
            trk.getMonteCarloPairEncounters(60.0, radius, pairs=[[0, 3]], **kw)
        if six:      # the constant-turn tracker answers here, and the Gaussian rule still refuses it
            with pytest.raises(NotImplementedError):
                trk.getEncounters(60, 60)
        else:
            gh = trk.getGlobalHypotheses(k=8)
            joint = trk.getMonteCarloPairEncounters(60.0, radius, weights=gh["leafProbability"], **kw)
            assert (joint["status"] == 0).all() and joint["within"].shape == got["within"].shape
    finally:
        trk.close()
