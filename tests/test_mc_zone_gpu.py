"""GPU: the zone engine on the device (`mht_mc_zone_encounters`, include/mht_amd.h; csrc/mht_mc_zone.hip) against its host twin
(tests/hostmath/mc_zone_host.cpp, the same header compiled for the CPU) under the borderline rule of tests/mc_zone_ref.py -- the
generator is integer only, so only the device's sin, cos and log can move a particle, and only a borderline one across an edge; the
scenes have none, so the counts are expected to be EQUAL and every test prints how many cells differed --, the seam's refusals, and the
drop-in path Tracker.getMonteCarloZoneEncounters on a models/pv and a models/ct tracker.  The outputs are preset to a sentinel.  Nothing
here is larger than 70 targets of 1 024 particles against six zones, except one target with 65 536 particles and 1 030 targets with 128."""
import numpy as np
import pytest

import encounter_ref as eref
import mc_ref as ref
import mc_zone_ref as zref
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
    return zref.build_twin(tmp_path_factory.mktemp("mc_zone_twin"))


def _raw(ctx, sc, zones, nulls=(), short=0, packed=None, guard=0, **over):
    """One call of the seam on a scene of tests/mc_ref.py and a list of zones (or packed = (zoneFirst, zoneXY) as they are), the outputs
    preset to a sentinel and the work buffer to a pattern: (return code, outputs).  guard > 0: that many bytes of the pattern lie behind
    the sizer's figure and must be the pattern after the call."""
    import torch
    dev = ctx.device
    zf, zxy = packed if packed is not None else zref.pack(zones)
    zf, zxy = np.ascontiguousarray(zf, dtype=np.int32), np.ascontiguousarray(zxy, dtype=np.float64)
    N, T, Z = sc["x"].shape[1], len(sc["first"]) - 1, len(zf) - 1
    xp, Pp = eref.pack(sc["x"], sc["P"])
    host = dict(Phi=np.ascontiguousarray(sc["Phi"]), Q=np.ascontiguousarray(sc["Q"]))
    first = np.ascontiguousarray(over.pop("first", sc["first"]), dtype=np.int32)
    arrays = dict(x=torch.from_numpy(xp).to(dev), P=torch.from_numpy(Pp).to(dev), first=torch.from_numpy(first).to(dev), cdf=torch.from_numpy(sc["cdf"]).to(dev),
                  zoneFirst=torch.from_numpy(zf).to(dev), zoneXY=torch.from_numpy(zxy).to(dev))
    o = zref.outputs(Z, sc["K"], T)
    for k in zref.COUNTS:
        arrays[k] = torch.from_numpy(o[k].view(np.int32)).to(dev)
    a = dict(nx=N, transition=1 if sc["ct"] else 0, nComp=len(sc["x"]), T=T, nZone=Z, nVert=len(zxy), K=sc["K"], S=sc["S"], seed=sc["seed"], dt=sc["dt"])
    a.update(over)
    need = int(ctx.lib.mht_mc_zone_work_bytes(N, len(sc["x"]), T, Z, sc["K"], sc["S"]))
    assert need > 0 and need == zref.work_bytes(N, len(sc["x"]), T, Z, sc["K"], sc["S"])
    arrays["work"] = guarded_work(need, guard, dev)
    ptr = lambda k: None if k in nulls else host[k].ctypes.data if k in host else arrays[k].data_ptr()
    torch.cuda.synchronize(dev)
    rc = ctx.lib.mht_mc_zone_encounters(None if "ctx" in nulls else ctx.handle, a["nx"], a["transition"], a["nComp"], a["T"], a["nZone"], a["nVert"], a["K"], a["S"],
                                        a["seed"], a["dt"], ptr("Phi"), ptr("Q"), ptr("x"), ptr("P"), ptr("first"), ptr("cdf"), ptr("zoneFirst"), ptr("zoneXY"),
                                        ptr("inside"), ptr("firstAt"), ptr("ever"), ptr("valid"), ptr("status"), ptr("work"), need - short)
    torch.cuda.synchronize(dev)
    assert guard_untouched(arrays["work"], need), "the call wrote behind the work buffer the sizer asks for"
    return rc, {k: arrays[k].cpu().numpy().view(o[k].dtype) for k in zref.COUNTS}


def _hold(label, got, want, sc, zones):
    """The device's counts against the twin's: equal, or -- a last-bit difference of sin, cos or log -- within the reference's
    borderline particles per cell.  Prints the cells that differ and returns their number."""
    assert not any((got[k] == zref.SENTINEL).any() for k in ("inside", "firstAt", "ever", "valid")) and not (got["status"] == -7).any(), (label, "a sentinel is left")
    differ = 0
    if not zref.same_counts(got, want):
        border = zref.encounters(sc, zones)
        differ = zref.hold_counts(label, got, dict(border, **{k: want[k] for k in zref.COUNTS}))
    print("%s: %d cells differ from the twin's" % (label, differ))
    zref.check_invariants(got)
    return differ


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_scene_z_equals_the_twin_on_both_builds(ctxs, twin, name):
    sc, zones = zref.scene_z(ct=name == "ct")
    assert ref.chunks(70, sc["S"]) == (4, 256)
    want = zref.call_twin(twin, sc, zones)
    for lib_nx in (4, 6):
        rc, got = _raw(ctxs[lib_nx], sc, zones)
        assert rc == 0
        assert _hold("scene Z, %s, %d-state build" % (name, lib_nx), got, want, sc, zones) == 0
    S, nan = sc["S"], [eref.NAN_X, eref.NAN_P]
    assert want["status"][nan].tolist() == [1, 1] and want["valid"][nan].tolist() == [0, 0] and int((want["status"] == 0).sum()) == 68
    scored = want["status"] == 0
    assert (want["inside"][zref.CONTAINING][:, scored] == S).all() and not want["ever"][zref.FAR].any()
    for z in (0, 1, 2, 5):
        assert int(((want["ever"][z] > 0) & (want["ever"][z] < S)).sum()) >= 57 and int((want["firstAt"][z, 1:] > 0).sum()) >= 190
    assert int(want["ever"][2].sum()) > 10 * int(want["inside"][2].sum())      # the sliver: crossed between steps


def test_the_stride_scene(ctxs, twin):
    sc, zones = zref.scene_stride()
    want = zref.call_twin(twin, sc, zones)
    zref.check_stride_counts(want)
    for lib_nx in (4, 6):
        rc, got = _raw(ctxs[lib_nx], sc, zones)
        assert rc == 0
        assert _hold("stride scene, %d-state build" % lib_nx, got, want, sc, zones) == 0
        zref.check_stride_counts(got)


def zones_about(c):
    """Scene Z's four zones that are partly hit, about another centre"""
    c = np.asarray(c, dtype=np.float64)
    return [zref.reg(5, 400.0, c, 0.1), c + zref.U_SHAPE, c + np.array([0.0, 37.3]) + zref.SLIVER, zref.reg(64, 250.0, c + np.array([120.0, -80.0]), 0.1)[::-1].copy()]


KINDS = ["S=64", "S=320", "T=1, S=65536", "T=1030", "K=1", "K=64", "Z=1", "Z=32", "nVert=1024 in one zone", "67 components", "a NaN component next to a good target"]


def _shape_scene(kind):
    a, c = ref.scene_a(), ref.scene_c()
    za = zref.zones_z(a)
    if kind == "S=64":
        return dict(a, S=64), za
    if kind == "S=320":
        return dict(c, S=320), za
    if kind == "T=1, S=65536":
        return ref.scene(a["x"][12:13], a["P"][12:13], [0, 1], [1.0], a["Phi"], a["Q"], a["own"], S=65536), zones_about(a["x"][12, :2] + [150.0, 60.0])
    if kind == "T=1030":
        idx = np.arange(1030) % 70
        return ref.scene(c["x"][idx], c["P"][idx], np.arange(1031), np.ones(1030), c["Phi"], c["Q"], c["own"], ct=True, S=128), za
    if kind in ("K=1", "K=64"):
        K = int(kind[2:])
        return dict(c if K == 1 else a, K=K, dt=35.0 / K, S=512), za
    if kind == "Z=1":
        return dict(a, S=512), za[:1]
    if kind == "Z=32":
        ctr = zref.centre_of(a)
        many = [zref.reg(3 + z % 6, 120.0 + 15.0 * z, ctr + 60.0 * np.array([np.cos(z), np.sin(2.0 * z)]), 0.1 * z)[::1 - 2 * (z % 2)].copy() for z in range(30)]
        return dict(c, S=256), many + [za[2], za[1]]
    if kind.startswith("nVert"):
        return dict(a, S=256), [zref.reg(1024, 300.0, zref.centre_of(a), 0.05)]
    rng = np.random.default_rng(67)
    if kind == "67 components":
        n = 67
        x, P = np.tile(a["x"][12], (n + 2, 1)), np.tile(a["P"][12], (n + 2, 1, 1))
        x[:n, :2] += rng.uniform(-120, 120, (n, 2))
        x[n + 1, :2] += [60.0, -40.0]
        w = np.append(rng.uniform(0, 1, n), [1.0, 1.0])
        w[[5, 66]] = 0.0
        return ref.scene(x, P, [0, n, n + 1, n + 2], w, a["Phi"], a["Q"], a["own"], S=1024), zones_about(a["x"][12, :2] + [150.0, 60.0])
    assert kind.startswith("a NaN")
    x, P = np.tile(c["x"][12], (7, 1)), np.tile(c["P"][12], (7, 1, 1))
    x[:, :2] += rng.uniform(-60, 60, (7, 2))
    x[2, 3] = np.nan
    return ref.scene(x, P, [0, 2, 5, 7], np.ones(7), c["Phi"], c["Q"], c["own"], ct=True, S=512), zones_about(c["x"][12, :2] + [150.0, 60.0])


@pytest.mark.parametrize("kind", KINDS)
def test_shapes_at_which_the_kernel_takes_another_path(ctxs, twin, kind):
    sc, zones = _shape_scene(kind)
    if sc["K"] != ref.K:      # (Phi and Q of the scene's own step)
        from pymht_amd.models import ct, pv
        if sc["ct"]:
            sc = dict(sc, Q=np.asarray(ct.Q(sc["dt"]), dtype=np.float32).astype(np.float64))
        else:
            Phi, Q = eref.model_matrices(pv, sc["dt"])
            sc = dict(sc, Phi=Phi, Q=Q)
    want = zref.call_twin(twin, sc, zones)
    for lib_nx in (4, 6):
        rc, got = _raw(ctxs[lib_nx], sc, zones)
        assert rc == 0, kind
        assert _hold("%s, %d-state build" % (kind, lib_nx), got, want, sc, zones) == 0
    S = sc["S"]
    assert want["inside"].any() and want["firstAt"][:, 1:].any() and ((want["ever"] > 0) & (want["ever"] < S)).any()
    if kind == "S=320":
        assert ref.chunks(70, 320) == (2, 256)      # a last chunk of 64: three wavefronts of it walk along and count nowhere
    if kind == "T=1, S=65536":
        assert ref.chunks(1, 65536) == (256, 256)
    if kind == "T=1030":
        assert ref.chunks(1030, 128) == (1, 256) and want["ever"].shape == (6, 1030)
        assert not np.array_equal(want["ever"][:, 0], want["ever"][:, 70])      # (the stream is keyed by the target: a copy is another draw)
    if kind == "K=64":
        assert want["inside"].shape == (6, 65, 70) and want["inside"][:, 64].any() and want["firstAt"][:, 33:].any()
    if kind == "Z=32":
        assert want["ever"].shape == (32, 70) and all(((want["ever"][z] > 0) & (want["ever"][z] < S)).any() for z in range(32))
    if kind.startswith("nVert"):
        assert zref.pack(zones)[0].tolist() == [0, 1024]
    if kind.startswith("a NaN"):
        assert want["status"].tolist() == [0, 1, 0] and want["valid"].tolist() == [512, 0, 512] and not want["inside"][:, :, 1].any()


def test_one_seed_one_result_whatever_the_split(ctxs, twin):
    sc, zones = zref.scene_z()
    ctx = ctxs[4]
    rc1, one = _raw(ctx, sc, zones)
    rc2, two = _raw(ctx, sc, zones)
    assert rc1 == 0 and rc2 == 0 and zref.same_counts(one, two)
    rc3, other = _raw(ctx, dict(sc, seed=sc["seed"] + 1), zones)
    assert rc3 == 0 and not np.array_equal(other["inside"], one["inside"]) and np.array_equal(other["status"], one["status"])
    # targets 0 .. 2 alone are cut into 4 chunks of 256 particles as among the 70; 1 030 copies would get one chunk: the split is not in a count
    sub = ref.scene(sc["x"][:3], sc["P"][:3], np.arange(4), np.ones(3), sc["Phi"], sc["Q"], sc["own"], S=sc["S"])
    rc4, few = _raw(ctx, sub, zones)
    assert rc4 == 0 and all(np.array_equal(few[k], one[k][..., :3]) for k in zref.COUNTS) and few["inside"][:3].any()


def test_the_seam_refuses_and_writes_nothing(ctxs):
    from pymht_amd import _lib
    a = ref.scene_a()
    sc = ref.scene(a["x"][:6], a["P"][:6], [0, 2, 3, 6], np.ones(6), a["Phi"], a["Q"], a["own"], S=128)
    zones = zones_about(a["x"][0, :2])[:3]
    zf, zxy = zref.pack(zones)
    assert zf.tolist() == [0, 5, 13, 17]
    bad_xy = zxy.copy()
    bad_xy[9, 0] = np.nan
    for lib_nx in (4, 6):
        ctx = ctxs[lib_nx]
        rc, out = _raw(ctx, sc, zones)
        assert rc == 0 and not zref.untouched(out)
        cases = [dict(nulls=(k,)) for k in ("ctx", "Phi", "Q", "x", "P", "first", "cdf", "zoneFirst", "zoneXY", "inside", "firstAt", "ever", "valid", "status", "work")]
        cases += [dict(short=1), dict(S=100), dict(S=32), dict(S=(1 << 20) + 64), dict(K=0), dict(K=65), dict(nZone=0), dict(nZone=33), dict(nZone=-1), dict(nVert=8),
                  dict(nVert=16), dict(nVert=18), dict(nVert=1025), dict(nVert=0), dict(nx=5), dict(transition=1), dict(transition=2), dict(T=0), dict(T=7),
                  dict(dt=0.0), dict(dt=float("nan")), dict(first=[0, 3, 2, 6]), dict(first=[0, 2, 2, 6]), dict(first=[1, 2, 3, 6]), dict(first=[0, 2, 3, 5]),
                  dict(packed=([0, 5, 7, 17], zxy)), dict(packed=([1, 5, 13, 17], zxy)), dict(packed=([0, 13, 5, 17], zxy)), dict(packed=([0, 5, 13, 16], zxy)),
                  dict(packed=(zf, bad_xy)), dict(packed=(zf, np.where(np.isnan(bad_xy), np.inf, bad_xy)))]
        for case in cases:
            rc, out = _raw(ctx, sc, zones, **case)
            assert rc == _lib.MHT_E_INVALID and zref.untouched(out), (lib_nx, case, rc)
        rc, out = _raw(ctx, sc, zones, packed=(zf, bad_xy))
        assert rc == _lib.MHT_E_INVALID and b"finite" in ctx.lib.mht_last_error() and b"mht_mc_zone_encounters" in ctx.lib.mht_last_error()
        indefinite = dict(sc, Q=np.diag([1.0, -1.0, 1.0, 1.0]))
        rc, out = _raw(ctx, indefinite, zones)
        assert rc == _lib.MHT_E_INVALID and zref.untouched(out)
        assert b"positive semidefinite" in ctx.lib.mht_last_error()


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_tracker_hands_its_leaves_to_the_zone_engine(name):
    from pymht_amd import evaluation, models
    from pymht_amd.tracker import Tracker
    model = getattr(models, name)
    six = name == "ct"
    trk = _scans(model, six)
    try:
        lb = trk.leafBatch()
        T = trk.nTargets
        assert T == 3 and len(lb["x"]) > T, "the scene keeps no second hypothesis"
        zones = zones_about(np.median(lb["x"][:, :2], axis=0))
        kw = dict(particles=1024, seed=5, steps=12)
        got = trk.getMonteCarloZoneEncounters(60.0, zones, **kw)
        widen = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64)
        Phi, Q = (widen(model.Phi(5.0, 0.0)), widen(model.Q(5.0))) if six else eref.model_matrices(model, 5.0)
        P = np.asarray(lb["P"], dtype=np.float64)
        flat = dict(particles=1024, seed=5, transition="ct" if six else "linear", ctx=trk._ctx)
        w = _weights(lb["cnllr"], lb["target"])
        want = evaluation.mc_zone_encounters(lb["x"], P, lb["target"], w, Phi, Q, 12, 5.0, zones, **flat)
        names = zref.COUNTS + ("pInside", "pInsideMax", "tInside", "pEver", "pEverBy", "sePInsideMax", "sePEver", "zoneFirst", "zoneXY", "targets", "cdf", "first", "order")
        for k in names:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), k
        assert (got["status"] == 0).all() and (got["valid"] == 1024).all() and got["inside"].shape == (4, 13, 3) and got["firstAt"].shape == (4, 13, 3)
        assert got["ever"].any() and ((got["ever"] > 0) & (got["ever"] < 1024)).any() and np.array_equal(got["pEverBy"][:, -1], got["pEver"])
        assert (got["firstAt"].sum(axis=1) == got["ever"]).all() and (got["ever"] >= got["inside"].max(axis=1)).all()
        ids = [int(i) for i in trk._tbl_["id"]]
        assert list(got["ids"]) == ids[:3] and np.array_equal(got["leafIds"], lb["ID"])
        cells = sorted(((z, t) for z in range(4) for t in range(3)), key=lambda c: (-got["pEver"][c], c))
        assert got["ranking"].tolist() == [list(c) for c in cells] and got["ranking"].dtype == np.int64
        # the selected leaves alone
        sel = trk._selected_leaves(lb, list(trk.getTrackNodes()))
        assert (sel >= 0).all()
        best = trk.getMonteCarloZoneEncounters(60.0, zones, hypotheses=False, **kw)
        only = evaluation.mc_zone_encounters(lb["x"][sel], P[sel], lb["target"][sel], np.ones(len(sel)), Phi, Q, 12, 5.0, zones, **flat)
        assert all(np.array_equal(best[k], only[k]) for k in zref.COUNTS) and np.array_equal(best["leafIds"], lb["ID"][sel])
        # no zone: empty arrays
        none = trk.getMonteCarloZoneEncounters(60.0, [], **kw)
        assert none["inside"].shape == (0, 13, 0) and none["ever"].shape == (0, 0) and none["ranking"].shape == (0, 2) and list(none["ids"]) == []
        for bad in (dict(zones=[zones[0][:2]]), dict(zones=[zones[0]] * 33), dict(horizon=-1.0), dict(particles=100)):
            with pytest.raises(ValueError, match="getMonteCarloZoneEncounters"):
                trk.getMonteCarloZoneEncounters(**dict(dict(horizon=60.0, zones=zones, **kw), **bad))
        if six:      # the constant-turn tracker answers here, and the Gaussian rule still refuses it
            with pytest.raises(NotImplementedError):
                trk.getEncounters(60, 60)
        else:
            gh = trk.getGlobalHypotheses(k=8)
            joint = trk.getMonteCarloZoneEncounters(60.0, zones, weights=gh["leafProbability"], **kw)
            assert (joint["status"] == 0).all() and joint["inside"].shape == got["inside"].shape
    finally:
        trk.close()
    # no live target: empty arrays
    idle = Tracker(model, 2.5, 2e-5, 1e-4, P_d=0.7, N=3, eta2=5.99, useInitiator=False)
    try:
        none = idle.getMonteCarloZoneEncounters(60.0, zones, **kw)
        assert none["inside"].shape == (4, 13, 0) and none["ever"].shape == (4, 0) and none["valid"].shape == (0,) and none["ranking"].shape == (0, 2)
        assert list(none["ids"]) == [] and len(none["leafIds"]) == 0
    finally:
        idle.close()
