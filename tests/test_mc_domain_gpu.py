"""GPU: the domain engine on the device (`mht_mc_domain_encounters`, include/mht_amd.h; csrc/mht_mc_domain.hip) against its host twin
(tests/hostmath/mc_domain_host.cpp, the same header compiled for the CPU) under the borderline rule of tests/mc_zone_ref.py -- the
generator is integer only, so only the device's sin, cos and log can move a particle, and only a borderline one across an edge;
tests/test_mc_domain_cpu.py asserts that the scenes here have none, so the counts are expected to be EQUAL and every test prints how
many cells differed --, the identity with `mht_mc_zone_encounters` under the pose (0, 0, 0, 1), the seam's refusals, and the drop-in
path Tracker.getMonteCarloDomainEncounters on a models/pv and a models/ct tracker.  The outputs are preset to a sentinel.  Nothing here
is larger than 70 targets of 1 024 particles against two domains on six paths, except one target with 65 536 particles, 1 030 targets
with 128, and 64 cells at 256 particles."""
import numpy as np
import pytest

import encounter_ref as eref
import mc_domain_ref as dref
import mc_ref as ref
import mc_zone_ref as zref
from test_encounter_gpu import GUARD_BYTE, guard_untouched, guarded_work
from test_mc_domain_cpu import check_shape
from test_mc_gpu import _scans, _weights

pytestmark = pytest.mark.gpu
GUARD = 256      # bytes behind the work buffer that no call may touch
assert GUARD_BYTE == 0xA5      # (the tests below look for the pattern by its value)


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
    return dref.build_twin(tmp_path_factory.mktemp("mc_domain_twin"))


def _raw(ctx, sc, domains, poses, nulls=(), short=0, packed=None, guard=GUARD, **over):
    """One call of the seam on a scene of tests/mc_ref.py, a list of domains (or packed = (domFirst, domXY) as they are) and poses, the
    outputs preset to a sentinel and the work buffer, with `guard` bytes behind it that must be the pattern after the call, to 0xA5:
    (return code, outputs, the buffer after the call as bytes)"""
    import torch
    dev = ctx.device
    df, dxy = packed if packed is not None else dref.pack(domains)
    df, dxy = np.ascontiguousarray(df, dtype=np.int32), np.ascontiguousarray(dxy, dtype=np.float64)
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    N, T, D, G = sc["x"].shape[1], len(sc["first"]) - 1, len(df) - 1, len(poses)
    xp, Pp = eref.pack(sc["x"], sc["P"])
    host = dict(Phi=np.ascontiguousarray(sc["Phi"]), Q=np.ascontiguousarray(sc["Q"]))
    first = np.ascontiguousarray(over.pop("first", sc["first"]), dtype=np.int32)
    arrays = dict(x=torch.from_numpy(xp).to(dev), P=torch.from_numpy(Pp).to(dev), first=torch.from_numpy(first).to(dev), cdf=torch.from_numpy(sc["cdf"]).to(dev),
                  ownPose=torch.from_numpy(poses).to(dev), domFirst=torch.from_numpy(df).to(dev), domXY=torch.from_numpy(dxy).to(dev))
    o = dref.outputs(D, G, sc["K"], T)
    for k in dref.COUNTS:
        arrays[k] = torch.from_numpy(o[k].view(np.int32)).to(dev)
    a = dict(nx=N, transition=1 if sc["ct"] else 0, nComp=len(sc["x"]), T=T, G=G, nDomain=D, nVert=len(dxy), K=sc["K"], S=sc["S"], seed=sc["seed"], dt=sc["dt"])
    a.update(over)
    need = int(ctx.lib.mht_mc_domain_work_bytes(N, len(sc["x"]), T, G, D, sc["K"], sc["S"]))
    assert need > 0 and need == dref.work_bytes(N, len(sc["x"]), T, G, D, sc["K"], sc["S"])
    arrays["work"] = guarded_work(need, guard, dev)
    ptr = lambda k: None if k in nulls else host[k].ctypes.data if k in host else arrays[k].data_ptr()
    torch.cuda.synchronize(dev)
    rc = ctx.lib.mht_mc_domain_encounters(None if "ctx" in nulls else ctx.handle, a["nx"], a["transition"], a["nComp"], a["T"], a["G"], a["nDomain"], a["nVert"], a["K"],
                                          a["S"], a["seed"], a["dt"], ptr("Phi"), ptr("Q"), ptr("x"), ptr("P"), ptr("first"), ptr("cdf"), ptr("ownPose"),
                                          ptr("domFirst"), ptr("domXY"), ptr("inside"), ptr("firstAt"), ptr("ever"), ptr("valid"), ptr("status"), ptr("work"),
                                          need - short)
    torch.cuda.synchronize(dev)
    assert guard_untouched(arrays["work"], need), "the call wrote behind the work buffer the sizer asks for"
    return rc, {k: arrays[k].cpu().numpy().view(o[k].dtype) for k in dref.COUNTS}, arrays["work"].cpu().numpy()


def _hold(label, got, want, sc, domains, poses):
    """The device's counts against the twin's: equal, or -- a last-bit difference of sin, cos or log -- within the reference's
    borderline particles per cell.  Prints the cells that differ and returns their number."""
    assert not any((got[k] == dref.SENTINEL).any() for k in ("inside", "firstAt", "ever", "valid")) and not (got["status"] == -7).any(), (label, "a sentinel is left")
    differ = 0
    if not dref.same_counts(got, want):
        border = dref.encounters(sc, domains, poses)
        differ = dref.hold_counts(label, got, dict(border, **{k: want[k] for k in dref.COUNTS}))
    print("%s: %d cells differ from the twin's" % (label, differ))
    dref.check_invariants(got)
    return differ


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_scene_d_equals_the_twin_on_both_builds(ctxs, twin, name):
    sc, doms, poses = dref.scene_d(ct=name == "ct")
    assert ref.chunks(70, sc["S"]) == (4, 256) and poses.shape == (6, 8, 4)
    want = dref.call_twin(twin, sc, doms, poses)
    for lib_nx in (4, 6):
        rc, got, work = _raw(ctxs[lib_nx], sc, doms, poses)
        assert rc == 0 and (work[-GUARD:] == 0xA5).all()
        assert _hold("scene D, %s, %d-state build" % (name, lib_nx), got, want, sc, doms, poses) == 0
    S, nan = sc["S"], [eref.NAN_X, eref.NAN_P]
    assert want["status"][nan].tolist() == [1, 1] and want["valid"][nan].tolist() == [0, 0] and int((want["status"] == 0).sum()) == 68
    partly = ((want["ever"] > 0) & (want["ever"] < S)).sum(axis=2)
    assert (partly[0] >= 25).all() and (partly[1] >= 34).all() and ((want["firstAt"][:, :, 1:] > 0).sum(axis=(2, 3)) >= 72).all()
    flat = want["ever"].reshape(12, 70)
    assert all(not np.array_equal(flat[i], flat[j]) for i in range(12) for j in range(i))      # a transposed or mis-strided store cannot pass


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_the_identity_pose_is_the_zone_seam_cell_for_cell(ctxs, name):
    """G = 1 and the pose (0, 0, 0, 1): the transform is exact, so the walk computes the zone walk's predicates on the zone walk's
    numbers -- on the same context, the two seams' counts are equal."""
    from test_mc_zone_gpu import _raw as zone_raw
    sc, zones = zref.scene_z(ct=name == "ct")
    for lib_nx in (4, 6):
        rc, want = zone_raw(ctxs[lib_nx], sc, zones)
        assert rc == 0
        for lo in (0, 2):
            rc, got, _ = _raw(ctxs[lib_nx], sc, zones[lo:lo + 4], dref.fixed_poses(dref.IDENTITY, sc["K"]))
            assert rc == 0
            for k in ("inside", "firstAt", "ever"):
                assert np.array_equal(got[k][:, 0], want[k][lo:lo + 4]), (lib_nx, lo, k, np.argwhere(got[k][:, 0] != want[k][lo:lo + 4])[:8].tolist())
            assert np.array_equal(got["valid"], want["valid"]) and np.array_equal(got["status"], want["status"])
    assert want["ever"][[0, 1, 2, 5]].any(axis=1).all()


@pytest.mark.parametrize("kind", dref.KINDS)
def test_shapes_at_which_the_kernel_takes_another_path(ctxs, twin, kind):
    sc, doms, poses = dref.shape_scene(kind)
    want = dref.call_twin(twin, sc, doms, poses)
    check_shape(kind, sc, doms, poses, want)
    for lib_nx in (4, 6):
        rc, got, work = _raw(ctxs[lib_nx], sc, doms, poses)
        assert rc == 0 and (work[-GUARD:] == 0xA5).all(), kind
        assert _hold("%s, %d-state build" % (kind, lib_nx), got, want, sc, doms, poses) == 0
        check_shape(kind, sc, doms, poses, got)


def test_one_seed_one_result_whatever_the_split(ctxs):
    sc, doms, poses = dref.scene_d()
    ctx = ctxs[4]
    rc1, one, _ = _raw(ctx, sc, doms, poses)
    rc2, two, _ = _raw(ctx, sc, doms, poses)
    assert rc1 == 0 and rc2 == 0 and dref.same_counts(one, two)
    rc3, other, _ = _raw(ctx, dict(sc, seed=sc["seed"] + 1), doms, poses)
    assert rc3 == 0 and not np.array_equal(other["inside"], one["inside"]) and np.array_equal(other["status"], one["status"])
    # targets 0 .. 2 alone are cut into 4 chunks of 256 particles as among the 70: the split is not in a count; nor are the other cells
    sub = ref.scene(sc["x"][:3], sc["P"][:3], np.arange(4), np.ones(3), sc["Phi"], sc["Q"], sc["own"], S=sc["S"])
    rc4, few, _ = _raw(ctx, sub, doms[1:], poses[1:4])
    assert rc4 == 0 and all(np.array_equal(few[k], one[k][1:, 1:4, ..., :3]) for k in ("inside", "firstAt", "ever")) and few["inside"].any()


def test_the_seam_refuses_and_writes_nothing(ctxs):
    from pymht_amd import _lib
    a = ref.scene_a()
    sc = ref.scene(a["x"][:6], a["P"][:6], [0, 2, 3, 6], np.ones(6), a["Phi"], a["Q"], a["own"], S=128)
    doms = dref.DOMAINS + [dref.ROUND[:6]]
    poses = dref.poses_of(a["x"][0, :4], dref.CANDIDATES[:3], sc["K"], sc["dt"])
    df, dxy = dref.pack(doms)
    assert df.tolist() == [0, 5, 11, 17]
    bad_xy = dxy.copy()
    bad_xy[9, 0] = np.nan
    long, nan, inf, zero = poses.copy(), poses.copy(), poses.copy(), poses.copy()
    long[1, 3, 2:] *= 1.001
    nan[2, 7, 0] = np.nan
    inf[0, 0, 3] = np.inf
    zero[2, 5, 2:] = 0.0
    for lib_nx in (4, 6):
        ctx = ctxs[lib_nx]
        rc, out, work = _raw(ctx, sc, doms, poses)
        assert rc == 0 and not dref.untouched(out) and (work[-GUARD:] == 0xA5).all() and not (work[:-GUARD] == 0xA5).all()
        cases = [dict(nulls=(k,)) for k in ("ctx", "Phi", "Q", "x", "P", "first", "cdf", "ownPose", "domFirst", "domXY", "inside", "firstAt", "ever", "valid", "status",
                                            "work")]
        cases += [dict(short=1), dict(S=100), dict(S=32), dict(S=(1 << 20) + 64), dict(K=0), dict(K=65), dict(G=0), dict(G=-1), dict(G=22), dict(G=65), dict(nDomain=0),
                  dict(nDomain=5), dict(nDomain=-1), dict(nVert=8), dict(nVert=16), dict(nVert=18), dict(nVert=257), dict(nVert=0), dict(nx=5), dict(transition=1),
                  dict(transition=2), dict(T=0), dict(T=7), dict(dt=0.0), dict(dt=float("nan")), dict(first=[0, 3, 2, 6]), dict(first=[0, 2, 2, 6]),
                  dict(first=[1, 2, 3, 6]), dict(first=[0, 2, 3, 5]), dict(packed=([0, 5, 7, 17], dxy)), dict(packed=([1, 5, 11, 17], dxy)),
                  dict(packed=([0, 11, 5, 17], dxy)), dict(packed=([0, 5, 11, 16], dxy)), dict(packed=(df, bad_xy)),
                  dict(packed=(df, np.where(np.isnan(bad_xy), np.inf, bad_xy)))]
        for case in cases:
            rc, out, work = _raw(ctx, sc, doms, poses, **case)
            assert rc == _lib.MHT_E_INVALID and dref.untouched(out) and (work == 0xA5).all(), (lib_nx, case, rc)
        for label, p in (("a heading of norm 1.001", long), ("a NaN position", nan), ("an infinite heading", inf), ("a heading of norm 0", zero)):
            rc, out, work = _raw(ctx, sc, doms, p)
            assert rc == _lib.MHT_E_INVALID and dref.untouched(out) and (work == 0xA5).all(), (lib_nx, label, rc)
            assert b"mht_mc_domain_encounters" in ctx.lib.mht_last_error()
        rc, out, _ = _raw(ctx, sc, doms, long)
        assert rc == _lib.MHT_E_INVALID and b"unit vector" in ctx.lib.mht_last_error()
        # nCell = 65 as 1 x 65 (3 x 22 = 66 and 3 x 65 are above; 64 cells are taken: the shapes)
        rc, out, work = _raw(ctx, sc, doms[:1], poses, G=65)
        assert rc == _lib.MHT_E_INVALID and dref.untouched(out) and (work == 0xA5).all() and b"cells" in ctx.lib.mht_last_error()
        rc, out, _ = _raw(ctx, sc, doms, poses, packed=(df, bad_xy))
        assert rc == _lib.MHT_E_INVALID and b"finite" in ctx.lib.mht_last_error()
        indefinite = dict(sc, Q=np.diag([1.0, -1.0, 1.0, 1.0]))
        rc, out, work = _raw(ctx, indefinite, doms, poses)
        assert rc == _lib.MHT_E_INVALID and dref.untouched(out) and (work == 0xA5).all()
        assert b"positive semidefinite" in ctx.lib.mht_last_error()


BOW_UP = [np.array([(-60, -80), (90, -80), (110, 120), (20, 330), (-70, 120)], dtype=np.float64),
          np.array([(-220, -200), (330, -200), (380, 300), (60, 820), (-260, 300)], dtype=np.float64)]


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_tracker_hands_its_leaves_to_the_domain_engine(name):
    from pymht_amd import evaluation, models
    from pymht_amd.tracker import Tracker
    model = getattr(models, name)
    six = name == "ct"
    trk = _scans(model, six)
    try:
        lb = trk.leafBatch()
        T = trk.nTargets
        assert T == 3 and len(lb["x"]) > T, "the scene keeps no second hypothesis"
        own = np.array([lb["x"][0, 0] - 300.0, lb["x"][0, 1] + 40.0, 8.0, 0.0])
        deg = np.pi / 180.0
        kw = dict(particles=1024, seed=5, courseChanges=[0.0, 40.0 * deg, -40.0 * deg], turnRate=0.05, speedFactors=[1.0, 0.5], steps=12)
        got = trk.getMonteCarloDomainEncounters(60.0, BOW_UP, own, **kw)
        widen = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64)
        Phi, Q = (widen(model.Phi(5.0, 0.0)), widen(model.Q(5.0))) if six else eref.model_matrices(model, 5.0)
        P = np.asarray(lb["P"], dtype=np.float64)
        assert got["candidates"].shape == (6, 3) and got["candidates"][:, 0].tolist() == [0.0, 0.0, 40.0 * deg, 40.0 * deg, -40.0 * deg, -40.0 * deg]
        poses = evaluation.mc_own_poses(own, got["candidates"], 0.05, 12, 5.0)
        flat = dict(particles=1024, seed=5, transition="ct" if six else "linear", ctx=trk._ctx)
        w = _weights(lb["cnllr"], lb["target"])
        want = evaluation.mc_domain_encounters(lb["x"], P, lb["target"], w, Phi, Q, 12, 5.0, BOW_UP, poses, **flat)
        names = dref.COUNTS + ("pInside", "pInsideMax", "tInside", "pEver", "pEverBy", "sePInsideMax", "sePEver", "domFirst", "domXY", "ownPoses", "targets", "cdf",
                               "first", "order")
        for k in names:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), k
        assert (got["status"] == 0).all() and (got["valid"] == 1024).all() and got["inside"].shape == (2, 6, 13, 3) and got["ever"].shape == (2, 6, 3)
        assert got["ever"].any() and ((got["ever"] > 0) & (got["ever"] < 1024)).any() and np.array_equal(got["pEverBy"][:, :, -1], got["pEver"])
        assert (got["firstAt"].sum(axis=2) == got["ever"]).all() and (got["ever"] >= got["inside"].max(axis=2)).all()
        # the identity pose: the zone engine's figures on the same leaves
        still = evaluation.mc_domain_encounters(lb["x"], P, lb["target"], w, Phi, Q, 12, 5.0, BOW_UP, dref.fixed_poses(dref.IDENTITY, 12), **flat)
        zone = evaluation.mc_zone_encounters(lb["x"], P, lb["target"], w, Phi, Q, 12, 5.0, BOW_UP, **flat)
        assert all(np.array_equal(still[k][:, 0], zone[k]) for k in ("inside", "firstAt", "ever"))
        ids = [int(i) for i in trk._tbl_["id"]]
        assert list(got["ids"]) == ids[:3] and np.array_equal(got["leafIds"], lb["ID"])
        # pEverMax, its target and best: domain 0 decides, the lowest index among equals
        assert got["pEverMax"].shape == (2, 6) and got["pEverMaxTarget"].shape == (2, 6) and got["pEverMaxTarget"].dtype == np.int64
        assert np.array_equal(got["pEverMax"], got["pEver"].max(axis=2)) and np.array_equal(got["pEverMaxTarget"], got["pEver"].argmax(axis=2))
        assert got["best"] == int(np.argmin(got["pEverMax"][0])) and (got["pEverMax"][1] >= got["pEverMax"][0]).all()
        swapped = trk.getMonteCarloDomainEncounters(60.0, BOW_UP[::-1], own, **kw)
        assert np.array_equal(swapped["ever"], got["ever"][::-1]) and swapped["best"] == int(np.argmin(got["pEverMax"][1]))
        # a repeated seed gives the same bits, another seed another draw
        again = trk.getMonteCarloDomainEncounters(60.0, BOW_UP, own, **kw)
        assert all(np.array_equal(again[k], got[k]) for k in dref.COUNTS)
        other = trk.getMonteCarloDomainEncounters(60.0, BOW_UP, own, **dict(kw, seed=6))
        assert not np.array_equal(other["inside"], got["inside"])
        # the selected leaves alone
        sel = trk._selected_leaves(lb, list(trk.getTrackNodes()))
        assert (sel >= 0).all()
        best = trk.getMonteCarloDomainEncounters(60.0, BOW_UP, own, hypotheses=False, **kw)
        only = evaluation.mc_domain_encounters(lb["x"][sel], P[sel], lb["target"][sel], np.ones(len(sel)), Phi, Q, 12, 5.0, BOW_UP, poses, **flat)
        assert all(np.array_equal(best[k], only[k]) for k in dref.COUNTS) and np.array_equal(best["leafIds"], lb["ID"][sel])
        bad = [dict(domains=[BOW_UP[0][:2]]), dict(domains=[BOW_UP[0]] * 5), dict(domains=[]), dict(horizon=-1.0), dict(particles=100), dict(ownShip=[0.0, 0.0, 0.0, 0.0]),
               dict(ownShip=[0.0, 0.0, 1.0]), dict(delay=-1.0), dict(courseChanges=[0.1], turnRate=None), dict(courseChanges=np.linspace(-1, 1, 11), speedFactors=[1.0] * 3),
               dict(courseChanges=np.linspace(-1, 1, 65))]
        for change in bad:
            with pytest.raises(ValueError, match="getMonteCarloDomainEncounters"):
                trk.getMonteCarloDomainEncounters(**dict(dict(horizon=60.0, domains=BOW_UP, ownShip=own, **kw), **change))
        with pytest.raises(ValueError, match="64 cells"):
            trk.getMonteCarloDomainEncounters(60.0, BOW_UP, own, **dict(kw, courseChanges=np.linspace(-1, 1, 11), speedFactors=[1.0, 0.9, 0.8]))
        if six:      # the constant-turn tracker answers here, and the Gaussian rule still refuses it
            with pytest.raises(NotImplementedError):
                trk.getEncounters(60, 60)
        else:
            gh = trk.getGlobalHypotheses(k=8)
            joint = trk.getMonteCarloDomainEncounters(60.0, BOW_UP, own, weights=gh["leafProbability"], **kw)
            assert (joint["status"] == 0).all() and joint["inside"].shape == got["inside"].shape
    finally:
        trk.close()
    # no live target: empty arrays, no figure, no best
    idle = Tracker(model, 2.5, 2e-5, 1e-4, P_d=0.7, N=3, eta2=5.99, useInitiator=False)
    try:
        none = idle.getMonteCarloDomainEncounters(60.0, BOW_UP, own, **kw)
        assert none["inside"].shape == (2, 6, 13, 0) and none["ever"].shape == (2, 6, 0) and none["valid"].shape == (0,)
        assert list(none["ids"]) == [] and len(none["leafIds"]) == 0 and none["best"] is None and np.isnan(none["pEverMax"]).all() and (none["pEverMaxTarget"] == -1).all()
    finally:
        idle.close()
