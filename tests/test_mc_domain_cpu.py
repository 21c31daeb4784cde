"""CPU: the domain engine's host twin (tests/hostmath/mc_domain_host.cpp, csrc/mht_mc_domain.h compiled for the CPU) against the NumPy
reference tests/mc_domain_ref.py, which is built on tests/mc_ref.py's own particles and takes tests/mc_zone_ref.py's geometry and
borderline rule; the identity with the zone engine under the pose (0, 0, 0, 1) and the three other quarter-turn headings; a disc
sandwiched between an inscribed and a circumscribed 64-gon against tests/mc_ref.py's disc; a bow-heavy domain that tells ahead from
astern and follows a turn; the scenes of tests/test_mc_domain_gpu.py, none of which has a borderline particle; and
pymht_amd.evaluation's host side (mc_own_poses, mc_domain_pack, mc_domain_derive, every ValueError) without a device.

SCENE D is mc_ref.scene_a() (70 models/pv targets, entries 5 and 9 NaN) or scene_c() (its constant-turn lift) at S = 1024, K = 7,
seed 12345, with two bow-up domains -- an inner pentagon with a pointed bow, 410 m long and 180 m wide, and an outer concave hexagon
1 020 m long -- carried along six own paths from entry 0's state: standing on, 40 degrees to port after 10 s, 40 degrees to starboard
at once, half speed, 20 degrees to port at 0.7 of the speed after 5 s, and 80 degrees to starboard after 5 s.  Read from the reference
when written: no borderline particle in either scene; per cell 26 to 34 targets (inner) and 36 to 54 (outer) are hit by some and not
all particles (pv), with 72 to 178 non-zero firstAt[k > 0] cells."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import encounter_ref as eref
import mc_domain_ref as dref
import mc_ref as ref
import mc_zone_ref as zref


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return dref.build_twin(tmp_path_factory.mktemp("mc_domain_twin"))


@pytest.fixture(scope="module")
def zone_twin(tmp_path_factory):
    return zref.build_twin(tmp_path_factory.mktemp("mc_domain_zone_twin"))


@pytest.fixture(scope="module")
def scenes(twin):
    """Scene D for models pv and ct: (scene, domains, poses, the twin's counts, the reference's), computed once (seconds)"""
    out = {}
    for name in ("pv", "ct"):
        sc, doms, poses = dref.scene_d(ct=name == "ct")
        out[name] = (sc, doms, poses, dref.call_twin(twin, sc, doms, poses), dref.encounters(sc, doms, poses, "c" if name == "ct" else "a"))
    return out


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_twin_equals_the_reference_on_scene_d(scenes, twin, name):
    sc, doms, poses, got, want = scenes[name]
    S, T = sc["S"], 70
    differ = dref.hold_counts("scene D, %s" % name, got, want)
    print("scene D, %s: %d borderline particles of %d walked, %d cells differ" % (name, want["border"], want["walked"], differ))
    assert want["border"] == 0 and not want["borderInside"].any() and differ == 0 and want["walked"] == 12 * 68 * S
    assert dref.same_counts(got, {k: want[k] for k in dref.COUNTS})
    assert not any((got[k] == dref.SENTINEL).any() for k in ("inside", "firstAt", "ever", "valid")) and got["inside"].shape == (2, 6, 8, T)
    dref.check_invariants(got)
    dref.check_invariants(want)
    nan = [eref.NAN_X, eref.NAN_P]
    assert got["status"][nan].tolist() == [1, 1] and got["valid"][nan].tolist() == [0, 0] and int((got["status"] == 0).sum()) == T - 2
    e = got["ever"]
    partly = ((e > 0) & (e < S)).sum(axis=2)
    assert (partly[0] >= 25).all() and (partly[1] >= 34).all() and ((got["firstAt"][:, :, 1:] > 0).sum(axis=(2, 3)) >= 72).all()
    # the paths differ, and so do the domains: no two cells with the same counts
    flat = e.reshape(12, T)
    assert all(not np.array_equal(flat[i], flat[j]) for i in range(12) for j in range(i))
    # entry 0 is where the own ship is: inside both domains at step 0 with (nearly) every particle, on every path
    assert (got["inside"][:, :, 0, 0] > 0.95 * S).all()
    # the skip moves no count
    assert dref.same_counts(got, dref.call_twin(twin, sc, doms, poses, skip=False))
    # a path's counts do not depend on the other paths of the call, nor a domain's on the other domains
    alone = dref.call_twin(twin, sc, doms[1:], poses[2:4])
    assert all(np.array_equal(alone[k], got[k][1:, 2:4]) for k in ("inside", "firstAt", "ever"))


def test_the_transform_on_hand_stated_cases(twin):
    body = lambda pose, x, y: dref.twin_body(twin, pose, x, y).tolist()
    # heading north (x east, y north): starboard is east, ahead is north
    assert body((10, 20, 0, 1), 13, 27) == [3.0, 7.0]
    # heading east: a point to the north is to port, one to the east ahead
    assert body((10, 20, 1, 0), 10, 25) == [-5.0, 0.0] and body((10, 20, 1, 0), 14, 20) == [0.0, 4.0]
    # heading south: east is to port; heading west: north is to starboard
    assert body((0, 0, 0, -1), 2, 0) == [-2.0, 0.0] and body((0, 0, -1, 0), 0, 3) == [3.0, 0.0]
    # 3-4-5: ahead along the heading, and the header's order of operations against NumPy's
    q = body((1, 1, 0.6, 0.8), 4, 5)      # (0.6 and 0.8 are not binary fractions: a rounding or two)
    assert abs(q[0]) < 1e-14 and abs(q[1] - 5.0) < 1e-14
    rng = np.random.default_rng(1)
    for _ in range(50):
        o, ang, p = rng.normal(0, 3e3, 2), rng.uniform(0, 7), rng.normal(0, 3e3, 2)
        pose = np.array([[o[0], o[1], np.sin(ang), np.cos(ang)]])
        qx, qy = dref.body(pose, np.array([[p[0]]]), np.array([[p[1]]]))
        assert body(pose[0], p[0], p[1]) == [qx[0, 0], qy[0, 0]]


def _turned(poly, u):
    """A polygon of the frame of the states in the body frame of the heading u at the origin (quarter turns: exact)"""
    poly = np.asarray(poly, dtype=np.float64)
    return np.stack([poly[:, 0] * u[1] - poly[:, 1] * u[0], poly[:, 0] * u[0] + poly[:, 1] * u[1]], axis=1)


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_the_identity_pose_is_the_zone_engine_bit_for_bit(twin, zone_twin, name):
    """G = 1 and the pose (0, 0, 0, 1): qx = dx * 1 - dy * 0 and qy = dx * 0 + dy * 1 are exact, so the domain twin computes the zone
    twin's predicates on the zone twin's numbers.  Under the other quarter-turn headings the body-frame point is the exact quarter turn
    of the position, and the polygon is turned with it (swapped and negated coordinates: exact); the predicates then run in the turned
    frame, and agree because scene Z has no borderline particle."""
    sc, zones = zref.scene_z(ct=name == "ct")
    assert zref.encounters(sc, zones, "c" if name == "ct" else "a")["border"] == 0
    want = zref.call_twin(zone_twin, sc, zones)
    for lo in (0, 2):      # four of the six zones a call: 0 .. 3 and 2 .. 5 (the 64-gon among them)
        for u in ((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0)):
            doms = [_turned(z, u) for z in zones[lo:lo + 4]]
            if u == (0.0, 1.0):
                assert all(np.array_equal(d, z) for d, z in zip(doms, zones[lo:lo + 4]))
            got = dref.call_twin(twin, sc, doms, dref.fixed_poses((0.0, 0.0) + u, sc["K"]))
            assert got["inside"].shape == (4, 1, 8, 70)
            for k in ("inside", "firstAt", "ever"):
                assert np.array_equal(got[k][:, 0], want[k][lo:lo + 4]), (lo, u, k)
            assert np.array_equal(got["valid"], want["valid"]) and np.array_equal(got["status"], want["status"])
    assert want["ever"][[0, 1, 2, 5]].any(axis=1).all()


def test_a_disc_lies_between_its_inscribed_and_circumscribed_polygon(twin):
    """Straight own paths (standing on, half speed, one and a half): the heading is constant, so the body-frame path is the relative
    path turned, and distances are kept.  A regular 64-gon inscribed in radius R - 1e-6 m lies in the disc, one circumscribed about
    R + 1e-6 m holds it: ever_in <= ever_disc <= ever_out and inside_in <= within <= inside_out, per cell, no exception.  The margin of
    1e-6 m is a condition, not a tolerance: the transform rounds at some 1e-12 m at these coordinates."""
    R = 150.0
    sc = dict(ref.scene_a(), S=1024, R=R)
    cand = np.array([[0.0, 1.0, 0.0], [0.0, 0.5, 0.0], [0.0, 1.5, 0.0]])
    poses = dref.poses_of(sc["x"][0, :4], cand, sc["K"], sc["dt"])
    assert (poses[:, :, 2:] == poses[0, 0, 2:]).all()
    own = np.ascontiguousarray(poses[:, :, :2])
    disc = ref.encounters(sc["x"], sc["P"], sc["first"], sc["cdf"], sc["Phi"], sc["Q"], own, sc["K"], sc["dt"], R, sc["S"], sc["seed"], False)
    doms = [zref.reg(64, R - 1e-6, (0.0, 0.0), 0.0), zref.reg(64, (R + 1e-6) / np.cos(np.pi / 64), (0.0, 0.0), 0.0)]
    assert np.abs(poses[..., :2]).max() < 1e4      # (coordinates of some km: eps * 1e4 * a few operations is of order 1e-12 m)
    want = dref.encounters(sc, doms, poses, "a")
    got = dref.call_twin(twin, sc, doms, poses)
    assert want["border"] == 0 and dref.same_counts(got, {k: want[k] for k in dref.COUNTS})
    for label, o in (("reference", want), ("twin", got)):
        assert (o["ever"][0] <= disc["ever"]).all() and (disc["ever"] <= o["ever"][1]).all(), label
        assert (o["inside"][0] <= disc["within"]).all() and (disc["within"] <= o["inside"][1]).all(), label
    # the sandwich is tight and not empty: the polygons differ from the disc by 0.12 % of R at most
    print("ever: inscribed %d, disc %d, circumscribed %d" % (got["ever"][0].sum(), disc["ever"].sum(), got["ever"][1].sum()))
    assert disc["ever"].sum() > 5000 and got["ever"][1].sum(dtype=np.int64) - got["ever"][0].sum(dtype=np.int64) <= 0.01 * disc["ever"].sum()
    assert ((disc["ever"] > 0) & (disc["ever"] < sc["S"])).sum() >= 20


BOW_HEAVY = np.array([(-100, -100), (100, -100), (100, 200), (0, 600), (-100, 200)], dtype=np.float64)      # 600 m ahead, 100 m astern


def test_a_bow_heavy_domain_tells_ahead_from_astern_and_follows_a_turn(twin):
    """The own ship at the origin, 5 m/s due north.  Two targets, 10 m/s east and 5 m/s north, so that each crosses the own ship's
    track from port to starboard at a constant distance: one 400 m AHEAD, one 400 m ASTERN (sigma 30 m and 1 m/s).  A disc cannot tell
    them apart; the domain reaches 600 m ahead and 100 m astern.  Standing on: 2 695 of 4 096 particles of the one ahead enter the
    domain, 451 of the one astern.  Turning 60 degrees to starboard at 3 degrees a second -- away from where the target ahead is --
    lowers the first figure to 789; turning 60 degrees to port, towards it, raises it to 4 094."""
    from pymht_amd import evaluation
    from pymht_amd.models import pv
    K, dt, S = 12, 5.0, 4096
    Phi, Q = eref.model_matrices(pv, dt)
    x = np.array([[-300.0, 400.0, 10.0, 5.0], [-300.0, -400.0, 10.0, 5.0]])
    P = np.tile(np.diag([900.0, 900.0, 1.0, 1.0]), (2, 1, 1))
    sc = ref.scene(x, P, [0, 1, 2], np.ones(2), Phi, Q, np.zeros((1, K + 1, 2)), K=K, dt=dt, S=S)
    cand = np.array([[0.0, 1.0, 0.0], [-np.radians(60.0), 1.0, 0.0], [np.radians(60.0), 1.0, 0.0]])
    poses = evaluation.mc_own_poses([0.0, 0.0, 0.0, 5.0], cand, np.radians(3.0), K, dt)
    got, want = dref.call_twin(twin, sc, [BOW_HEAVY], poses), dref.encounters(sc, [BOW_HEAVY], poses)
    assert want["border"] == 0 and dref.same_counts(got, {k: want[k] for k in dref.COUNTS})
    ever = got["ever"][0]
    print("ever [path][target]: %s" % ever.tolist())
    assert ever.tolist() == [[2695, 451], [789, 583], [4094, 577]]
    d = evaluation.mc_domain_derive(got["inside"], got["firstAt"], got["ever"], got["valid"], dt)
    assert d["pEver"][0, 0, 0] > 5 * d["pEver"][0, 0, 1] and d["pEver"][0, 1, 0] < 0.3 * d["pEver"][0, 0, 0] and d["pEver"][0, 2, 0] > 0.99
    # the mirror image: the domain drawn stern-heavy scores the two targets the other way round
    stern = BOW_HEAVY * np.array([1.0, -1.0])
    back = dref.call_twin(twin, sc, [stern], poses[:1])["ever"][0, 0]
    assert back[1] > 5 * back[0]


@pytest.mark.parametrize("kind", dref.KINDS)
def test_no_scene_of_the_gpu_tests_has_a_borderline_particle(twin, kind):
    """What reduces the GPU criterion to equality.  A scene that has one is moved, not the rule."""
    sc, doms, poses = dref.shape_scene(kind)
    want = dref.encounters(sc, doms, poses)
    got = dref.call_twin(twin, sc, doms, poses)
    print("%s: %d borderline particles of %d walked" % (kind, want["border"], want["walked"]))
    assert want["border"] == 0 and not want["borderInside"].any()
    assert dref.same_counts(got, {k: want[k] for k in dref.COUNTS})
    dref.check_invariants(got)
    check_shape(kind, sc, doms, poses, got)


def check_shape(kind, sc, doms, poses, o):
    """What a shape's scene is for, on a set of counts (the twin's here, the device's in tests/test_mc_domain_gpu.py)"""
    S, D, G = sc["S"], len(doms), len(poses)
    assert o["inside"].shape == (D, G, sc["K"] + 1, len(sc["first"]) - 1)
    if kind == "every target far":
        assert not o["inside"].any() and not o["firstAt"].any() and not o["ever"].any() and (o["valid"] == S).sum() == 68
        return
    assert o["inside"].any() and o["firstAt"][:, :, 1:].any() and ((o["ever"] > 0) & (o["ever"] < S)).any()
    if kind == "S=320":
        assert ref.chunks(70, 320) == (2, 256)      # a last chunk of 64: three wavefronts of it walk along and count nowhere
    if kind == "T=1, S=65536":
        assert ref.chunks(1, 65536) == (256, 256)
    if kind == "T=1030":
        assert ref.chunks(1030, 128) == (1, 256) and not np.array_equal(o["ever"][..., :70], o["ever"][..., 70:140])      # (keyed by the target: a copy is another draw)
    if kind == "K=64":
        assert o["inside"][:, :, 64].any() and o["firstAt"][:, :, 33:].any()
    if kind in ("1 x 64", "4 x 16"):
        assert D * G == 64 and all(((o["ever"][d, g] > 0) & (o["ever"][d, g] < S)).any() for d in range(D) for g in range(G))
        flat = o["ever"].reshape(64, -1)
        assert len({row.tobytes() for row in flat}) == 64      # every cell its own counts: no two lanes' rows confused
    if kind == "256 vertices":
        assert dref.pack(doms)[0].tolist() == [0, 256]
    if kind == "67 components":
        assert (sc["first"][1:] - sc["first"][:-1]).tolist() == [67, 1, 1]
    if kind.startswith("near and far"):
        # half of every target's particles are 20 km away and never enter; of the near half some do
        assert (o["ever"] <= 0.62 * S).all() and (o["ever"][1] > 0.1 * S).all()


def _pv():
    from pymht_amd.models import pv
    return eref.model_matrices(pv, ref.DT)


def test_own_poses():
    from pymht_amd import evaluation
    own, w = [100.0, -50.0, 3.0, 4.0], np.radians(2.0)
    cand = np.array([[0.0, 1.0, 0.0], [0.6, 1.0, 10.0], [-0.6, 0.5, 0.0], [np.pi, 1.0, 0.0], [np.nan, 1.0, 0.0], [0.3, 0.0, 7.5]])
    poses = evaluation.mc_own_poses(own, cand, w, 9, 5.0)
    paths = evaluation.mc_own_paths(own, cand, w, 9, 5.0)
    assert poses.shape == (6, 10, 4) and poses.dtype == np.float64 and poses.flags["C_CONTIGUOUS"]
    assert np.array_equal(poses[:, :, :2], paths, equal_nan=True) and poses[:, :, :2].tobytes() == paths.tobytes()      # bit for bit
    assert np.isnan(poses[4]).all() and np.isfinite(np.delete(poses, 4, axis=0)).all()
    good = np.delete(poses, 4, axis=0)
    assert np.abs(good[..., 2] ** 2 + good[..., 3] ** 2 - 1.0).max() <= 1e-12
    assert (poses[0, :, 2:] == [0.6, 0.8]).all()      # standing on: v0 / |v0| at every step
    # the turn: 0 until t0 = 10 s, w (t - t0) on the arc, dpsi after te = t0 + 0.6 / w = 27.2 s; counter-clockwise for dpsi > 0
    ang = np.arctan2(poses[1, :, 3], poses[1, :, 2]) - np.arctan2(0.8, 0.6)
    want = np.clip(w * (np.arange(10) * 5.0 - 10.0), 0.0, 0.6)
    assert np.abs(ang - want).max() < 1e-12 and np.abs(np.arctan2(poses[2, -1, 3], poses[2, -1, 2]) - np.arctan2(0.8, 0.6) + 0.6) < 1e-12
    # the heading is the direction of travel: the chord of a step on the straight legs, the velocity's direction at the arc's end
    leg = paths[1, 9] - paths[1, 8]
    assert np.abs(leg / np.hypot(*leg) - poses[1, 9, 2:]).max() < 1e-9
    assert np.abs(poses[3, -1, 2:] - [-0.8, 0.6]).max() < 1e-12      # 45 s at 2 degrees a second: a quarter turn to port of a half turn asked for
    # a ship that stops keeps its heading
    assert np.abs(poses[5, -1, 2:] - [0.6 * np.cos(0.3) - 0.8 * np.sin(0.3), 0.6 * np.sin(0.3) + 0.8 * np.cos(0.3)]).max() < 1e-12
    assert np.isnan(evaluation.mc_own_poses([0.0, np.nan, 1.0, 1.0], cand[:1], w, 3, 5.0)).all()
    for bad in (dict(own=[0.0, 0.0, 0.0, 0.0]), dict(own=[0.0, 0.0, 1.0]), dict(own=[0.0, 0.0, np.inf, 1.0]), dict(turnRate=0.0), dict(turnRate=-1.0), dict(steps=0),
                dict(steps=65), dict(dt=0.0), dict(candidates=[[4.0, 1.0, 0.0]]), dict(candidates=[[0.0, -1.0, 0.0]]), dict(candidates=np.zeros((0, 3)))):
        with pytest.raises(ValueError, match="mc_own_poses"):
            evaluation.mc_own_poses(**dict(dict(own=own, candidates=cand, turnRate=w, steps=9, dt=5.0), **bad))
    with pytest.raises(ValueError, match="speed 0"):
        evaluation.mc_own_poses([1.0, 2.0, 0.0, 0.0], cand, w, 9, 5.0)


TRIANGLE = [[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]]
SQUARE = [(0, 0), (10, 0), (10, 10), (0, 10)]


def test_every_value_error_is_raised_without_a_device(monkeypatch):
    from pymht_amd import evaluation

    def no_device(*a, **kw):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(evaluation, "Context", no_device)
    Phi, Q = _pv()
    x, P = np.zeros((3, 4)), np.tile(np.eye(4), (3, 1, 1))
    pose = dref.fixed_poses((1.0, 2.0, 0.6, 0.8), 4, G=2)
    good = dict(x=x, P=P, target=[4, 4, 9], weight=[1.0, 2.0, 1.0], Phi=Phi, Q=Q, steps=4, dt=5.0, domains=[TRIANGLE], ownPoses=pose)
    off, nan, inf = pose.copy(), pose.copy(), pose.copy()
    off[1, 3, 2:] = [0.6, 0.8004]
    nan[0, 0, 0] = np.nan
    inf[1, 4, 3] = np.inf
    bad = [dict(x=np.zeros((3, 5))), dict(P=P[:2]), dict(Phi=np.eye(6)), dict(Q=np.full((4, 4), np.nan)), dict(steps=0), dict(steps=65), dict(steps=2.0),
           dict(dt=0.0), dict(dt=np.inf), dict(particles=100), dict(particles=32), dict(particles=(1 << 20) + 64), dict(particles=64.0),
           dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5), dict(transition="ct"), dict(transition="arc"), dict(target=[0, 0]), dict(target=[0.0, 0.0, 1.0]),
           dict(weight=[1.0, 2.0]), dict(weight=[1.0, -2.0, 1.0]), dict(weight=[0.0, 0.0, 1.0]), dict(weight=[1.0, np.inf, 1.0]), dict(weight=[1.0, np.nan, 1.0]),
           dict(domains=[TRIANGLE[:2]]), dict(domains=[TRIANGLE, [[0.0, 0.0, 0.0]] * 3]), dict(domains=[np.zeros(6)]), dict(domains=np.zeros((3, 2))),
           dict(domains=[[[0.0, 0.0], [1.0, np.nan], [1.0, 1.0]]]), dict(domains=[[[0.0, 0.0], [np.inf, 0.0], [1.0, 1.0]]]), dict(domains=[TRIANGLE] * 5),
           dict(domains=[np.zeros((257, 2))]), dict(domains=[np.zeros((128, 2)), np.zeros((129, 2))]), dict(domains=[["a", "b"]] * 3), dict(domains=5),
           dict(domains=[]), dict(ownPoses=pose[:, :4]), dict(ownPoses=pose[:, :, :2]), dict(ownPoses=pose[0]), dict(ownPoses=pose[:0]), dict(ownPoses="north"),
           dict(ownPoses=off), dict(ownPoses=nan), dict(ownPoses=inf), dict(ownPoses=dref.fixed_poses((0.0, 0.0, 0.0, 1.0), 4, G=65)),
           dict(ownPoses=dref.fixed_poses((0.0, 0.0, 0.0, 1.0), 4, G=17), domains=[TRIANGLE] * 4), dict(ownPoses=dref.fixed_poses((0.0, 0.0, 0.0, 0.0), 4))]
    for change in bad:
        with pytest.raises(ValueError, match="mc_domain_encounters"):
            evaluation.mc_domain_encounters(**dict(good, **change))
    with pytest.raises(ValueError, match="domain 1"):
        evaluation.mc_domain_encounters(**dict(good, domains=[TRIANGLE, TRIANGLE[:2]]))
    with pytest.raises(ValueError, match="256 vertices"):
        evaluation.mc_domain_encounters(**dict(good, domains=[np.zeros((257, 2))]))
    with pytest.raises(ValueError, match="64 cells"):
        evaluation.mc_domain_encounters(**dict(good, domains=[TRIANGLE] * 2, ownPoses=dref.fixed_poses((0.0, 0.0, 0.0, 1.0), 4, G=33)))
    with pytest.raises(ValueError, match="unit vector"):
        evaluation.mc_domain_encounters(**dict(good, ownPoses=off))
    # no component: empty arrays and no device call
    empty = evaluation.mc_domain_encounters(np.zeros((0, 4)), np.zeros((0, 4, 4)), np.zeros(0, dtype=np.int64), np.zeros(0), Phi, Q, 4, 5.0, [TRIANGLE, SQUARE], pose)
    assert empty["inside"].shape == (2, 2, 5, 0) and empty["firstAt"].shape == (2, 2, 5, 0) and empty["ever"].shape == (2, 2, 0) and empty["pEver"].shape == (2, 2, 0)
    assert empty["domFirst"].tolist() == [0, 3, 7] and empty["domXY"].shape == (7, 2) and empty["pInsideMax"].shape == (2, 2, 0) and empty["pEverBy"].shape == (2, 2, 5, 0)
    assert empty["inside"].dtype == np.uint32 and empty["status"].dtype == np.int32 and empty["status"].shape == (0,) and np.array_equal(empty["ownPoses"], pose)
    assert (evaluation.MC_DOMAIN_MAX_DOMAINS, evaluation.MC_DOMAIN_MAX_VERTS, evaluation.MC_DOMAIN_MAX_CELLS) == (dref.MAX_DOMAINS, dref.MAX_VERTS, dref.MAX_CELLS) == (4, 256, 64)
    # the packing itself
    df, dxy = evaluation.mc_domain_pack([TRIANGLE, SQUARE])
    wf, wxy = dref.pack([TRIANGLE, SQUARE])
    assert df.dtype == np.int32 and dxy.dtype == np.float64 and np.array_equal(df, wf) and np.array_equal(dxy, wxy) and dxy.flags["C_CONTIGUOUS"]
    assert evaluation.mc_domain_pack(np.zeros((2, 3, 2)) + np.arange(3)[None, :, None])[0].tolist() == [0, 3, 6]
    for wrong in ([TRIANGLE] * 5, [np.zeros((257, 2))], [TRIANGLE[:2]]):
        with pytest.raises(ValueError, match="mc_domain_pack"):
            evaluation.mc_domain_pack(wrong)


def test_the_hosts_figures():
    """mc_domain_derive on hand-made counts: mc_zone_derive's fields over the cell axes [nDomain, G]"""
    from pymht_amd import evaluation
    inside = np.zeros((2, 3, 4, 2), dtype=np.uint32)
    first_at = np.zeros((2, 3, 4, 2), dtype=np.uint32)
    ever = np.zeros((2, 3, 2), dtype=np.uint32)
    inside[1, 2, :, 0], first_at[1, 2, :, 0], ever[1, 2, 0] = [0, 32, 32, 5], [0, 32, 0, 8], 40
    inside[0, 1, :, 0], first_at[0, 1, :, 0], ever[0, 1, 0] = [64, 0, 0, 0], [64, 0, 0, 0], 64
    inside[:, :, :, 1] = 10
    valid = np.array([64, 0], dtype=np.uint32)
    d = evaluation.mc_domain_derive(inside, first_at, ever, valid, 2.5)
    z = evaluation.mc_zone_derive(inside.reshape(6, 4, 2), first_at.reshape(6, 4, 2), ever.reshape(6, 2), valid, 2.5)
    assert sorted(d) == sorted(z) == sorted(["pInside", "pInsideMax", "tInside", "pEver", "pEverBy", "sePInsideMax", "sePEver"])
    assert all(np.array_equal(d[k].reshape(z[k].shape), z[k], equal_nan=True) for k in d)
    assert d["pInside"].shape == (2, 3, 4, 2) and d["pEverBy"].shape == (2, 3, 4, 2) and all(d[k].shape == (2, 3, 2) for k in ("pInsideMax", "tInside", "pEver", "sePEver"))
    assert d["pInside"][1, 2, :, 0].tolist() == [0.0, 0.5, 0.5, 5 / 64] and d["pInsideMax"][1, 2, 0] == 0.5 and d["tInside"][1, 2, 0] == 2.5
    assert d["pEver"][1, 2, 0] == 40 / 64 and d["pEverBy"][1, 2, :, 0].tolist() == [0.0, 0.5, 0.5, 40 / 64] and d["pEver"][0, 1, 0] == 1.0 and d["tInside"][0, 1, 0] == 0.0
    assert d["sePEver"][1, 2, 0] == np.sqrt((40 / 64) * (24 / 64) / 64) and d["pEver"][0, 0, 0] == 0.0
    assert all(np.isnan(d[k][..., 1]).all() for k in d)


def test_the_documents_say_what_the_definition_says():
    from pymht_amd import evaluation
    from pymht_amd.tracker import Tracker
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    read = lambda *p: open(os.path.join(root, *p)).read()
    texts = [evaluation.mc_domain_encounters.__doc__, Tracker.getMonteCarloDomainEncounters.__doc__, read("include", "mht_amd.h"), read("README.md"),
             read("pymht_amd", "csrc", "mht_mc_domain.h")]
    for text in texts:
        flat = " ".join(text.replace("\n * ", "\n").replace("\n// ", "\n").split()).lower()
        for item in ("straight", "chord", "right of the heading", "ahead", "stationary own ship", "scales with speed", "holes", "64 cells"):
            assert item in flat, item
    assert "DECIDING DOMAIN GOES FIRST" in texts[1] and "pEverBy" in texts[0]
    readme = " ".join(read("README.md").split())
    assert "getMonteCarloDomainEncounters" in readme and "mc_domain_cost.txt" in readme


def test_the_twin_refuses_what_the_seam_refuses(twin):
    sc, doms, poses = dref.shape_scene("S=64")
    df, dxy = dref.pack(doms)
    assert df.tolist() == [0, 5, 11]
    assert not dref.untouched(dref.call_twin(twin, sc, doms, poses))
    bad_xy = dxy.copy()
    bad_xy[7, 1] = np.inf
    for packed in (([0, 5, 7, 11], dxy), ([0, 9, 11], dxy), ([1, 5, 11], dxy), ([0, 5, 10], dxy), ([0, 11, 5], dxy), (df, bad_xy),
                   (np.arange(6) * 3, np.zeros((15, 2))), ([0, 257], np.zeros((257, 2)))):
        assert dref.untouched(dref.call_twin(twin, sc, None, poses, expect=-1, packed=packed))
    long, nan, many = poses.copy(), poses.copy(), np.tile(poses[:1], (33, 1, 1))
    long[3, 2, 2:] *= 1.001
    nan[5, 7, 1] = np.nan
    for p in (long, nan, many):
        assert dref.untouched(dref.call_twin(twin, sc, doms, p, expect=-1))
    for change in (dict(S=100), dict(K=0), dict(K=65), dict(dt=0.0)):
        assert dref.untouched(dref.call_twin(twin, dict(sc, **change), doms, poses, expect=-1))


def test_the_twin_on_its_own_under_a_sanitizer(tmp_path):
    """tests/hostmath/mc_domain_host_main.cpp: a program of its own (nothing of it is loaded into Python, nothing is preloaded), built
    with -fsanitize=address,undefined and run as a child process on dumped scenes D (pv and ct) at S = 256; it prints the reference's
    counts."""
    gxx = shutil.which("g++") or "g++"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mc_domain_host_main")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # (the runtimes in the program itself: it needs nothing from its environment)
                           os.path.join(root, "tests", "hostmath", "mc_domain_host_main.cpp"), "-o", exe])
    files, wants = [], []
    for name in ("pv", "ct"):
        sc, doms, poses = dref.scene_d(ct=name == "ct", S=256)
        files.append(str(tmp_path / ("scene_d_%s.bin" % name)))
        dref.dump(sc, doms, poses, files[-1])
        want = dref.encounters(sc, doms, poses)
        assert want["border"] == 0
        wants.append("%s: inside %d firstAt %d ever %d valid %d" % (files[-1], want["inside"].sum(dtype=np.int64), want["firstAt"].sum(dtype=np.int64),
                                                                   want["ever"].sum(dtype=np.int64), want["valid"].sum(dtype=np.int64)))
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.strip().splitlines() == wants, (run.stdout, wants)
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    short = str(tmp_path / "short.bin")
    with open(files[0], "rb") as fh, open(short, "wb") as out:
        out.write(fh.read()[:-8])
    assert subprocess.run([exe, short], capture_output=True).returncode == 1
