"""CPU: the zone engine's host twin (tests/hostmath/mc_zone_host.cpp, csrc/mht_mc_zone.h compiled for the CPU) against the NumPy
reference tests/mc_zone_ref.py, which is built on tests/mc_ref.py's own particles and states the borderline rule every comparison of
counts uses; the header's predicates on hand-stated cases; an independent half-plane rule for the convex zones; and
pymht_amd.evaluation's host side (mc_zone_pack, every ValueError of mc_zone_encounters, the derived figures) without a device.

SCENE Z is mc_ref.scene_a() (70 models/pv targets, entries 5 and 9 NaN) or scene_c() (its constant-turn lift) at S = 1024, K = 7,
seed 12345, with six zones about c, the median of the targets' positions: a pentagon of radius 400, a concave U, a sliver 2 m wide and
4 km long, a square of +-1e5 that holds every scored particle at every step, a triangle 70 km away that nothing touches, and a 64-gon in
reversed order.  Read from the reference when written: no borderline particle in either scene, so the twin's counts are expected to
EQUAL the reference's; zones 0, 1, 2 and 5 are hit by some and not all particles of 61, 63, 64 and 57 targets (pv) and 57, 59, 63 and 58
(ct), with 196 to 261 non-zero firstAt[k > 0] cells per zone; the sliver has 589 particle-steps inside and 14 387 particles that hit it
(pv): what the segment test is for."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import encounter_ref as eref
import mc_pair_ref as pref
import mc_ref as ref
import mc_zone_ref as zref


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return zref.build_twin(tmp_path_factory.mktemp("mc_zone_twin"))


@pytest.fixture(scope="module")
def scenes(twin):
    """Scene Z for models pv and ct: (scene, zones, the twin's counts, the reference's), computed once (seconds)"""
    out = {}
    for name in ("pv", "ct"):
        sc, zones = zref.scene_z(ct=name == "ct")
        out[name] = (sc, zones, zref.call_twin(twin, sc, zones), zref.encounters(sc, zones, "c" if name == "ct" else "a"))
    return out


PARTLY = {"pv": {0: 61, 1: 63, 2: 64, 5: 57}, "ct": {0: 57, 1: 59, 2: 63, 5: 58}}


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_twin_equals_the_reference_on_scene_z(scenes, name):
    sc, zones, got, want = scenes[name]
    S, T = sc["S"], 70
    differ = zref.hold_counts("scene Z, %s" % name, got, want)
    print("scene Z, %s: %d borderline particles of %d walked, %d cells differ" % (name, want["border"], want["walked"], differ))
    assert want["border"] == 0 and differ == 0 and want["walked"] == 6 * 68 * S
    assert not any((got[k] == zref.SENTINEL).any() for k in ("inside", "firstAt", "ever", "valid")) and got["inside"].shape == (6, 8, T)
    zref.check_invariants(got)
    zref.check_invariants(want)
    nan = [eref.NAN_X, eref.NAN_P]
    assert got["status"][nan].tolist() == [1, 1] and got["valid"][nan].tolist() == [0, 0] and int((got["status"] == 0).sum()) == T - 2
    scored = got["status"] == 0
    # the containing zone: every scored particle at every step, all of them first at step 0; the far zone: nothing
    assert (got["inside"][zref.CONTAINING][:, scored] == S).all() and (got["ever"][zref.CONTAINING][scored] == S).all()
    assert (got["firstAt"][zref.CONTAINING][0, scored] == S).all() and not got["firstAt"][zref.CONTAINING][1:].any()
    assert not got["inside"][zref.FAR].any() and not got["firstAt"][zref.FAR].any() and not got["ever"][zref.FAR].any()
    for z, n in PARTLY[name].items():
        e = got["ever"][z]
        cells = int((got["firstAt"][z, 1:] > 0).sum())
        assert int(((e > 0) & (e < S)).sum()) == n and 190 <= cells <= 270, (z, cells)
    if name == "pv":      # the sliver: few particle-steps inside, many particles through it
        assert int(got["inside"][2].sum()) == 589 and int(got["ever"][2].sum()) == 14387


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_vertex_order_and_start_do_not_move_a_count(scenes, twin, name):
    sc, zones, got, want = scenes[name]
    assert not want["borderInside"].any()      # (no borderline point: inside is held too)
    for label, other in (("reversed", [z[::-1].copy() for z in zones]), ("rotated", [np.roll(z, 1 + len(z) // 3, axis=0) for z in zones])):
        again = zref.call_twin(twin, sc, other)
        assert zref.same_counts(again, got), label
    # zones in another order: the same rows in that order
    perm = [5, 0, 3, 1, 4, 2]
    again = zref.call_twin(twin, sc, [zones[z] for z in perm])
    assert all(np.array_equal(again[k], got[k][perm]) for k in ("inside", "firstAt", "ever"))


@pytest.mark.parametrize("name", ["pv", "ct"])
def test_a_half_plane_rule_agrees_on_the_convex_zones(scenes, name):
    sc, zones, got, _ = scenes[name]
    status, paths = pref.target_paths(sc, "c" if name == "ct" else "a")
    steps = 0
    for z in zref.CONVEX:
        for t in np.flatnonzero(np.asarray(status) == 0):
            x, y = paths[int(t)][:, 0], paths[int(t)][:, 1]
            mine, plain = zref.point_in(zones[z], x, y), zref.half_plane_inside(zones[z], x, y)
            assert np.array_equal(mine, plain), (z, t)
            assert np.array_equal(got["inside"][z, :, t], plain.sum(axis=1))      # the twin's counts are that rule's
            steps += mine.size
    assert steps == 2 * 68 * 8 * sc["S"]


def test_a_particle_is_the_other_engines_particle_and_the_skip_moves_no_flag(scenes, twin):
    for name in ("pv", "ct"):
        sc, zones, got, _ = scenes[name]
        _, paths = pref.target_paths(sc, "c" if name == "ct" else "a")
        came = np.zeros(6, dtype=np.int64)
        for t, p in ((0, 0), (12, 7), (33, 1023), (69, 500), (20, 64)):
            one, every = zref.twin_path(twin, sc, zones, t, p), zref.twin_path(twin, sc, zones, t, p, skip=False)
            assert all(np.array_equal(one[k], every[k]) for k in ("states", "inside", "first", "came"))
            want = paths[t][:, :, p]
            assert np.abs(one["states"][:, :2] - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
            x, y = one["states"][:, 0], one["states"][:, 1]
            for z, poly in enumerate(zones):
                i = zref.point_in(poly, x, y)
                hit = i.copy()
                hit[1:] |= zref.segment_crosses(poly, x[:-1], y[:-1], x[1:], y[1:])
                first = hit & ~np.concatenate([[False], np.logical_or.accumulate(hit)[:-1]])
                assert np.array_equal(one["inside"][z], i) and np.array_equal(one["first"][z], first) and one["came"][z] == hit.any()
            came += one["came"]
        assert came[zref.CONTAINING] == 5 and came[zref.FAR] == 0


SQUARE = [(0, 0), (10, 0), (10, 10), (0, 10)]
NOTCHED = [(0, 0), (10, 0), (6, 5), (10, 10), (0, 10)]      # (6, 5) is a reflex vertex, not an extreme of the box


def test_the_predicates_on_hand_stated_cases(twin):
    point = lambda poly, p: zref.twin_test(twin, poly, p)[0]
    cross = lambda poly, p, q: zref.twin_test(twin, poly, p, q)[1]
    both = lambda poly, p, q: zref.twin_test(twin, poly, p, q)
    for poly in (SQUARE, SQUARE[::-1], SQUARE[2:] + SQUARE[:2]):
        # a point on a vertex, on a horizontal edge: the lower and left sides belong to the zone, the upper and right ones do not
        assert point(poly, (0, 0)) and not point(poly, (10, 10)) and not point(poly, (10, 0)) and not point(poly, (0, 10))
        assert point(poly, (5, 0)) and not point(poly, (5, 10)) and point(poly, (0, 5)) and not point(poly, (10, 5))
        assert point(poly, (5, 5)) and not point(poly, (-1e-9, 5)) and not point(poly, (5, 10.000001))
        # collinear with the bottom edge: disjoint misses (the box test), overlapping and touching hit
        assert not cross(poly, (12, 0), (20, 0)) and cross(poly, (5, 0), (15, 0)) and cross(poly, (10, 0), (20, 0)) and not cross(poly, (-9, 0), (-1, 0))
        # a segment ending on a vertex, from outside
        assert both(poly, (-5, -5), (0, 0)) == (True, True) and both(poly, (15, 15), (10, 10)) == (False, True)
        # a zero-length segment: away from the zone, inside it (the step test's business, no edge is met) and on an edge
        assert both(poly, (20, 20), (20, 20)) == (False, False) and both(poly, (5, 5), (5, 5)) == (True, False) and both(poly, (5, 10), (5, 10)) == (False, True)
        # through the zone with both ends outside, and passing it by
        assert both(poly, (-5, 3), (15, 4)) == (False, True) and both(poly, (-5, 3), (-1, 30)) == (False, False)
        # wholly inside: no edge is met, the steps see it
        assert both(poly, (2, 2), (8, 7)) == (True, False)
    for poly in (NOTCHED, NOTCHED[::-1]):
        # level with the vertex (6, 5): the > rule counts the two edges that meet there once between them
        assert point(poly, (3, 5)) and not point(poly, (8, 5)) and point(poly, (5.999, 5)) and not point(poly, (6.001, 5))
        assert not point(poly, (-3, 5)) and not point(poly, (12, 5))
    # the sliver, 2 m wide: a segment through it with both ends outside
    assert both(zref.SLIVER, (0, -10), (0, 10)) == (False, True) and both(zref.SLIVER, (0, -10), (3, -2)) == (False, False)
    assert both(zref.SLIVER, (0, -10), (0, 0.25)) == (True, True)
    # the U's notch: crossed without entering -- through its open end, and from side to side inside it; its floor is an edge
    for u in (zref.U_SHAPE, zref.U_SHAPE[::-1]):
        assert both(u, (0, 400), (0, -100)) == (False, False) and both(u, (-100, 100), (100, 100)) == (False, False)
        assert both(u, (0, 400), (0, -200)) == (True, True) and both(u, (-100, 100), (200, 100)) == (True, True)
        assert both(u, (-100, 100), (400, 100)) == (False, True) and point(u, (0, -200)) and not point(u, (0, 0))
    # fewer than three vertices, and a vertex that is not finite: refused
    out = np.zeros(2, dtype=np.int32)
    for bad in (np.array(SQUARE[:2], dtype=np.float64), np.array([(0, 0), (1, 0), (np.nan, 1)])):
        assert twin.mc_zone_test_host(len(bad), bad.ctypes.data, 0.0, 0.0, 0.0, 0.0, 0, out.ctypes.data) == -1


def test_the_twin_refuses_what_the_seam_refuses(twin):
    sc, zones = zref.scene_stride()
    sc = dict(sc, S=64)
    zf, zxy = zref.pack(zones)
    assert zf.tolist() == [0, 3, 7, 14]
    good = zref.call_twin(twin, sc, zones)
    assert not zref.untouched(good)
    nan = zxy.copy()
    nan[5, 1] = np.inf
    for packed in (([0, 3, 5, 14], zxy), ([0, 12, 14], zxy), ([1, 3, 7, 14], zxy), ([0, 3, 7, 13], zxy), ([0, 7, 3, 14], zxy), (zf, nan),
                   (np.arange(34) * 3, np.zeros((99, 2))), ([0, 1025], np.zeros((1025, 2)))):
        assert zref.untouched(zref.call_twin(twin, sc, None, expect=-1, packed=packed))
    for change in (dict(S=100), dict(K=0), dict(K=65), dict(dt=0.0)):
        assert zref.untouched(zref.call_twin(twin, dict(sc, **change), zones, expect=-1))


def _pv():
    from pymht_amd.models import pv
    return eref.model_matrices(pv, ref.DT)


TRIANGLE = [[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]]


def test_every_value_error_is_raised_without_a_device(monkeypatch):
    from pymht_amd import evaluation

    def no_device(*a, **kw):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(evaluation, "Context", no_device)
    Phi, Q = _pv()
    x, P = np.zeros((3, 4)), np.tile(np.eye(4), (3, 1, 1))
    good = dict(x=x, P=P, target=[4, 4, 9], weight=[1.0, 2.0, 1.0], Phi=Phi, Q=Q, steps=4, dt=5.0, zones=[TRIANGLE])
    bad = [dict(x=np.zeros((3, 5))), dict(P=P[:2]), dict(Phi=np.eye(6)), dict(Q=np.full((4, 4), np.nan)), dict(steps=0), dict(steps=65), dict(steps=2.0),
           dict(dt=0.0), dict(dt=np.inf), dict(particles=100), dict(particles=32), dict(particles=(1 << 20) + 64), dict(particles=64.0),
           dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5), dict(transition="ct"), dict(transition="arc"), dict(target=[0, 0]), dict(target=[0.0, 0.0, 1.0]),
           dict(weight=[1.0, 2.0]), dict(weight=[1.0, -2.0, 1.0]), dict(weight=[0.0, 0.0, 1.0]), dict(weight=[1.0, np.inf, 1.0]), dict(weight=[1.0, np.nan, 1.0]),
           dict(zones=[TRIANGLE[:2]]), dict(zones=[TRIANGLE, [[0.0, 0.0, 0.0]] * 3]), dict(zones=[np.zeros(6)]), dict(zones=np.zeros((3, 2))),
           dict(zones=[[[0.0, 0.0], [1.0, np.nan], [1.0, 1.0]]]), dict(zones=[[[0.0, 0.0], [np.inf, 0.0], [1.0, 1.0]]]), dict(zones=[TRIANGLE] * 33),
           dict(zones=[np.zeros((1025, 2))]), dict(zones=[np.zeros((512, 2)), np.zeros((513, 2))]), dict(zones=[["a", "b"]] * 3), dict(zones=5)]
    for change in bad:
        with pytest.raises(ValueError, match="mc_zone_encounters"):
            evaluation.mc_zone_encounters(**dict(good, **change))
    with pytest.raises(ValueError, match="zone 1"):
        evaluation.mc_zone_encounters(**dict(good, zones=[TRIANGLE, TRIANGLE[:2]]))
    with pytest.raises(ValueError, match="1024 vertices"):
        evaluation.mc_zone_encounters(**dict(good, zones=[np.zeros((1025, 2))]))
    # no zone, or no component: empty arrays and no device call
    none = evaluation.mc_zone_encounters(**dict(good, zones=[]))
    assert none["inside"].shape == (0, 5, 0) and none["ever"].shape == (0, 0) and none["valid"].shape == (0,) and none["pEverBy"].shape == (0, 5, 0)
    empty = evaluation.mc_zone_encounters(np.zeros((0, 4)), np.zeros((0, 4, 4)), np.zeros(0, dtype=np.int64), np.zeros(0), Phi, Q, 4, 5.0, [TRIANGLE, SQUARE])
    assert empty["inside"].shape == (2, 5, 0) and empty["firstAt"].shape == (2, 5, 0) and empty["ever"].shape == (2, 0) and empty["pEver"].shape == (2, 0)
    assert empty["zoneFirst"].tolist() == [0, 3, 7] and empty["zoneXY"].shape == (7, 2) and empty["pInsideMax"].shape == (2, 0)
    for r in (none, empty):
        assert r["inside"].dtype == np.uint32 and r["status"].dtype == np.int32 and r["status"].shape == (0,)
    assert (evaluation.MC_ZONE_MAX_ZONES, evaluation.MC_ZONE_MAX_VERTS) == (zref.MAX_ZONES, zref.MAX_VERTS) == (32, 1024)
    # the packing itself
    zf, zxy = evaluation.mc_zone_pack([TRIANGLE, SQUARE])
    wf, wxy = zref.pack([TRIANGLE, SQUARE])
    assert zf.dtype == np.int32 and zxy.dtype == np.float64 and np.array_equal(zf, wf) and np.array_equal(zxy, wxy) and zxy.flags["C_CONTIGUOUS"]
    assert evaluation.mc_zone_pack(np.zeros((2, 3, 2)) + np.arange(3)[None, :, None])[0].tolist() == [0, 3, 6]


def test_the_hosts_figures():
    """mc_zone_derive on hand-made counts: pEverBy = cumsum(firstAt) / valid with its last row pEver, NaN where valid is 0"""
    from pymht_amd import evaluation
    inside = np.array([[[0, 10], [32, 10], [32, 10], [5, 10]]], dtype=np.uint32)        # [1, 4, 2]
    first_at = np.array([[[0, 0], [32, 0], [0, 0], [8, 0]]], dtype=np.uint32)
    ever, valid = np.array([[40, 0]], dtype=np.uint32), np.array([64, 0], dtype=np.uint32)
    d = evaluation.mc_zone_derive(inside, first_at, ever, valid, 2.5)
    assert sorted(d) == sorted(["pInside", "pInsideMax", "tInside", "pEver", "pEverBy", "sePInsideMax", "sePEver"])
    assert d["pInside"][0, :, 0].tolist() == [0.0, 0.5, 0.5, 5 / 64] and d["pInsideMax"][0, 0] == 0.5 and d["tInside"][0, 0] == 2.5
    assert d["pEver"][0, 0] == 40 / 64 and d["pEverBy"][0, :, 0].tolist() == [0.0, 0.5, 0.5, 40 / 64] and d["pEverBy"][0, -1, 0] == d["pEver"][0, 0]
    assert d["sePInsideMax"][0, 0] == evaluation.mc_standard_error(0.5, 64) == np.sqrt(0.25 / 64)
    assert d["sePEver"][0, 0] == np.sqrt((40 / 64) * (24 / 64) / 64)
    assert all(np.isnan(d[k][..., 1]).all() for k in d)
    assert d["pInside"].shape == (1, 4, 2) and d["pEverBy"].shape == (1, 4, 2) and all(d[k].shape == (1, 2) for k in ("pInsideMax", "tInside", "pEver", "sePEver"))


def test_the_docstrings_name_what_is_out_of_scope():
    from pymht_amd import evaluation
    from pymht_amd.tracker import Tracker
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    texts = [evaluation.mc_zone_encounters.__doc__, Tracker.getMonteCarloZoneEncounters.__doc__, open(os.path.join(root, "include", "mht_amd.h")).read(),
             open(os.path.join(root, "README.md")).read(), open(os.path.join(root, "INTEGRATION.md")).read()]
    for text in texts:
        flat = " ".join(text.replace("\n * ", "\n").split())      # (the header's comment lines begin with a star)
        for item in ("move with the own ship", "polygonal ship domain", "open gates and polylines", "thin quadrilateral", "holes", "geodetic", "dwell time"):
            assert item in flat, item
    assert "ranking" in texts[1] and "pEverBy" in texts[0]


def test_the_twin_on_its_own_under_a_sanitizer(tmp_path):
    """tests/hostmath/mc_zone_host_main.cpp: a program of its own (nothing of it is loaded into Python, nothing is preloaded), built with
    -fsanitize=address,undefined and run as a child process on dumped scenes Z (pv and ct) at S = 256; it prints the reference's counts."""
    gxx = shutil.which("g++") or "g++"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mc_zone_host_main")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # (the runtimes in the program itself: it needs nothing from its environment)
                           os.path.join(root, "tests", "hostmath", "mc_zone_host_main.cpp"), "-o", exe])
    files, wants = [], []
    for name in ("pv", "ct"):
        sc, zones = zref.scene_z(ct=name == "ct")
        sc = dict(sc, S=256)
        files.append(str(tmp_path / ("scene_z_%s.bin" % name)))
        zref.dump(sc, zones, files[-1])
        want = zref.encounters(sc, zones)
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
