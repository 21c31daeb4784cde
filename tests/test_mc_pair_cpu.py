"""CPU: the pair engine's host twin (tests/hostmath/mc_pair_host.cpp, csrc/mht_mc_pair.h compiled for the CPU) against the NumPy
reference tests/mc_pair_ref.py, which is built on tests/mc_ref.py's own particles and states the borderline rule every comparison of
counts uses; against the own-ship engine's twin, particle for particle; against the Gaussian rule; and pymht_amd.evaluation's host
side (mc_pair_screen, every ValueError of mc_pair_encounters, the derived figures) without a device.

The scenes are mc_ref.scene_a() (70 models/pv targets, entries 5 and 9 NaN) and scene_c() (its constant-turn lift), all 2 415 pairs,
R = 80, K = 7, seed 12345, S = 4096.  Read from the reference's paths when written: no borderline pair-particle-step in either scene
(steps and segments), so the twin's counts are expected to EQUAL the reference's; 1 763 pairs (A) and 1 644 (C) have ever > 0, 1 761 and
1 642 have 0 < ever < S, and 137 pairs touch a NaN target.

Against the Gaussian rule (scene A): |within / S - pck| <= 4.5 sqrt(max(pck (1 - pck), 1 / S) / S) in every cell with
1e-3 < pck < 0.999, pck from encounter_ref.encounters.  The seed is fixed, so this is a deterministic statement about this draw: read
from the reference's paths, 4 150 such cells with a largest ratio of 3.93, and 4.5 is the margin over that -- a ratio far above it means
the sampler is wrong.  Cells below 1e-3 are in the Poisson regime (the largest ratio there is 6.5, a count of 11 where 1.9 are
expected): printed, not held."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import encounter_ref as eref
import mc_pair_ref as pref
import mc_ref as ref

NAN_PAIRS = 137


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return pref.build_twin(tmp_path_factory.mktemp("mc_pair_twin"))


@pytest.fixture(scope="module")
def own_twin(tmp_path_factory):
    return ref.build_twin(tmp_path_factory.mktemp("mc_twin_for_pairs"))


@pytest.fixture(scope="module")
def scenes(twin):
    """Scenes A and C, all pairs, S = 4096: (scene, pairs, the twin's counts, the reference's), computed once (tens of seconds)"""
    out = {}
    for name, sc in (("a", ref.scene_a()), ("c", ref.scene_c())):
        pairs = pref.all_pairs(len(sc["x"]))
        out[name] = (sc, pairs, pref.call_twin(twin, sc, pairs), pref.encounters(sc, pairs, name))
    return out


def _pv():
    from pymht_amd.models import pv
    return pv, *eref.model_matrices(pv, ref.DT)


@pytest.mark.parametrize("name", ["a", "c"])
def test_twin_equals_the_reference_on_all_pairs(scenes, name):
    sc, pairs, got, want = scenes[name]
    assert len(pairs) == 2415
    differ = pref.hold_counts("scene %s" % name.upper(), got, want)
    live = int((got["ever"] > 0).sum()), int(((got["ever"] > 0) & (got["ever"] < sc["S"])).sum())
    print("scene %s: %d borderline pair-particle-steps of %d, %d cells differ; ever > 0 in %d pairs, 0 < ever < S in %d"
          % (name.upper(), want["border"], want["steps"], differ, live[0], live[1]))
    assert want["border"] == 0 and differ == 0 and not any((got[k] == pref.SENTINEL).any() for k in ("within", "firstAt", "ever", "valid"))
    assert live == ((1763, 1761) if name == "a" else (1644, 1642))
    pref.check_invariants(got)
    pref.check_invariants(want)
    touched = np.isin(pairs, [eref.NAN_X, eref.NAN_P]).any(axis=1)
    assert int(touched.sum()) == NAN_PAIRS and np.array_equal(got["status"] == 1, touched) and (got["status"][~touched] == 0).all()
    assert (got["valid"][touched] == 0).all() and (got["valid"][~touched] == sc["S"]).all()
    assert not got["within"][:, touched].any() and not got["firstAt"][:, touched].any() and not got["ever"][touched].any()
    assert int((got["firstAt"][1:] > 0).sum()) > 1000, "no pair comes inside after the first step: firstAt is not exercised"


@pytest.mark.parametrize("name", ["a", "c"])
def test_a_particle_is_the_own_ship_engines_particle(twin, own_twin, name):
    """Particle p of target t in the pair twin against mc_path_host's walk from the same X_0, bit for bit: four states (scene A), six
    (scene C, constant turn), and six states walked linearly."""
    sc = dict(ref.scene_a() if name == "a" else ref.scene_c(), S=64)
    N = sc["x"].shape[1]
    cases = [(sc, 1 if sc["ct"] else 0)]
    if name == "c":
        from pymht_amd.models import ct
        cases.append((dict(sc, ct=False, Phi=np.asarray(ct.Phi(ref.DT, 0.0), dtype=np.float64)), 0))
    for case, transition in cases:
        Phi, Q = np.ascontiguousarray(case["Phi"]), np.ascontiguousarray(case["Q"])
        for a, b, p in ((0, 12, 0), (12, 0, 5), (69, 3, 63), (20, 21, 4000), (33, 34, (1 << 20) - 1)):
            got = pref.twin_path(twin, case, a, b, p)
            for side, t in enumerate((a, b)):
                out = np.zeros((case["K"] + 1, N))
                x0 = np.ascontiguousarray(got["states"][0, side])
                assert own_twin.mc_path_host(N, transition, case["K"], case["dt"], Phi.ctypes.data, Q.ctypes.data, x0.ctypes.data, case["seed"], p, t,
                                             out.ctypes.data) == 0
                assert out.tobytes() == np.ascontiguousarray(got["states"][:, side]).tobytes(), (a, b, p, side)
            d = got["states"][:, 0, :2] - got["states"][:, 1, :2]
            assert d.tobytes() == got["rel"].tobytes()
            assert np.array_equal(got["inside"], (d * d).sum(axis=1) < case["R"] ** 2) and got["came"] == bool(got["first"].any()) and got["first"].sum() <= 1
    # X_0 itself: the reference's particle (mc_ref.encounters' draw), to the last bits of log, sin and cos
    _, paths = pref.target_paths(sc)
    got = pref.twin_path(twin, sc, 0, 12, 7)
    for side, t in enumerate((0, 12)):
        want = paths[t][:, :, 7]
        assert np.abs(got["states"][:, side, :2] - want).max() <= 1e-9 * max(1.0, np.abs(want).max())


def test_both_orders_a_duplicate_and_a_pair_alone(scenes, twin):
    for name in ("a", "c"):
        sc, pairs, whole, _ = scenes[name]
        live = np.flatnonzero((whole["ever"] > 0) & (whole["ever"] < sc["S"]))
        pick = np.array([live[0], live[7], live[len(live) // 2], live[-1], 2414, 4])      # (pair 4 is (0, 5): a NaN target; 2414 is (68, 69))
        mixed = np.concatenate([pairs[pick], pairs[pick][:, ::-1], pairs[pick[:2]]])
        got = pref.call_twin(twin, sc, mixed)
        for k in pref.COUNTS:
            want = whole[k][..., pick]
            assert np.array_equal(got[k][..., :6], want) and np.array_equal(got[k][..., 6:12], want) and np.array_equal(got[k][..., 12:], want[..., :2]), (name, k)
        j = int(pick[2])
        alone = pref.call_twin(twin, sc, pairs[j:j + 1])
        assert all(np.array_equal(alone[k][..., 0], whole[k][..., j]) for k in pref.COUNTS) and alone["ever"][0] > 0
        assert got["status"].tolist()[:6] == [0, 0, 0, 0, 0, 1]


def test_a_passage_between_two_steps(twin):
    pv, Phi, _ = _pv()
    x = np.array([[-100.0, 10.0, 40.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    sc = ref.scene(x, np.zeros((2, 4, 4)), [0, 1, 2], [1.0, 1.0], Phi, np.zeros((4, 4)), np.zeros((1, 2, 2)), K=1, S=128)
    for pairs in ([[0, 1]], [[1, 0]]):
        got, want = pref.call_twin(twin, sc, pairs), pref.encounters(sc, pairs)
        assert pref.hold_counts("passage", got, want) == 0
        assert got["ever"].tolist() == [128] and not got["within"].any() and got["firstAt"].tolist() == [[0], [128]] and got["status"].tolist() == [0]


def test_scene_a_agrees_with_the_gaussian_rule(scenes):
    sc, pairs, got, _ = scenes["a"]
    pck = eref.encounters(sc["x"], sc["P"], sc["Phi"], sc["Q"], sc["K"], sc["dt"], sc["R"], pc_mp=False)["pck"][:, pairs[:, 0], pairs[:, 1]]      # [K + 1, n]
    S = float(sc["S"])
    finite = np.isfinite(pck)
    assert (got["status"][finite.any(axis=0)] == 0).all()
    with np.errstate(all="ignore"):
        ratio = np.abs(got["within"] / S - pck) / np.sqrt(np.fmax(pck * (1.0 - pck), 1.0 / S) / S)
    held = finite & (pck > 1e-3) & (pck < 0.999)
    rare = finite & (pck <= 1e-3)
    print("%d informative cells, largest ratio %.2f; below 1e-3 (Poisson regime, not held): largest ratio %.2f"
          % (int(held.sum()), float(ratio[held].max()), float(ratio[rare].max())))
    assert int(held.sum()) >= 4000
    assert (ratio[held] <= 4.5).all(), float(ratio[held].max())


def test_the_split_is_the_own_ship_engines(twin):
    out = np.zeros(2, dtype=np.int32)
    for nPair, S in ((1, 64), (1, 320), (1, 65536), (4, 320), (64, 4096), (2415, 1024), (1030, 256), (124750, 4096), (1 << 20, 1 << 20)):
        twin.mc_pair_chunks_host(nPair, S, out.ctypes.data)
        chunks, slab = int(out[0]), int(out[1])
        assert (chunks, slab) == ref.chunks(nPair, S)
        assert slab % 256 == 0 and (chunks - 1) * slab < S <= chunks * slab and (nPair >= 1024) <= (chunks == 1)
    assert ref.chunks(2415, 1024) == (1, 1024) and ref.chunks(64, 4096) == (16, 256) and ref.chunks(4, 320) == (2, 256) and ref.chunks(1, 65536) == (256, 256)


def _loop_screen(mean, ok, horizon, distance):
    keep = []
    for a in range(len(mean)):
        for b in range(a + 1, len(mean)):
            if not (ok[a] and ok[b]):
                continue
            rx, ry, vx, vy = mean[a] - mean[b]
            rv, vv = rx * vx + ry * vy, vx * vx + vy * vy
            ts = min(max(-rv / vv, 0.0), horizon) if vv > 0 else 0.0
            cx, cy = rx + ts * vx, ry + ts * vy
            if cx * cx + cy * cy < distance * distance:
                keep.append((a, b))
    return np.array(keep, dtype=np.int64).reshape(-1, 2)


def test_screen_against_a_plain_double_loop():
    from pymht_amd import evaluation
    sc = ref.scene_a()
    x = sc["x"]
    ok = ~np.isnan(x[:, :4]).any(axis=1)
    assert not ok[eref.NAN_X]      # (entry 5 has its NaN in the last of its four states)
    for horizon, distance in ((35.0, 300.0), (0.0, 500.0), (600.0, 80.0)):
        got = evaluation.mc_pair_screen(x, np.arange(70), np.ones(70), horizon, distance, block=32)
        want = _loop_screen(x[:, :4], ok, horizon, distance)
        assert got.dtype == np.int64 and np.array_equal(got, want) and 0 < len(got) < 2415
        assert not (got == eref.NAN_X).any() and (got[:, 0] < got[:, 1]).all()
    # components: the weight-normalised mean, target VALUES, a component of weight 0 does not enter, a target of weight 0 is in no pair
    x2 = np.concatenate([x[:4, :4], x[:4, :4] + 10.0, [[np.nan] * 4]])
    tg, w = np.array([7, 3, 9, 11, 7, 3, 9, 11, 3]), np.array([1.0, 1.0, 1.0, 0.0, 3.0, 1.0, 1.0, 0.0, 0.0])
    mean = {7: x[0, :4] + 7.5, 3: x[1, :4] + 5.0, 9: x[2, :4] + 5.0}
    got = evaluation.mc_pair_screen(x2, tg, w, 35.0, 1e9)
    assert got.tolist() == [[3, 7], [3, 9], [7, 9]]
    order = [3, 7, 9]
    want = _loop_screen(np.array([mean[t] for t in order]), [True] * 3, 35.0, 900.0)
    assert np.array_equal(evaluation.mc_pair_screen(x2, tg, w, 35.0, 900.0), np.array(order)[want].reshape(-1, 2))
    assert evaluation.mc_pair_screen(np.zeros((0, 4)), np.zeros(0, dtype=np.int64), np.zeros(0), 10.0, 10.0).shape == (0, 2)
    for bad in (dict(x=np.zeros((9, 3))), dict(target=tg[:3]), dict(weight=-w), dict(horizon=-1.0), dict(distance=0.0), dict(distance=np.nan)):
        with pytest.raises(ValueError, match="mc_pair_screen"):
            evaluation.mc_pair_screen(**dict(dict(x=x2, target=tg, weight=w, horizon=35.0, distance=100.0), **bad))
    assert "pre-filter" in evaluation.mc_pair_screen.__doc__.lower()


def test_every_value_error_is_raised_without_a_device(monkeypatch):
    from pymht_amd import evaluation

    def no_device(*a, **kw):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(evaluation, "Context", no_device)
    pv, Phi, Q = _pv()
    x, P = np.zeros((3, 4)), np.tile(np.eye(4), (3, 1, 1))
    good = dict(x=x, P=P, target=[4, 4, 9], weight=[1.0, 2.0, 1.0], Phi=Phi, Q=Q, steps=4, dt=5.0, radius=50.0, pairs=[[4, 9]])
    bad = [dict(x=np.zeros((3, 5))), dict(P=P[:2]), dict(Phi=np.eye(6)), dict(Q=np.full((4, 4), np.nan)), dict(steps=0), dict(steps=65), dict(steps=2.0),
           dict(dt=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(particles=100), dict(particles=32), dict(particles=(1 << 20) + 64), dict(particles=64.0),
           dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5), dict(transition="ct"), dict(transition="arc"), dict(target=[0, 0]), dict(target=[0.0, 0.0, 1.0]),
           dict(weight=[1.0, 2.0]), dict(weight=[1.0, -2.0, 1.0]), dict(weight=[0.0, 0.0, 1.0]), dict(weight=[1.0, np.inf, 1.0]), dict(weight=[1.0, np.nan, 1.0]),
           dict(pairs=[[4, 9, 4]]), dict(pairs=[4, 9]), dict(pairs=[[4.0, 9.0]]), dict(pairs=[[4, 4]]), dict(pairs=[[4, 9], [9, 9]]), dict(pairs=[[4, 5]]),
           dict(pairs=[[0, 1]]), dict(pairs=[[4, 9], [10, 4]]), dict(pairs=[[-1, 4]]), dict(pairs=np.zeros(((1 << 20) + 1, 2), dtype=np.int32))]
    for change in bad:
        with pytest.raises(ValueError, match="mc_pair_encounters"):
            evaluation.mc_pair_encounters(**dict(good, **change))
    with pytest.raises(ValueError, match="target 5"):
        evaluation.mc_pair_encounters(**dict(good, pairs=[[9, 4], [4, 5]]))
    with pytest.raises(ValueError, match="twice"):
        evaluation.mc_pair_encounters(**dict(good, pairs=[[9, 9]]))
    # no pair, or no component: empty arrays and no device call
    for none in (evaluation.mc_pair_encounters(**dict(good, pairs=np.zeros((0, 2), dtype=np.int64))), evaluation.mc_pair_encounters(**dict(good, pairs=[])),
                 evaluation.mc_pair_encounters(np.zeros((0, 4)), np.zeros((0, 4, 4)), np.zeros(0, dtype=np.int64), np.zeros(0), Phi, Q, 4, 5.0, 50.0, [])):
        assert none["within"].shape == (5, 0) and none["firstAt"].shape == (5, 0) and none["pEverBy"].shape == (5, 0) and none["pc"].shape == (5, 0)
        assert all(none[k].shape == (0,) for k in ("ever", "valid", "status", "pEver", "pcMax", "tpc", "sePEver", "sePcMax")) and none["pairs"].shape == (0, 2)
        assert none["within"].dtype == np.uint32 and none["status"].dtype == np.int32
    with pytest.raises(ValueError, match="mc_pair_encounters"):
        evaluation.mc_pair_encounters(np.zeros((0, 4)), np.zeros((0, 4, 4)), np.zeros(0, dtype=np.int64), np.zeros(0), Phi, Q, 4, 5.0, 50.0, [[0, 1]])
    assert evaluation.MC_MAX_PAIRS == pref.MAX_PAIRS == 1 << 20


def test_the_hosts_figures():
    """mc_derive's rules on a pair's counts, pEverBy = cumsum(firstAt) / valid with its last row pEver, NaN where valid is 0"""
    from pymht_amd import evaluation
    within = np.array([[0, 10], [32, 10], [32, 10], [5, 10]], dtype=np.uint32)        # [4, 2]
    first_at = np.array([[0, 0], [32, 0], [0, 0], [8, 0]], dtype=np.uint32)
    ever, valid = np.array([40, 0], dtype=np.uint32), np.array([64, 0], dtype=np.uint32)
    d = evaluation.mc_pair_derive(within, first_at, ever, valid, 2.5)
    assert d["pc"][:, 0].tolist() == [0.0, 0.5, 0.5, 5 / 64] and np.isnan(d["pc"][:, 1]).all()
    assert d["pcMax"][0] == 0.5 and d["tpc"][0] == 2.5 and np.isnan(d["pcMax"][1]) and np.isnan(d["tpc"][1])
    assert d["pEver"][0] == 40 / 64 and d["sePcMax"][0] == np.sqrt(0.25 / 64) and d["sePEver"][0] == np.sqrt((40 / 64) * (24 / 64) / 64)
    assert d["pEverBy"][:, 0].tolist() == [0.0, 0.5, 0.5, 40 / 64] and d["pEverBy"][-1, 0] == d["pEver"][0]
    assert all(np.isnan(d[k][..., 1]).all() for k in ("pc", "pcMax", "tpc", "pEver", "sePcMax", "sePEver", "pEverBy"))
    assert all(d[k].shape == (2,) for k in ("pcMax", "tpc", "pEver", "sePcMax", "sePEver")) and d["pc"].shape == (4, 2) and d["pEverBy"].shape == (4, 2)


def test_the_twin_on_its_own_under_a_sanitizer(tmp_path):
    """tests/hostmath/mc_pair_host_main.cpp: a program of its own (nothing of it is loaded into Python, nothing is preloaded), built with
    -fsanitize=address,undefined and run as a child process on dumped scenes A and C at S = 256; it prints the reference's counts."""
    gxx = shutil.which("g++") or "g++"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mc_pair_host_main")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # (the runtimes in the program itself: it needs nothing from its environment)
                           os.path.join(root, "tests", "hostmath", "mc_pair_host_main.cpp"), "-o", exe])
    files, wants = [], []
    for name, base in (("a", ref.scene_a()), ("c", ref.scene_c())):
        sc = dict(base, S=256)
        pairs = pref.all_pairs(len(sc["x"]))
        files.append(str(tmp_path / ("scene_%s.bin" % name)))
        pref.dump(sc, pairs, files[-1])
        want = pref.encounters(sc, pairs)
        assert want["border"] == 0
        wants.append("%s: within %d firstAt %d ever %d valid %d" % (files[-1], want["within"].sum(dtype=np.int64), want["firstAt"].sum(dtype=np.int64),
                                                                   want["ever"].sum(dtype=np.int64), want["valid"].sum(dtype=np.int64)))
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.strip().splitlines() == wants, (run.stdout, wants)
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    short = str(tmp_path / "short.bin")
    with open(files[0], "rb") as fh, open(short, "wb") as out:
        out.write(fh.read()[:-8])
    assert subprocess.run([exe, short], capture_output=True).returncode == 1
