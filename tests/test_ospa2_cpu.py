"""CPU: OSPA(2) of a window (csrc/mht_ospa2.h: the base distance and ospa2_window, what the kernels of mht_ospa2.hip run) compiled for
the host (tests/hostmath/ospa2_host.cpp, the 64 lanes of a sweep as a loop) and held to the criterion of tests/ospa2_ref.py: the issue's
two known answers, the brute force over all partial assignments on tiny windows, the SciPy reference on tracker-like scenes and on the
member counts tests/test_ospa2_gpu.py runs; and what is host-only in pymht_amd.evaluation.ospa2_windows and Tracker.getOspa2: the
refusals that need no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import gospa_ref
import ospa2_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    so = str(tmp_path_factory.mktemp("ospa2_host") / "libospa2_host.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "ospa2_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.ospa2_window_host.restype = C.c_int
    lib.ospa2_window_host.argtypes = ([C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_double, C.c_int32] + [C.c_void_p] * 4)
    lib.ospa2_base_host.restype = C.c_double
    lib.ospa2_base_host.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_double]
    return lib


def packed(run):
    trkXY, trkOn, truXY, truOn = run
    K = len(trkOn)
    return (np.ascontiguousarray(np.asarray(trkXY, dtype=np.float64).reshape(K, -1, 2)), np.ascontiguousarray(np.asarray(trkOn, dtype=np.uint8).reshape(K, -1)),
            np.ascontiguousarray(np.asarray(truXY, dtype=np.float64).reshape(K, -1, 2)), np.ascontiguousarray(np.asarray(truOn, dtype=np.uint8).reshape(K, -1)))


def host_window(lib, run, lo, hi, c, p=2):
    """((total, loc, nAssigned, n_w, m_w, match), sweeps) of one window from the host twin; every output cell is written and the cell
    behind the matches is not."""
    trkXY, trkOn, truXY, truOn = packed(run)
    n = trkOn.shape[1]
    win, count = np.full(2, float(SENTINEL)), np.full(3, SENTINEL, dtype=np.int32)
    match, sweeps = np.full(n + 1, SENTINEL, dtype=np.int32), np.full(1, SENTINEL, dtype=np.int32)
    rc = lib.ospa2_window_host(len(trkOn), n, trkXY.ctypes.data, trkOn.ctypes.data, truOn.shape[1], truXY.ctypes.data, truOn.ctypes.data, lo, hi, c, p,
                               win.ctypes.data, count.ctypes.data, match.ctypes.data, sweeps.ctypes.data)
    assert rc == 0
    assert match[-1] == SENTINEL and not (match[:-1] == SENTINEL).any() and not (count == SENTINEL).any() and not (win == SENTINEL).any()
    return (win[0], win[1], count[0], count[1], count[2], match[:-1]), int(sweeps[0])


def same_bits(a, b):
    return (np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes()
            and tuple(int(v) for v in a[2:5]) == tuple(int(v) for v in b[2:5]) and np.array_equal(a[5], b[5]))


def test_known_answer_a_split_track_costs_what_per_scan_gospa_cannot_see(twin):
    """One truth over 20 steps, two exact half-length tracks, whole-run window, c = 10: one fragment is assigned at D = c / 2, the other
    pays the cut-off.  Per-scan GOSPA of the same data is 0 at every scan."""
    run = ref.split_track()
    got, _ = host_window(twin, run, 0, 19, 10.0, 1)
    assert got[:5] == (15.0, 5.0, 1, 2, 1) and sorted(got[5].tolist()) == [-1, 0]
    ref.hold(got, ref.reference(*run, 0, 19, 10.0, 1), 20, "split track p 1", match=False)
    got, _ = host_window(twin, run, 0, 19, 10.0, 2)
    assert got[:5] == (125.0, 25.0, 1, 2, 1)
    ref.hold(got, ref.reference(*run, 0, 19, 10.0, 2), 20, "split track p 2", match=False)
    for t in range(20):
        on = run[1][t] != 0
        assert float(gospa_ref.reference(run[0][t][on], run[2][t], 10.0)["total"]) == 0.0
    one = (run[2], run[3], run[2], run[3])      # the unbroken track
    assert host_window(twin, one, 0, 19, 10.0)[0][:5] == (0.0, 0.0, 1, 1, 1)


def test_known_answer_a_window_of_one_step_with_equal_counts_is_gospa(twin):
    """W = 1 and n_w = m_w: the objective is GOSPA's (alpha = 2); total and nAssigned agree with gospa_ref.reference, 50 random sets."""
    rng = np.random.default_rng(4)
    for k in range(50):
        n = int(rng.integers(1, 9))
        run = ref.random_run(rng, n, n, 1, field=25.0, p_on=1.0)
        for p in (1, 2):
            got, _ = host_window(twin, run, 0, 0, 8.0, p)
            want = gospa_ref.reference(run[0][0], run[2][0], 8.0, p)
            assert got[2] == want["nAssigned"] and got[3] == got[4] == n
            assert abs(np.longdouble(got[0]) - want["total"]) <= (want["nAssigned"] + 2 + 14) * ref.EPS * want["total"]
            ref.hold(got, ref.reference(*run, 0, 0, 8.0, p), 1)


def test_twin_against_the_brute_force_on_tiny_windows(twin):
    """200 random runs of 0 .. 5 objects a side over 1 .. 4 steps with random flags, one random window each, c in {5, 12, 100}, both p:
    the total is the minimum over ALL partial assignments, and the window meets the reference's criterion."""
    rng = np.random.default_rng(0)
    for _ in range(200):
        n, m, K = int(rng.integers(0, 6)), int(rng.integers(0, 6)), int(rng.integers(1, 5))
        run = ref.random_run(rng, n, m, K)
        lo = int(rng.integers(0, K))
        hi = int(rng.integers(lo, K))
        for c in (5.0, 12.0, 100.0):
            for p in (1, 2):
                got, _ = host_window(twin, run, lo, hi, c, p)
                want = ref.reference(*run, lo, hi, c, p)
                best = ref.brute(*run, lo, hi, c, p)
                assert abs(got[0] - best) <= 2 * ref.bounds(want, hi - lo + 1)[1], (n, m, K, lo, hi, c, p, got, best)
                ref.hold(got, want, hi - lo + 1, match=False)


@pytest.mark.parametrize("T", [5, 30, 64])
def test_twin_against_the_reference_on_tracker_like_scenes(twin, T):
    run = ref.tracker_scene(T, seed=T)
    biggest = 0.0
    for W in (1, 5, 16):
        for lo, hi in ref.sliding(ref.K_SCENE, W, every=3) + [(ref.K_SCENE - W, ref.K_SCENE - 1)]:
            for p in (1, 2):
                want = ref.reference(*run, lo, hi, ref.C_SCENE, p)
                got, sweeps = host_window(twin, run, lo, hi, ref.C_SCENE, p)
                ref.hold(got, want, hi - lo + 1, "T %d window [%d, %d] p %d, %d sweeps" % (T, lo, hi, p, sweeps))
                assert sweeps <= min(got[3], got[4]) * (max(got[3], got[4]) + 2)      # (the loop bounds, summed)
                if want["edge"].any():
                    biggest = max(biggest, float(want["D"][want["edge"]].max()))
    print("largest base distance of an edge: %.4f c" % (biggest / ref.C_SCENE))
    whole = host_window(twin, run, 0, ref.K_SCENE - 1, ref.C_SCENE)[0]
    assert whole[2] < whole[3] and whole[2] <= whole[4]      # (fragments and false tracks: more tracks than can be assigned)


@pytest.mark.parametrize("p", [1, 2])
def test_twin_on_the_member_counts_of_the_gpu_tests(twin, p):
    for label, run, c in ref.shape_runs():
        for lo, hi in ((0, 4), (2, 2), (0, 0)):
            got, _ = host_window(twin, run, lo, hi, c, p)
            ref.hold(got, ref.reference(*run, lo, hi, c, p), hi - lo + 1, "%s [%d, %d] p %d" % (label, lo, hi, p))


def test_empty_windows_and_one_sided_windows(twin):
    rng = np.random.default_rng(6)
    run = list(ref.random_run(rng, 4, 3, 6))
    run[1][2:4] = 0
    run[3][2:4] = 0
    run[0], run[2] = ref.poison(run[0], run[1]), ref.poison(run[2], run[3])
    got, sweeps = host_window(twin, run, 2, 3, 10.0)      # nobody is present
    assert got[:5] == (0.0, 0.0, 0, 0, 0) and got[5].tolist() == [-2] * 4 and sweeps == 0
    run[1][3, 1] = run[1][3, 3] = 1      # tracks only
    run[0][3] = 5.0
    for p in (1, 2):
        got, _ = host_window(twin, run, 2, 3, 10.0, p)
        assert got[:5] == (2 * 10.0 ** p, 0.0, 0, 2, 0) and got[5].tolist() == [-2, -1, -2, -1]
        ref.hold(got, ref.reference(*run, 2, 3, 10.0, p), 2)
    swapped = (run[2], run[3], run[0], run[1])      # truths only
    got, _ = host_window(twin, swapped, 2, 3, 10.0)
    assert got[:5] == (200.0, 0.0, 0, 0, 2) and got[5].tolist() == [-2] * 3


def test_a_pair_that_is_never_near_has_the_cutoff_bit_for_bit(twin):
    """c = 0.1 * 3 is not representable: (c nFar + 0) / U would round away from c; D is c itself.  The pair is unassigned."""
    c = 0.1 * 3
    K = 7
    trkXY, truXY = np.zeros((K, 1, 2)), np.full((K, 1, 2), 1.0)
    trkOn, truOn = np.ones((K, 1), dtype=np.uint8), np.ones((K, 1), dtype=np.uint8)
    truOn[5] = 0
    D = twin.ospa2_base_host(1, trkXY.ctypes.data, trkOn.ctypes.data, 0, 1, truXY.ctypes.data, truOn.ctypes.data, 0, 0, K - 1, c)
    assert np.float64(D).tobytes() == np.float64(c).tobytes()
    got, _ = host_window(twin, (trkXY, trkOn, truXY, truOn), 0, K - 1, c, 1)
    assert got[:5] == (c, 0.0, 0, 1, 1) and got[5].tolist() == [-1]
    truXY[3] = 0.125      # one near step out of seven
    D = twin.ospa2_base_host(1, trkXY.ctypes.data, trkOn.ctypes.data, 0, 1, truXY.ctypes.data, truOn.ctypes.data, 0, 0, K - 1, c)
    assert D == (c * 6.0 + np.sqrt(0.03125)) / 7.0 and D < c
    got, _ = host_window(twin, (trkXY, trkOn, truXY, truOn), 0, K - 1, c, 1)
    assert got[:5] == (D, D, 1, 1, 1) and got[5].tolist() == [0]


def test_swapping_the_roles_gives_the_same_total(twin):
    for T in (5, 30):
        run = ref.tracker_scene(T, seed=100 + T)
        swapped = (run[2], run[3], run[0], run[1])
        for lo, hi in ((0, 15), (3, 7), (9, 9)):
            for p in (1, 2):
                a, _ = host_window(twin, run, lo, hi, ref.C_SCENE, p)
                b, _ = host_window(twin, swapped, lo, hi, ref.C_SCENE, p)
                want = ref.reference(*run, lo, hi, ref.C_SCENE, p)
                ref.hold(a, want, hi - lo + 1)
                assert abs(np.longdouble(b[0]) - want["total"]) <= ref.bounds(want, hi - lo + 1)[1]
                assert (b[2], b[3], b[4]) == (a[2], a[4], a[3])


def test_a_perfect_run_scores_zero_and_poison_changes_nothing(twin):
    run = ref.tracker_scene(30, seed=9)
    perfect = (run[2], run[3], run[2], run[3])
    for lo, hi in ((0, 15), (4, 8), (15, 15)):
        got, _ = host_window(twin, perfect, lo, hi, ref.C_SCENE)
        assert got[0] == 0.0 and got[1] == 0.0 and got[2] == got[3] == got[4]
    # the same run with finite numbers where the flags are 0: the same bits
    rng = np.random.default_rng(1)
    filled = (np.where(np.isnan(run[0]), rng.uniform(-1e3, 1e3, size=run[0].shape), run[0]), run[1],
              np.where(np.isnan(run[2]), rng.uniform(-1e3, 1e3, size=run[2].shape), run[2]), run[3])
    assert np.isnan(run[0]).any() and np.isnan(run[2]).any() and not np.isnan(filled[0]).any()
    for lo, hi in ((0, 15), (4, 8), (15, 15), (0, 0)):
        for p in (1, 2):
            assert same_bits(host_window(twin, run, lo, hi, ref.C_SCENE, p)[0], host_window(twin, filled, lo, hi, ref.C_SCENE, p)[0])


def test_twin_refusals(twin):
    run = packed(ref.random_run(np.random.default_rng(2), 2, 2, 3))
    out = np.zeros(8)

    def call(n_steps=3, lo=0, hi=2, c=5.0, p=2, n=2):
        return twin.ospa2_window_host(n_steps, n, run[0].ctypes.data, run[1].ctypes.data, 2, run[2].ctypes.data, run[3].ctypes.data, lo, hi, c, p,
                                      *[out.ctypes.data] * 4)
    for c, p in ((0.0, 2), (-1.0, 2), (np.inf, 2), (np.nan, 1), (1e200, 2), (5.0, 0), (5.0, 3)):
        assert call(c=c, p=p) == -1
    assert call(lo=-1) == -1 and call(hi=3) == -1 and call(lo=2, hi=1) == -1
    assert call(n=2049) == -3
    assert call() == 0


def test_reference_is_self_consistent():
    """tests/ospa2_ref.py alone: SciPy's total is the brute force's; total = loc + c^p (N - nAssigned); np.longdouble is wider."""
    assert np.finfo(np.longdouble).eps < 1e-18
    rng = np.random.default_rng(1)
    for _ in range(60):
        n, m, K = int(rng.integers(0, 6)), int(rng.integers(0, 6)), int(rng.integers(1, 5))
        run = ref.random_run(rng, n, m, K)
        for c, p in ((5.0, 1), (12.0, 2), (100.0, 2)):
            w = ref.reference(*run, 0, K - 1, c, p)
            assert abs(float(w["total"]) - ref.brute(*run, 0, K - 1, c, p)) <= 1e-12 * max(1.0, float(w["total"]))
            assert w["total"] == w["loc"] + np.longdouble(c) ** p * (max(w["nTracks"], w["nTruths"]) - w["nAssigned"])
            assert (w["match"] >= 0).sum() == w["nAssigned"] and (w["match"] > -2).sum() == w["nTracks"]
    assert ref.sliding(7, 3, 3) == [(0, 0), (1, 3), (4, 6)] and ref.sliding(3, 5) == [(0, 0), (0, 1), (0, 2)]


def test_refusals_that_need_no_gpu():
    from pymht_amd.evaluation import ospa2_windows
    rng = np.random.default_rng(3)
    trkXY, trkOn, truXY, truOn = ref.random_run(rng, 3, 2, 4)
    good = dict(trackXY=trkXY, trackOn=trkOn, truthXY=truXY, truthOn=truOn, c=10.0)

    def refused(match, **over):
        with pytest.raises(ValueError, match=match):
            ospa2_windows(**dict(good, **over))
    refused("trackXY", trackXY=trkXY[:, :, 0])
    refused("trackXY", trackXY=trkXY[:3])
    refused("truthOn", truthOn=truOn[:, :1])
    refused("truthXY", truthXY=np.zeros((4, 2, 3)))
    refused("flags", trackOn=trkOn.astype(np.float64))
    refused("flags", truthOn=truOn.astype(object))
    for c in (0.0, -1.0, np.inf, np.nan, None, "10", True, 1e200):
        refused("c", c=c)
    for p in (0, 3, 1.5, None, True):
        refused("p must", p=p)
    refused("exclusive", window=2, windows=[(0, 1)])
    for w in (0, -1, 1.5, True):
        refused("window", window=w)
    for e in (0, -2, 1.5):
        refused("every", window=2, every=e)
    for wins in ([(-1, 2)], [(0, 4)], [(2, 1)], [(0, 1, 2)], [0, 1]):
        refused("window", windows=wins)
    bad = trkXY.copy()
    bad[np.flatnonzero(trkOn[:, 0])[0], 0, 1] = np.inf
    refused("finite", trackXY=bad)
    bad = truXY.copy()
    bad[np.flatnonzero(truOn[:, 1])[0], 1, 0] = np.nan
    refused("finite", truthXY=bad)
    refused("2048", trackXY=np.zeros((4, 2049, 2)), trackOn=np.ones((4, 2049), dtype=np.uint8))
    refused("maxWorkBytes", maxWorkBytes=64)
    out = ospa2_windows(**dict(good, windows=[]))      # (no windows: nothing to launch, no device needed)
    assert out["match"].shape == (0, 3) and out["windows"].shape == (0, 2) and out["nAssigned"].dtype == np.int32
    assert all(len(out[k]) == 0 for k in ("ospa2", "total", "localisation", "cardinality", "nAssigned", "nTracks", "nTruths"))
    empty = ospa2_windows(np.zeros((0, 3, 2)), np.zeros((0, 3), dtype=bool), np.zeros((0, 2, 2)), np.zeros((0, 2), dtype=bool), 10.0)
    assert len(empty["total"]) == 0      # (no steps: the whole-run window does not exist)


def test_get_ospa2_is_declared_with_its_switches_off():
    import inspect
    from pymht_amd.tracker import Tracker
    p = inspect.signature(Tracker.getOspa2).parameters
    assert p["p"].default == 2 and p["window"].default is None and p["every"].default == 1 and p["terminated"].default is True
    assert p["smooth"].default is False and p["constantTurn"].default is False and p["ais"].default is False and p["truthIds"].default is None
    doc = " ".join(Tracker.getOspa2.__doc__.lower().split())
    assert "as they stand at the call" in doc and "gospa" in doc


def test_truth_trajectories_from_rows_and_from_identities():
    from pymht_amd.evaluation import truth_trajectories
    a, b = np.array([[1.0, 2.0, 9.0], [np.nan, np.nan, 0.0]]), np.array([[3.0, 4.0, 9.0], [5.0, 6.0, 9.0]])
    XY, on = truth_trajectories([a, b])
    assert XY.shape == (2, 2, 2) and on.tolist() == [[1, 0], [1, 1]] and XY[1].tolist() == [[3.0, 4.0], [5.0, 6.0]]
    with pytest.raises(ValueError, match="rows"):
        truth_trajectories([a, b[:1]])
    XY, on = truth_trajectories([a[:1], b], truthIds=[["x"], ["y", "x"]])
    assert on.tolist() == [[1, 0], [1, 1]] and XY[1].tolist() == [[5.0, 6.0], [3.0, 4.0]] and XY[0, 0].tolist() == [1.0, 2.0]
    with pytest.raises(ValueError, match="identit"):
        truth_trajectories([a, b], truthIds=[["x"], ["y", "x"]])
    with pytest.raises(ValueError, match="twice"):
        truth_trajectories([b], truthIds=[["x", "x"]])
