"""CPU: the GOSPA search (csrc/mht_gospa.h: gospa_step, what the wavefront of gospa_kernel runs for its step) compiled for the host
(tests/hostmath/gospa_host.cpp, the 64 lanes of a sweep as a loop) and held to the criterion of tests/gospa_ref.py: against the brute
force over all partial assignments on small sets, against the SciPy reference on the shapes tests/test_gospa_gpu.py runs, the sweep
counts of the sparse scenes (the cut-off-tie pathology of a padded square problem must not come back); and what is host-only in
pymht_amd.evaluation: id_switches, the truth's two forms, and the refusals that need no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import gospa_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    so = str(tmp_path_factory.mktemp("gospa_host") / "libgospa_host.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "gospa_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.gospa_step_host.restype = C.c_int
    lib.gospa_step_host.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_int32] + [C.c_void_p] * 4
    lib.gospa_table_bytes_host.restype = C.c_uint64
    lib.gospa_table_bytes_host.argtypes = [C.c_int32, C.c_int32]
    return lib


def host_step(lib, X, Y, c, p=2):
    """((total, loc, nAssigned, nMissed, nFalse, match), sweeps) of one step from the host twin; every output cell is written and the
    cell behind the matches is not."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(-1, 2))
    Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1, 2))
    step, count = np.full(2, float(SENTINEL)), np.full(3, SENTINEL, dtype=np.int32)
    match, sweeps = np.full(len(X) + 1, SENTINEL, dtype=np.int32), np.full(1, SENTINEL, dtype=np.int32)
    rc = lib.gospa_step_host(len(X), X.ctypes.data, len(Y), Y.ctypes.data, c, p, step.ctypes.data, count.ctypes.data, match.ctypes.data,
                             sweeps.ctypes.data)
    assert rc == 0
    assert match[-1] == SENTINEL and not (match[:-1] == SENTINEL).any() and not (count == SENTINEL).any() and not (step == SENTINEL).any()
    return (step[0], step[1], count[0], count[1], count[2], match[:-1]), int(sweeps[0])


def test_twin_against_the_brute_force_on_small_sets(twin):
    """300 random sets of 0 .. 5 objects a side on a 30 x 30 field, c in {5, 12, 100}, both p: the total is the minimum over ALL partial
    assignments (the brute force sums in another order: (k + 10) eps64 on both sides), and the step meets the reference's criterion."""
    rng = np.random.default_rng(0)
    for _ in range(300):
        n, m = rng.integers(0, 6, size=2)
        X, Y = ref.random_sets(rng, n, m)
        for c in (5.0, 12.0, 100.0):
            for p in (1, 2):
                got, _ = host_step(twin, X, Y, c, p)
                best = ref.brute(X, Y, c, p)
                assert abs(got[0] - best) <= 2 * (got[2] + 10) * ref.EPS * best, (n, m, c, p, got, best)
                ref.hold(got, ref.reference(X, Y, c, p))


@pytest.mark.parametrize("p", [1, 2])
def test_twin_against_the_reference_on_the_shapes_of_the_gpu_tests(twin, p):
    for label, X, Y, c in ref.shape_cases():
        got, sweeps = host_step(twin, X, Y, c, p)
        ref.hold(got, ref.reference(X, Y, c, p), "%s p %d, %d sweeps" % (label, p, sweeps))
        assert sweeps <= min(len(X), len(Y)) * (max(len(X), len(Y)) + 1)      # (the loop bounds, summed)
    X, Y = ref.dense_scene()
    got, sweeps = host_step(twin, X, Y, ref.C_SCENE, p)
    ref.hold(got, ref.reference(X, Y, ref.C_SCENE, p), "dense 137x130 p %d, %d sweeps" % (p, sweeps))
    assert got[2] == 130      # (everybody inside one cut-off: every truth is assigned)


def test_greedy_traps_boundary_and_ties(twin):
    got, _ = host_step(twin, [(0, 0), (2, 0)], [(1.1, 0), (3.3, 0)], 10.0)
    ref.hold(got, ref.reference([(0, 0), (2, 0)], [(1.1, 0), (3.3, 0)], 10.0))
    assert abs(got[0] - 2.90) < 1e-12 and got[5].tolist() == [0, 1]      # (nearest pair first: 11.70)
    got, _ = host_step(twin, [(0, 0), (2, 0)], [(1.2, 0), (-1.5, 0)], 10.0)
    assert abs(got[0] - 2.89) < 1e-12 and got[5].tolist() == [1, 0]      # (row-order greedy: 13.69)
    got, _ = host_step(twin, [(0, 0)], [(3, 4)], 5.0)      # d == c: not assigned
    assert got[:5] == (25.0, 0.0, 0, 1, 1) and got[5].tolist() == [-1]
    got, _ = host_step(twin, [(0, 0)], [(3, 4)], 5.000001)
    assert got[:5] == (25.0, 25.0, 1, 0, 0) and got[5].tolist() == [0]
    for p, c, want in ((1, 5.0, (5.0, 0.0, 0, 1, 1)), (1, 5.000001, (5.0, 5.0, 1, 0, 0))):
        assert host_step(twin, [(0, 0)], [(3, 4)], c, p)[0][:5] == want
    # two estimates on one point and one truth: the match is not unique, the figures are
    got, _ = host_step(twin, [(1, 1), (1, 1)], [(2, 1)], 10.0)
    ref.hold(got, ref.reference([(1, 1), (1, 1)], [(2, 1)], 10.0), match=False)
    assert sorted(got[5].tolist()) == [-1, 0]
    # a coordinate that is not finite: its object is never assigned
    got, _ = host_step(twin, [(np.nan, 0), (0, 0), (np.inf, 1)], [(1, 0), (0, np.inf)], 10.0)
    assert got[:5] == (1.0 + 50.0 * 3, 1.0, 1, 1, 2) and got[5].tolist() == [-1, 0, -1]


def test_sparse_scenes_take_one_sweep_per_row(twin):
    """Tracker-like scenes of 64, 130 and 500 targets (gospa_ref.sparse_scene: cfg3's density, 10 % undetected, 10 % false estimates,
    sigma 2.5, c = 20): at most rows + 8 column sweeps.  A padded square problem needed 2 080 for 64 x 64.  Measured: 64, 131, 501."""
    for T in (64, 130, 500):
        X, Y = ref.sparse_scene(T, seed=T)
        got, sweeps = host_step(twin, X, Y, ref.C_SCENE)
        ref.hold(got, ref.reference(X, Y, ref.C_SCENE), "sparse scene of %d targets (%d x %d), %d sweeps" % (T, len(X), len(Y), sweeps))
        assert sweeps <= min(len(X), len(Y)) + 8, (T, sweeps)
        assert got[3] >= T // 10 and got[4] >= T // 10


def test_twin_refusals_and_table_size(twin):
    one = np.zeros((1, 2))
    out = np.zeros(4)
    for c, p in ((0.0, 2), (-1.0, 2), (np.inf, 2), (np.nan, 1), (1e200, 2), (1e-200, 2), (5.0, 0), (5.0, 3)):
        assert twin.gospa_step_host(1, one.ctypes.data, 1, one.ctypes.data, c, p, *[out.ctypes.data] * 4) == -1
    big = np.zeros((2049, 2))
    assert twin.gospa_step_host(2049, big.ctypes.data, 1, one.ctypes.data, 5.0, 2, *[out.ctypes.data] * 4) == -3
    assert twin.gospa_table_bytes_host(2048, 2048) == 56 * 1024 and twin.gospa_table_bytes_host(0, 0) == 0
    assert twin.gospa_table_bytes_host(1, 1) % 16 == 0 and twin.gospa_table_bytes_host(63, 65) % 16 == 0


def test_reference_is_self_consistent():
    """tests/gospa_ref.py alone: SciPy's total is the brute force's; total = loc + c^p / 2 (nMissed + nFalse); np.longdouble is wider."""
    assert np.finfo(np.longdouble).eps < 1e-18
    rng = np.random.default_rng(1)
    for _ in range(60):
        n, m = rng.integers(0, 6, size=2)
        X, Y = ref.random_sets(rng, n, m)
        for c, p in ((5.0, 1), (12.0, 2), (100.0, 2)):
            w = ref.reference(X, Y, c, p)
            assert abs(float(w["total"]) - ref.brute(X, Y, c, p)) <= 1e-12 * max(1.0, float(w["total"]))
            assert w["total"] == w["loc"] + np.longdouble(c) ** p / 2 * (w["nMissed"] + w["nFalse"])
            assert w["nAssigned"] + w["nMissed"] == m and w["nAssigned"] + w["nFalse"] == n and (w["match"] >= 0).sum() == w["nAssigned"]


def test_id_switches_on_a_hand_made_sequence():
    from pymht_amd.evaluation import id_switches
    # truth 0: track 7, 7, (lost), 9 -> one switch; truth 1: track 8, (lost), 8, 8 -> none; truth 2: 5 once -> none; track 3 never assigned
    match = [np.array([0, 1, -1]), np.array([-1, 0]), np.array([1, 2]), np.array([0, 1])]
    ids = [[7, 8, 3], [8, 7], [8, 5], [9, 8]]
    total, per = id_switches(match, ids)
    assert total == 1 and per == {0: 1, 1: 0, 2: 0}
    # with truth identities: the rows of the truth change between steps, the identities do not
    total, per = id_switches([np.array([1]), np.array([0]), np.array([0])], [[4], [4], [6]], truthIds=[["a", "b"], ["b"], ["b", "a"]])
    assert total == 1 and per == {"b": 1}
    assert id_switches([], []) == (0, {})
    with pytest.raises(ValueError, match="per step"):
        id_switches([np.array([0])], [])
    with pytest.raises(ValueError, match="step 0"):
        id_switches([np.array([0, 1])], [[1]])


def test_truth_is_taken_in_both_forms():
    from pymht_amd.evaluation import truth_steps
    pos = [np.zeros((3, 4)), np.ones((2, 2))]
    for form in ((np.array([1.0, 3.5]), pos), ([1.0, 3.5], pos), [(1.0, pos[0]), (3.5, pos[1])], ((1.0, pos[0]), (3.5, pos[1]))):
        times, Y = truth_steps(form)
        assert times.tolist() == [1.0, 3.5] and Y[0] is pos[0] and Y[1] is pos[1]
    times, Y = truth_steps([(2.0, pos[1])])
    assert times.tolist() == [2.0] and Y[0] is pos[1]
    assert truth_steps([])[0].shape == (0,)
    with pytest.raises(ValueError, match="time"):
        truth_steps([(1.0, pos[0]), pos[1], (2.0, pos[1])])


def test_refusals_that_need_no_gpu():
    from pymht_amd.evaluation import gospa_steps
    a, b = np.zeros((2, 2)), np.ones((3, 4))
    with pytest.raises(ValueError, match="steps"):
        gospa_steps([a], [b, b], 10.0)
    for bad in (np.array([[0.0, np.nan]]), np.array([[np.inf, 0.0]])):
        with pytest.raises(ValueError, match="finite"):
            gospa_steps([bad], [b], 10.0)
        with pytest.raises(ValueError, match="finite"):
            gospa_steps([a], [bad], 10.0)
    for c in (0.0, -1.0, np.inf, np.nan, None, "10", True, 1e200):
        with pytest.raises(ValueError, match="c"):
            gospa_steps([a], [b], c)
    for p in (0, 3, 1.5, None, True):
        with pytest.raises(ValueError, match="p must"):
            gospa_steps([a], [b], 10.0, p=p)
    with pytest.raises(ValueError, match="array"):
        gospa_steps([np.zeros((2, 1))], [b], 10.0)
    with pytest.raises(ValueError, match="2048"):
        gospa_steps([np.zeros((2049, 2))], [b], 10.0)
    out = gospa_steps([], [], 10.0)      # (no steps: nothing to launch, no device needed)
    assert out["match"] == [] and all(len(out[k]) == 0 for k in ("gospa", "total", "localisation", "missed", "false", "nAssigned"))


def test_get_gospa_is_declared_with_its_switches_off():
    import inspect
    from pymht_amd.tracker import Tracker
    p = inspect.signature(Tracker.getGospa).parameters
    assert p["p"].default == 2 and p["terminated"].default is True
    assert p["smooth"].default is False and p["constantTurn"].default is False and p["ais"].default is False
    assert "as they stand at the call" in " ".join(Tracker.getGospa.__doc__.lower().split())
