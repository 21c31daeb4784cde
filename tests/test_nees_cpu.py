"""CPU: the NEES evaluation (csrc/mht_nees.h: nees_cell / nees_eval, what a lane of the kernels of mht_nees.hip runs per cell) compiled for
the host and held to the criterion of tests/test_nees_gpu.py on that test's own cell cases; the reference (tests/nees_ref.py) against
itself and against a plain solve; the host-side tests of the figures (pymht_amd.evaluation.nees_consistency) on a simulated batch; and
the refusals that need no GPU.

Criterion, the smoothers': per output family (error, nees2, nees4, nees) e = max |got - truth| / (1 + |truth|) over the cells that are
not NaN in the truth, e <= 8 max(e_np, eps64), truth the np.longdouble evaluation of the reference and e_np its float64 evaluation's
error; the NaN cells are the truth's exactly.  The scale e_np carries cond(P) -- the reference factorises the same matrices -- so no
absolute tolerance is named.  The measured ratios are in the docstrings of the tests."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import filter_ref
import nees_ref as ref
import smooth_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 2.5
FACTOR = 8.0
SENTINEL = -7.0
N_CPU, L_CPU = 23, 11      # (the GPU test runs the same cases at 130 x 60)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    so = str(tmp_path_factory.mktemp("nees_host") / "libnees_host.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "nees_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.nees_nodes_host.restype = C.c_int
    lib.nees_nodes_host.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 5
    return lib


def host_nees(lib, x, P, truth, present, D):
    """The twin on a batch in the seam's layouts: nees_ref.nees_batch's dict; every cell is written."""
    L_max, N, n = x.shape
    x, P, truth, present = [np.ascontiguousarray(a) for a in (x, P, truth, present)]
    out = np.full((L_max, N + 3, n), SENTINEL)
    assert lib.nees_nodes_host(N, n, L_max, D, x.ctypes.data, P.ctypes.data, truth.ctypes.data, present.ctypes.data, out.ctypes.data) == 0
    assert not (out == SENTINEL).any()
    return ref.seam_dict(out, N)


def _hold(label, got, truth, f64):
    res = ref.ratios([got], [truth], [f64], ref.NAMES)
    print(label + ": " + " | ".join("%s e %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert ref.same_nan([got], [truth], ref.NAMES), "the NaN cells are not the truth's"
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, (k, e, e_np, ratio)


def check_special_cells(got, N, D):
    """What the four special cells of nees_ref.cell_batch must look like in any evaluation"""
    b = ref.BAD_PIVOT
    assert np.isfinite(got["error"][b][:D]).all() and np.isnan(got["error"][b][D:]).all()
    assert np.isfinite(got["nees2"][b]) and got["nees2"][b] > 0 and np.isnan(got["nees4"][b]) and np.isnan(got["nees"][b])
    for cell in (ref.ABSENT, ref.NAN_X, ref.NAN_P):
        assert all(np.isnan(got[k][cell]).all() for k in ref.NAMES), cell
    assert np.isnan(got["nees4"]).all() == (D < 4) and np.isnan(got["nees"]).all() == (D < N)
    assert np.isfinite(got["nees2"]).sum() > 0.6 * got["nees2"].size


@pytest.mark.parametrize("N,D", [(4, 2), (4, 4), (6, 2), (6, 4), (6, 6)])
def test_nees_evaluation_on_the_host_meets_the_accuracy_criterion(lib, N, D):
    """nees_ref.cell_batch(N, 23, 11, seed 5): 253 cells, a fifth absent, covariances of varied conditioning.  Measured, host build
    (g++ -O2 -mfma), ratios e / max(e_np, eps64) for error / nees2 / nees4 / nees (the families a D does not reach have no finite cell:
    ratio 0):
        N 4 D 2   0 / 0.90 / 0 / 0             N 4 D 4   0.44 / 0.90 / 0.89 / 0.89
        N 6 D 2   0 / 1.00 / 0 / 0             N 6 D 4   0.49 / 1.00 / 1.03 / 0        N 6 D 6   0.49 / 1.00 / 1.03 / 0.81
    with e_np 1.1e-16 / 5.4e-16 / 8.1e-16 / 7.9e-14 at N 6 D 6 and 9.7e-17 / 4.2e-16 / 3.3e-14 / 3.3e-14 at N 4 D 4 (the error is one
    subtraction: the same bits as NumPy's).  The special cells: a pivot that is not positive at component 2 leaves
    nees2 and gives NaN in nees4 and nees; an absent cell and a cell with a NaN in x or P are NaN throughout."""
    assert np.finfo(np.longdouble).eps < 1e-18
    x, P, truth, present = ref.cell_batch(N, N_CPU, L_CPU, seed=5)
    got = host_nees(lib, x, P, truth, present, D)
    want, f64 = ref.nees_batch(x, P, truth, present, D, np.longdouble), ref.nees_batch(x, P, truth, present, D, np.float64)
    _hold("host build of the NEES evaluation, N %d D %d" % (N, D), got, want, f64)
    for ev in (got, want, f64):
        check_special_cells(ev, N, D)
    assert np.array_equal(got["error"], f64["error"], equal_nan=True)
    if N == 4 and D == 4:
        assert np.array_equal(got["nees4"], got["nees"], equal_nan=True)


@pytest.mark.parametrize("N", [4, 6])
def test_prefix_property_bit_for_bit(lib, N):
    """nees2 of a D = N call is nees2 of a D = 2 call, nees4 of a D = N call that of a D = 4 call, the errors the leading ones: the
    same bits (one factorisation, prefix sums); the components the smaller D does not carry are never read (NaN there changes nothing)."""
    x, P, truth, present = ref.cell_batch(N, N_CPU, L_CPU, seed=6)
    full = host_nees(lib, x, P, truth, present, N)
    for D in (2, 4):
        t = truth.copy()
        t[:, D:] = np.nan
        part = host_nees(lib, x, P, t, present, D)
        assert np.array_equal(part["nees2"], full["nees2"], equal_nan=True)
        assert np.array_equal(part["error"][..., :D], full["error"][..., :D], equal_nan=True)
        if D == 4:
            assert np.array_equal(part["nees4"], full["nees4"], equal_nan=True)


def test_bad_dimensions_are_refused_by_the_twin(lib):
    a = np.zeros(64)
    for nx, D in ((5, 2), (4, 3), (4, 6), (6, 5), (6, 0)):
        assert lib.nees_nodes_host(nx, 1, 1, D, a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data) == -1
    assert (a == 0).all()


def test_reference_is_self_consistent():
    """tests/nees_ref.py alone: float64 against longdouble below 1e-9 per family; every prefix sum is e_d' P_dd^-1 e_d under the
    marginal covariance, by a plain solve; the per-track form agrees with the batch form."""
    for N in (4, 6):
        x, P, truth, present = ref.cell_batch(N, N_CPU, L_CPU, seed=5)
        want, f64 = ref.nees_batch(x, P, truth, present, N, np.longdouble), ref.nees_batch(x, P, truth, present, N, np.float64)
        assert want["nees"].dtype == np.longdouble and ref.same_nan([f64], [want], ref.NAMES)
        res = ref.ratios([f64], [want], [f64], ref.NAMES)
        print(N, {k: v[0] for k, v in res.items()})
        assert all(np.isfinite(e) and e < 1e-9 for e, _, _ in res.values())
        Pm = filter_ref.full(np.moveaxis(P, 1, 2), N)
        for k, t in ((4, 3), (5, 7), (9, 20)):
            if np.isnan(f64["nees"][k, t]):
                continue
            e = f64["error"][k, t]
            for d, key in ((2, "nees2"), (4, "nees4"), (N, "nees")):
                assert np.isclose(f64[key][k, t], e[:d] @ np.linalg.solve(Pm[k, t][:d, :d], e[:d]), rtol=1e-9)
        t = 5
        tr = np.where(present[:, None, t] != 0, truth[:, :, t], np.nan)
        one = ref.nees_nodes(x[:, :, t], Pm[:, t], tr)
        assert all(np.array_equal(one[k], f64[k][:, t], equal_nan=True) for k in ref.NAMES)


SEED, N_SIM, L_SIM = 2, 150, 12


def _consistency_batch():
    from pymht_amd.models import pv
    tracks, states = ref.simulate(pv, PERIOD, N_SIM, L_SIM, SEED)
    mats = sr.model_matrices(pv, PERIOD)
    return [filter_ref.filter_lin(*mats, *t) for t in tracks], states


def test_nees_consistency_tells_an_honest_covariance_from_a_dishonest_one(lib):
    """pymht_amd.evaluation.nees_consistency on ONE batch simulated from models/pv's own Phi, Q, R (nees_ref.simulate: 150 tracks of
    12 nodes, seed 3, detection probability 0.9), filtered by tests/filter_ref.py in float64 and scored against the simulated states
    by tests/nees_ref.py in float64: the reference alone puts the matched filter inside both pooled intervals and inside the per-step
    interval at 11 or more of the 12 steps, P / 4 above every interval and P x 4 below (seeds 1 .. 8 were looked at on the CPU; all eight
    give the three pooled verdicts, seven of them 11 or more steps inside at both dimensions, and seed 2 lies nearest the middle of
    its intervals).  Observed, alpha = 0.05, dof 2 / 4:
        matched   mean 1.005 in (0.954, 1.047) / 1.003 in (0.968, 1.033)   outliers 0.053 / 0.052   steps inside 12 / 11
        P / 4     mean 4.021 / 4.010                                        P x 4   mean 0.251 / 0.251
    The host twin of the device evaluation, run on the same states, returns the same verdicts."""
    from pymht_amd.evaluation import nees_consistency
    alpha = 0.05
    filtered, states = _consistency_batch()

    def by_ref(scale):
        return [ref.nees_nodes(f["xf"], scale * f["Pf"], s) for f, s in zip(filtered, states)]

    def by_twin(scale):
        iu = np.triu_indices(4)
        x = np.ascontiguousarray(np.stack([f["xf"] for f in filtered], axis=2))
        P = np.ascontiguousarray(np.stack([(scale * f["Pf"])[:, iu[0], iu[1]] for f in filtered], axis=2))
        truth = np.ascontiguousarray(np.stack(states, axis=2))
        got = host_nees(lib, x, P, truth, np.ones((L_SIM, N_SIM), dtype=np.uint8), 4)
        return [{k: got[k][:, t] for k in ref.NAMES} for t in range(N_SIM)]

    verdicts = {}
    for how, run in (("reference", by_ref), ("twin", by_twin)):
        matched, small, big = (nees_consistency(run(s), alpha=alpha) for s in (1.0, 0.25, 4.0))
        for name, c in (("matched", matched), ("P / 4", small), ("P x 4", big)):
            print(how, name, {d: (round(f["mean"], 4), tuple(round(v, 4) for v in f["interval"]), round(f["outlierFraction"], 4),
                                  int(sum(v is True for v in f["perStep"]["inside"]))) for d, f in c["dims"].items()})
        assert sorted(matched["dims"]) == [2, 4] and matched["nCells"] == N_SIM * L_SIM
        for dof in (2, 4):
            m, s, b = matched["dims"][dof], small["dims"][dof], big["dims"][dof]
            assert m["n"] == N_SIM * L_SIM and m["inside"] is True and m["interval"][0] < 1.0 < m["interval"][1]
            assert sum(v is True for v in m["perStep"]["inside"]) >= L_SIM - 1 and len(m["perStep"]["step"]) == L_SIM
            assert (m["perStep"]["n"] == N_SIM).all() and np.array_equal(m["perStep"]["step"], np.arange(L_SIM))
            sigma = np.sqrt(alpha * (1 - alpha) / m["n"])
            assert abs(m["outlierFraction"] - alpha) <= 3 * sigma
            assert s["inside"] is False and s["mean"] > s["interval"][1] and all(v is False for v in s["perStep"]["inside"])
            assert (s["perStep"]["mean"] > s["perStep"]["hi"]).all() and s["outlierFraction"] > 4 * alpha
            assert b["inside"] is False and b["mean"] < b["interval"][0] and (b["perStep"]["mean"] < b["perStep"]["lo"]).all()
            assert np.isclose(s["mean"], 4 * m["mean"], rtol=1e-9) and np.isclose(b["mean"], m["mean"] / 4, rtol=1e-9)
        assert 1.0 < matched["rmsPosition"] < 10.0 and 0.1 < matched["rmsVelocity"] < 10.0
        verdicts[how] = [(c["dims"][d]["inside"], list(c["dims"][d]["perStep"]["inside"])) for c in (matched, small, big) for d in (2, 4)]
    assert verdicts["twin"] == verdicts["reference"]


def test_nees_consistency_of_degenerate_inputs_and_bad_alpha():
    from pymht_amd.evaluation import nees_consistency
    nan = np.nan
    blank = lambda L, N: dict(error=np.full((L, N), nan), nees2=np.full(L, nan), nees4=np.full(L, nan), nees=np.full(L, nan))
    for results in ([], [blank(1, 4)], [blank(5, 6), blank(2, 6)]):
        c = nees_consistency(results)
        assert c["nCells"] == 0 and c["dims"] == {} and np.isnan(c["rmsPosition"]) and np.isnan(c["rmsVelocity"]) and c["alpha"] == 0.05
    # positions only: one dimension, no velocity error; the steps given explicitly, a negative one left out
    r = blank(4, 6)
    r["error"][:3, :2] = [[3.0, 4.0], [0.0, 0.0], [6.0, 8.0]]
    r["nees2"][:3] = [2.0, 0.0, 50.0]
    r["step"] = np.array([7, 7, -1, 2])
    c = nees_consistency([r])
    assert c["nCells"] == 2 and sorted(c["dims"]) == [2] and np.isnan(c["rmsVelocity"]) and np.isclose(c["rmsPosition"], np.sqrt(12.5))
    f = c["dims"][2]
    assert f["n"] == 2 and f["mean"] == 0.5 and f["outlierFraction"] == 0.0 and f["perStep"]["step"].tolist() == [7] and f["perStep"]["n"].tolist() == [2]
    # a poisoned cell: NaN, not a verdict
    r["nees2"][0] = nan
    f = nees_consistency([r])["dims"][2]
    assert np.isnan(f["mean"]) and f["inside"] is None and np.isnan(f["outlierFraction"]) and f["perStep"]["inside"].tolist() == [None]
    with pytest.raises(ValueError, match="state dimension"):
        nees_consistency([blank(2, 4), blank(2, 6)])
    for alpha in (0.0, 1.0, -0.1, 1.5, float("nan"), None, "0.05", True):
        with pytest.raises(ValueError, match="alpha"):
            nees_consistency([r], alpha=alpha)


def test_refusals_that_need_no_gpu_and_what_the_docstrings_say():
    from pymht_amd import evaluation
    from pymht_amd.tracker import Tracker
    assert evaluation.nees_nodes([], [], []) == []
    x, P = np.zeros((3, 4)), np.tile(np.eye(4), (3, 1, 1))
    for bad in (([x], [P], []), ([np.zeros((3, 5))], [P], [np.zeros((3, 2))]), ([x], [P], [np.zeros((3, 3))]), ([x], [P], [np.zeros((2, 2))]),
                ([x], [np.zeros((3, 4, 3))], [np.zeros((3, 2))]), ([x], [P], [np.zeros((3, 6))])):
        with pytest.raises(ValueError, match="nees"):
            evaluation.nees_nodes(*bad)
    p = inspect.signature(Tracker.getNees).parameters
    assert [p[k].default for k in ("dims", "smooth", "constantTurn", "ais", "terminated", "alpha")] == [None, False, False, False, True, 0.05]
    doc = " ".join(Tracker.getNees.__doc__.split())
    assert "biases the NEES LOW" in doc and "AS THEY STAND AT THE CALL" in doc and "several standard deviations" in doc
    assert "correlated" in " ".join(evaluation.nees_consistency.__doc__.split())
