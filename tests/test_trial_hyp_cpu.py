"""CPU: the trial manoeuvres against every hypothesis (csrc/mht_trial_hyp.h: hyp_weights, hyp_cell, hyp_piece, hyp_target, what a lane of
the kernels of mht_trial_hyp.hip runs) compiled for the host and held to the properties of tests/test_trial_hyp_gpu.py, with
tests/trial_hyp_ref.py as the reference; and the refusals and docstring facts that need no GPU.

The properties (`check_figures` holds 2, 3 and 8 for both test files):
  1  the table is bit for bit mht_trial_manoeuvres' for n = L (here: the host twin of mht_trial.h)
  2  pcWorst, dcpaMin and their leaves are bit for bit NumPy's nanmax / nanmin per segment of the twin's own table, lowest index on ties
  3  the Sel rows are bit for bit the table's column sel[t], NaN where sel[t] = -1
  4  with one leaf per target pcMean == pcWorst == pcSel bit for bit
  5  table = NULL gives the same fig bits
  6  a permutation of the candidates permutes the rows bit for bit
  7  every bad argument is refused and nothing is written
  8  pcMean and weight: with the np.longdouble fold of the twin's OWN table and the input cnllr as the truth,
     |got - truth| <= (2 nLeaves + 64) eps truth + 2 eps  (trial_hyp_ref.mean_ratio states where the bound comes from)
Measured, host build (g++ -O2 -mfma, glibc's exp), the worst ratio to that bound over all cases here: pcMean 0.0085, weight 0.0070."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import encounter_ref as eref
import trial_hyp_ref as ref
import trial_ref
from test_encounter_cpu import RADIUS, hold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.03125e10      # (a value no case here produces)
DT = 5.0
LAYOUTS = {"mixed": (ref.SIZES, ref.NAN_SEGMENT, ref.NO_SELECTED), "span": (ref.SIZES_SPAN, 3, 0), "one": ((600,), None, None)}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    d = tmp_path_factory.mktemp("trial_hyp_host")
    libs = []
    for name in ("trial_hyp_host", "trial_host"):
        so = str(d / ("lib%s.so" % name))
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", os.path.join(ROOT, "tests", "hostmath", name + ".cpp"), "-o", so])
        libs.append(C.CDLL(so))
    lib, trial = libs
    lib.trial_hypotheses_host.restype = C.c_int
    lib.trial_hypotheses_host.argtypes = [C.c_int32] * 5 + [C.c_double] * 2 + [C.c_void_p] * 9 + [C.c_double] + [C.c_void_p] * 5 + [C.c_double]
    lib.trial_hyp_host_work_doubles.restype = C.c_int64
    lib.trial_hyp_host_work_doubles.argtypes = [C.c_int32] * 4
    trial.trial_manoeuvres_host.restype = C.c_int
    trial.trial_manoeuvres_host.argtypes = [C.c_int32] * 4 + [C.c_double] * 2 + [C.c_void_p] * 6 + [C.c_double] + [C.c_void_p] * 4
    trial.trial_host_work_doubles.restype = C.c_int64
    trial.trial_host_work_doubles.argtypes = [C.c_int32] * 3
    lib.trial = trial
    return lib


def host_hyp(lib, x, P, cnllr, seg, sel, Phi, Q, K, dt, R, own, Sown, w, cand, table=True):
    """The twin on x [L, N], P [L, N, N]: (table [5, G, L] or None, fig [8, G, T], weight [L]), every output preset to SENTINEL and none
    left"""
    L, N = x.shape
    cand = np.ascontiguousarray(cand, dtype=np.float64)
    G, T = len(cand), len(seg) - 1
    xp, Pp = eref.pack(x, P)
    Phi, Q = np.ascontiguousarray(Phi, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    own, Sown, cn = [np.ascontiguousarray(v, dtype=np.float64) for v in (own, Sown, cnllr)]
    seg, sel = np.ascontiguousarray(seg, dtype=np.int32), np.ascontiguousarray(sel, dtype=np.int32)
    tab = np.full((5, G, L), SENTINEL) if table else None
    fig, weight = np.full((8, G, T), SENTINEL), np.full(L, SENTINEL)
    work = np.full(int(lib.trial_hyp_host_work_doubles(L, T, G, K)), SENTINEL)
    rc = lib.trial_hypotheses_host(N, L, T, G, K, dt, R, Phi.ctypes.data, Q.ctypes.data, xp.ctypes.data, Pp.ctypes.data, cn.ctypes.data, seg.ctypes.data,
                                   sel.ctypes.data, own.ctypes.data, Sown.ctypes.data, w, cand.ctypes.data, tab.ctypes.data if table else None, fig.ctypes.data,
                                   weight.ctypes.data, work.ctypes.data, SENTINEL)
    assert rc == 0
    assert not (fig == SENTINEL).any() and not (weight == SENTINEL).any() and (tab is None or not (tab == SENTINEL).any())
    return tab, fig, weight


def host_trial_table(lib, x, P, Phi, Q, K, dt, R, own, Sown, w, cand):
    """out [5, G, n] of the host twin of mht_trial.h for the same call with n = L"""
    n, N = x.shape
    cand = np.ascontiguousarray(cand, dtype=np.float64)
    G = len(cand)
    xp, Pp = eref.pack(x, P)
    Phi, Q = np.ascontiguousarray(Phi, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    own, Sown = np.ascontiguousarray(own, dtype=np.float64), np.ascontiguousarray(Sown, dtype=np.float64)
    out, summary = np.full((5, G, n), SENTINEL), np.full((4, G), SENTINEL)
    work = np.zeros(int(lib.trial.trial_host_work_doubles(n, G, K)))
    assert lib.trial.trial_manoeuvres_host(N, n, G, K, dt, R, Phi.ctypes.data, Q.ctypes.data, xp.ctypes.data, Pp.ctypes.data, own.ctypes.data, Sown.ctypes.data, w,
                                           cand.ctypes.data, out.ctypes.data, summary.ctypes.data, work.ctypes.data) == 0
    return out


def check_figures(label, fig, weight, table, cnllr, seg, sel):
    """Properties 2, 3 and 8 of a call's fig [8, G, T] and weight [L] against its own table [5, G, L]; prints and returns the two ratios
    to the bound of property 8"""
    tab = eref.seam_dict(table)
    want = ref.fold(tab, cnllr, seg, sel, np.longdouble)
    for f, name in enumerate(ref.NAMES):
        if name != "pcMean":
            assert np.array_equal(fig[f], want[name].astype(np.float64), equal_nan=True), (label, name)
    n = want["nLeaves"]
    r_mean = ref.mean_ratio(fig[4], want["pcMean"], n[None, :])
    r_weight = ref.mean_ratio(weight, want["weight"], np.repeat(n, n))
    print("%s: worst ratio to the bound, pcMean %.3g, weight %.3g" % (label, r_mean, r_weight))
    assert r_mean <= 1.0 and r_weight <= 1.0, (label, r_mean, r_weight)
    # the weights of a target sum to 1, and pcMean lies between the smallest and the largest pc of its leaves
    for t in range(len(seg) - 1):
        wt = weight[seg[t]:seg[t + 1]]
        if len(wt) and not np.isnan(wt).all():
            assert abs(np.nansum(wt) - 1.0) <= max(len(wt), 2) * ref.EPS, (label, t)
    lo = np.array([[np.nanmin(tab["pc"][g, seg[t]:seg[t + 1]]) if not np.isnan(fig[4][g, t]) else np.nan for t in range(len(seg) - 1)] for g in range(len(fig[4]))])
    with np.errstate(invalid="ignore"):
        assert not (fig[4] > fig[0] * (1 + 4 * ref.EPS)).any() and not (fig[4] < lo * (1 - 4 * ref.EPS)).any(), label
    return r_mean, r_weight


_scenes = {}


def scene(N, layout):
    """trial_hyp_ref.make_leaves for a layout of LAYOUTS, once for both test files: (x, P, cnllr, seg, sel, own, Sown, Phi, Q)"""
    if (N, layout) not in _scenes:
        from pymht_amd.models import ca, pv
        model = pv if N == 4 else ca
        sizes, nan_segment, no_selected = LAYOUTS[layout]
        x, P, cnllr, target, sel, own, Sown = ref.make_leaves(model, sizes, seed=3, nan_segment=nan_segment, no_selected=no_selected)
        Phi, Q = eref.model_matrices(model, DT)
        _scenes[N, layout] = (x, P, cnllr, ref.segments(target, len(sizes)), sel, own, Sown, Phi, Q)
    return _scenes[N, layout]


CASES = [(4, 1, 3, "mixed"), (4, 7, 1, "span"), (6, 7, 3, "mixed"), (6, 1, 1, "one"), (4, 7, 3, "one"), (6, 1, 3, "span")]


@pytest.mark.parametrize("N,K,G,layout", CASES)
def test_host_twin_holds_the_properties(lib, N, K, G, layout):
    """600 leaves over three tiles in the layouts of trial_hyp_ref (segments of 1, 63, 64, 65, 0, one that ends at leaf 256, one of 300
    over two tiles with a second piece in its first tile; one of 258 over three tiles; everything in one target), G 1 and 3, K 1 and 7:
    a NaN leaf, a segment all NaN, two identical leaves, a NaN and a +inf cnllr, a spread of 800, sel = -1.  Properties 1, 2, 3, 5, 6, 8."""
    x, P, cnllr, seg, sel, own, Sown, Phi, Q = scene(N, layout)
    cand = trial_ref.CANDIDATES[:G]
    args = (Phi, Q, K, DT, RADIUS, own, Sown, trial_ref.TURN_RATE)
    table, fig, weight = host_hyp(lib, x, P, cnllr, seg, sel, *args, cand)
    assert np.array_equal(table, host_trial_table(lib, x, P, *args, cand), equal_nan=True)
    check_figures("host N %d K %d G %d %s" % (N, K, G, layout), fig, weight, table, cnllr, seg, sel)
    _, bare, bw = host_hyp(lib, x, P, cnllr, seg, sel, *args, cand, table=False)
    assert np.array_equal(bare, fig, equal_nan=True) and np.array_equal(bw, weight, equal_nan=True)
    if G == 3:
        order = np.array([2, 0, 1])
        ptab, pfig, pw = host_hyp(lib, x, P, cnllr, seg, sel, *args, cand[order])
        assert np.array_equal(ptab, table[:, order], equal_nan=True) and np.array_equal(pfig, fig[:, order], equal_nan=True) and np.array_equal(pw, weight, equal_nan=True)
    # what the scene is for
    assert np.isnan(weight[140]) and weight[141] == 0.0 and (weight == 0.0).sum() >= 15 and np.isnan(table[:, :, 70]).all()
    assert np.array_equal(table[:, :, 130], table[:, :, 131], equal_nan=True)
    if layout == "mixed":
        t = ref.NAN_SEGMENT
        assert np.isnan(fig[[0, 2, 4]][:, :, t]).all() and (fig[[1, 3]][:, :, t] == -1).all()
        assert np.isnan(fig[[0, 2, 4, 5, 6, 7]][:, :, 4]).all() and (fig[[1, 3]][:, :, 4] == -1).all()      # the empty target
        assert np.isnan(fig[5:, :, ref.NO_SELECTED]).all() and not np.isnan(fig[0, :, ref.NO_SELECTED]).any()


@pytest.mark.parametrize("N", [4, 6])
def test_one_leaf_per_target_gives_the_cell_bit_for_bit(lib, N):
    """Property 4: 300 targets of one leaf each (w = exp(-0.0) = 1, 1 * pc / 1): pcMean == pcWorst == pcSel == the table's pc, dcpaMin ==
    dcpaSel, the leaves are the leaves, every weight is 1; also where the cnllr is large or negative.  A leaf without a cnllr has no
    pcMean and keeps the rest."""
    from pymht_amd.models import ca, pv
    model = pv if N == 4 else ca
    L = 300
    x, P, cnllr, target, sel, own, Sown = ref.make_leaves(model, (1,) * L, seed=5, special=False)
    cnllr[7], cnllr[9], cnllr[11] = 1e6, -1e6, np.nan
    seg = ref.segments(target, L)
    Phi, Q = eref.model_matrices(model, DT)
    table, fig, weight = host_hyp(lib, x, P, cnllr, seg, sel, Phi, Q, 7, DT, RADIUS, own, Sown, trial_ref.TURN_RATE, trial_ref.CANDIDATES[:3])
    assert np.array_equal(sel, np.arange(L))
    has = np.arange(L) != 11
    assert np.array_equal(fig[4][:, has], table[3][:, has], equal_nan=True) and np.isnan(fig[4][:, 11]).all() and not np.isnan(table[3][:, 11]).any()
    assert np.array_equal(fig[0], table[3], equal_nan=True) and np.array_equal(fig[5], table[3], equal_nan=True)
    assert np.array_equal(fig[2], table[1], equal_nan=True) and np.array_equal(fig[6], table[1], equal_nan=True) and np.array_equal(fig[7], table[0], equal_nan=True)
    assert np.array_equal(fig[1], np.where(np.isnan(table[3]), -1, np.arange(L)[None, :])) and (weight[has] == 1.0).all() and np.isnan(weight[11])
    assert int(np.sum(table[3] > 0)) > 20


def test_table_meets_the_cells_criterion_and_the_float64_reference_its_own():
    """trial_hyp_ref.cells (trial_ref.manoeuvres on the leaves) in float64 and np.longdouble agree under the project's criterion
    (test_encounter_cpu.hold), and the float64 fold of trial_hyp_ref -- the header's order of the sums -- meets property 8 against the
    np.longdouble fold of the same table."""
    from pymht_amd.models import pv
    x, P, cnllr, target, sel, own, Sown = ref.make_leaves(pv, (1, 30, 0, 39), seed=4, special=False)
    seg = ref.segments(target, 4)
    Phi, Q = eref.model_matrices(pv, DT)
    args = (x, P, Phi, Q, 3, DT, RADIUS, own, Sown, trial_ref.TURN_RATE, trial_ref.CANDIDATES[:2])
    f64, truth = ref.cells(*args), ref.cells(*args, truth=True)
    hold("float64 cells of the leaves", f64, truth, f64, DT, names=("tcpa", "dcpa", "md2"))
    mine, want = ref.fold(f64, cnllr, seg, sel), ref.fold(f64, cnllr, seg, sel, np.longdouble)
    assert all(np.array_equal(mine[k], want[k].astype(mine[k].dtype), equal_nan=True) for k in ref.NAMES if k != "pcMean")
    assert ref.mean_ratio(mine["pcMean"], want["pcMean"], want["nLeaves"][None, :]) <= 1.0
    assert ref.mean_ratio(mine["weight"], want["weight"], np.repeat(want["nLeaves"], want["nLeaves"])) <= 1.0
    assert mine["pcMean"][0, 0] == f64["pc"][0, 0] and np.isnan(mine["pcMean"][:, 2]).all() and want["nLeaves"].tolist() == [1, 30, 0, 39]


def test_refusals_that_need_no_gpu_and_what_the_docstrings_say(lib):
    """Property 7 on the twin: nothing is written.  evaluation.trial_hypotheses: ValueError for every argument that does not fit, before
    a device is needed; no leaf gives empty arrays.  The signatures and docstring facts of the two entry points; the constant-turn
    refusal."""
    from pymht_amd import evaluation
    from pymht_amd.models import ct, pv
    from pymht_amd.tracker import Tracker
    a = np.zeros(512)
    p = a.ctypes.data
    nan, inf = float("nan"), float("inf")
    seg, sel = np.array([0, 1, 2], dtype=np.int32), np.array([0, -1], dtype=np.int32)
    ok = dict(nx=4, L=2, T=2, G=2, K=3, dt=1.0, R=1.0, w=0.1, seg=seg, sel=sel)
    i32 = lambda v: np.array(v, dtype=np.int32)
    for bad in (dict(nx=5), dict(K=0), dict(K=65), dict(G=0), dict(G=4097), dict(L=-1), dict(dt=0.0), dict(dt=nan), dict(dt=inf), dict(R=0.0), dict(R=-1.0), dict(R=inf),
                dict(w=0.0), dict(w=-0.1), dict(w=nan), dict(w=inf), dict(T=0), dict(T=3, seg=i32([0, 1, 2, 2]), sel=i32([0, 1, -1])), dict(seg=i32([1, 1, 2])),
                dict(seg=i32([0, 1, 3])), dict(seg=i32([0, 1, 1])), dict(T=3, L=3, seg=i32([0, 2, 1, 3]), sel=i32([-1, -1, -1])), dict(sel=i32([1, -1])), dict(sel=i32([0, 0])),
                dict(sel=i32([0, 2])), dict(sel=i32([-2, -1]))):
        kw = dict(ok)
        kw.update(bad)
        rc = lib.trial_hypotheses_host(kw["nx"], kw["L"], kw["T"], kw["G"], kw["K"], kw["dt"], kw["R"], p, p, p, p, p, kw["seg"].ctypes.data, kw["sel"].ctypes.data, p, p,
                                       kw["w"], p, p, p, p, p, 0.0)
        assert rc == -1, bad
    for c in ([4.0, 1.0, 0.0], [0.1, -0.5, 0.0], [0.1, 1.0, -1.0], [inf, 1.0, 0.0]):
        cand = np.array([[0.0, 1.0, 0.0], c])
        assert lib.trial_hypotheses_host(4, 2, 2, 2, 3, 1.0, 1.0, p, p, p, p, p, seg.ctypes.data, sel.ctypes.data, p, p, 0.1, cand.ctypes.data, p, p, p, p, 0.0) == -1, c
    assert (a == 0).all()
    x, P = np.zeros((3, 4)), np.tile(np.eye(4), (3, 1, 1))
    Phi, Q = eref.model_matrices(pv, 2.5)
    good = dict(x=x, P=P, cnllr=[1.0, 2.0, nan], target=[0, 0, 2], Phi=Phi, Q=Q, steps=4, dt=2.5, radius=50.0, own=[0.0, 0.0, 1.0, 0.0],
                candidates=[[0.0, 1.0, 0.0], [0.5, 1.0, 0.0]], turnRate=0.05)
    for bad in (dict(x=np.zeros((3, 5))), dict(x=np.zeros(4)), dict(P=np.zeros((3, 4, 3))), dict(P=np.zeros((2, 4, 4))), dict(Phi=np.eye(6)), dict(Q=np.eye(3)), dict(steps=0),
                dict(steps=65), dict(steps=2.5), dict(steps=True), dict(dt=0.0), dict(dt=nan), dict(radius=0.0), dict(radius=inf), dict(Phi=np.full((4, 4), nan)),
                dict(turnRate=0.0), dict(turnRate=nan), dict(turnRate=None), dict(own=[0.0, 0.0]), dict(own=[0.0, 0.0, 1.0, inf]), dict(ownCovariance=np.eye(3)),
                dict(ownCovariance=[[1.0, 0.5], [0.2, 1.0]]), dict(candidates=[]), dict(candidates=[[3.2, 1.0, 0.0]]), dict(candidates=[[0.1, inf, 0.0]]),
                dict(cnllr=[1.0, 2.0]), dict(cnllr=[1.0, -inf, 2.0]), dict(cnllr=np.zeros((3, 1))), dict(target=[0, 2, 1]), dict(target=[-1, 0, 0]), dict(target=[0, 0]),
                dict(target=[0.0, 0.0, 1.0]), dict(selected=[0, -1]), dict(selected=[2, -1, -1]), dict(selected=[0, 0, 2]), dict(selected=[0, -1, 3]),
                dict(selected=[0.0, -1.0, 2.0]), dict(selected=[[0, -1, 2]])):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError, match="trial_hypotheses"):
            evaluation.trial_hypotheses(**kw)
    for table in (False, True):      # no leaf: empty arrays, no device
        out = evaluation.trial_hypotheses(**dict(good, x=x[:0], P=P[:0], cnllr=[], target=np.zeros(0, dtype=np.int32), selected=[-1, -1], leafTable=table))
        assert sorted(out) == sorted(ref.NAMES + ("weight", "nLeaves", "candidates") + (eref.NAMES if table else ()))
        assert all(out[k].shape == (2, 2) for k in ref.NAMES) and out["weight"].shape == (0,) and out["nLeaves"].tolist() == [0, 0]
        assert np.isnan(out["pcMean"]).all() and out["pcWorstLeaf"].dtype == np.int64 and (out["pcWorstLeaf"] == -1).all() and (out["dcpaMinLeaf"] == -1).all()
        assert not table or all(out[k].shape == (2, 0) for k in eref.NAMES)
    assert evaluation.TRIAL_HYP_NAMES == ref.NAMES
    sig = inspect.signature(evaluation.trial_hypotheses).parameters
    assert list(sig) == ["x", "P", "cnllr", "target", "Phi", "Q", "steps", "dt", "radius", "own", "candidates", "turnRate", "selected", "ownCovariance", "leafTable",
                         "device", "ctx"]
    doc = " ".join(evaluation.trial_hypotheses.__doc__.split())
    assert "NORMALISE INSIDE ONE TARGET" in doc and "exclusion constraints between targets" in doc and "one leaf has pcMean = pc" in doc and "-inf is refused" in doc
    hdr = " ".join(open(os.path.join(ROOT, "pymht_amd", "csrc", "mht_trial_hyp.h")).read().split())
    assert "normalise INSIDE ONE TARGET" in hdr and "exp(-0.0) = 1 exactly" in hdr and "track-oriented approximation" in hdr
    sig = inspect.signature(Tracker.getHypothesisEncounters).parameters
    assert list(sig) == ["self", "horizon", "radius", "ownShip", "courseChanges", "turnRate", "speedFactors", "delay", "ownCovariance", "steps", "leafTable"]
    assert sig["courseChanges"].default == (0.0,) and sig["turnRate"].default is None and sig["speedFactors"].default == (1.0,) and sig["leafTable"].default is False
    src = inspect.getsource(Tracker.getHypothesisEncounters)
    assert "encounter_model" in src and "leafBatch" in src and "getFilteredTracks" not in src.split('"""')[2]
    doc = " ".join(Tracker.getHypothesisEncounters.__doc__.split())
    assert "include the AIS updates" in doc and "NotImplementedError" in doc and "INSIDE ONE TARGET" in doc and "track-oriented approximation" in doc
    with pytest.raises(NotImplementedError, match="ct"):
        evaluation.encounter_model(ct, 2.5)
    # getEncounters and getTrialManoeuvres still say what they do not use
    assert "AIS-aided filter's state is NOT used" in " ".join(Tracker.getTrialManoeuvres.__doc__.split())
