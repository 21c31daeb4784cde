"""GPU: the device trial manoeuvres against every live hypothesis (`mht_trial_hypotheses`, include/mht_amd.h;
pymht_amd.evaluation.trial_hypotheses) and the drop-in path on top (Tracker.getHypothesisEncounters).

The properties are those tests/test_trial_hyp_cpu.py states and holds the host twin of the same header to; `check_figures` there holds
2, 3 and 8 against the device's OWN table:
  1  the table is bit for bit mht_trial_manoeuvres' out for n = L          5  table = NULL gives the same fig bits
  2  pcWorst, dcpaMin and their leaves: NumPy's nanmax / nanmin per segment   6  a permutation of the candidates permutes the rows
  3  the Sel rows are the table's column sel[t]                             7  every bad argument: MHT_E_INVALID, nothing written
  4  one leaf per target: pcMean == pcWorst == pcSel bit for bit            8  pcMean and weight within (2 nLeaves + 64) eps truth + 2 eps
     of the np.longdouble fold of the device's own table and the input cnllr
Every case prints the worst ratio to the bound of property 8 -- measured on an MI355X over all cases here, both builds alike:
    pcMean 0.0077, weight 0.0081   (the device's exp is within an ulp where it matters: the bound is not close)
and tools/trial_hyp_cost.py writes them into profiles/trial_hyp_cost.txt.  Nothing here is larger than 600 leaves, 3 candidates and 7
steps.  The shapes at which the kernels go round their grid-stride loops are
held in tests/test_encounter_strides_gpu.py."""
import numpy as np
import pytest

import encounter_ref as eref
import trial_hyp_ref as ref
import trial_ref
from test_encounter_cpu import RADIUS
from test_encounter_gpu import guard_untouched, guarded_work
from test_trial_hyp_cpu import CASES, DT, LAYOUTS, check_figures, scene

pytestmark = pytest.mark.gpu

SENTINEL = -7.03125e10


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


def _raw(ctx, x, P, cnllr, seg, sel, Phi, Q, K, dt, R, own, Sown, w, cand, table=True, nulls=(), nx=None, L=None, T=None, G=None, short=0,
         guard=0):
    """One call of the seam on x [L, N], P [L, N, N], the outputs preset to SENTINEL: (return code, table [5, G, L] or None, fig [8, G, T],
    weight [L], the table's array whether it was passed or not).  guard > 0: that many bytes of a pattern lie behind the sizer's figure
    and must be the pattern after the call."""
    import torch
    dev = ctx.device
    N = x.shape[1]
    cand = np.ascontiguousarray(cand, dtype=np.float64)
    xp, Pp = eref.pack(x, P)
    host = dict(Phi=np.ascontiguousarray(Phi, dtype=np.float64), Q=np.ascontiguousarray(Q, dtype=np.float64), own=np.ascontiguousarray(own, dtype=np.float64),
                Sown=np.ascontiguousarray(Sown, dtype=np.float64), cand=cand, seg=np.ascontiguousarray(seg, dtype=np.int32), sel=np.ascontiguousarray(sel, dtype=np.int32))
    n_l, n_t, n_g = len(x), len(host["sel"]), len(cand)
    arrays = dict(x=torch.from_numpy(xp).to(dev), P=torch.from_numpy(Pp).to(dev), cnllr=torch.from_numpy(np.ascontiguousarray(cnllr, dtype=np.float64)).to(dev))
    arrays["table"] = torch.full((5, n_g, n_l), SENTINEL, dtype=torch.float64, device=dev)
    arrays["fig"] = torch.full((8, n_g, n_t), SENTINEL, dtype=torch.float64, device=dev)
    arrays["weight"] = torch.full((n_l,), SENTINEL, dtype=torch.float64, device=dev)
    need = int(ctx.lib.mht_trial_hyp_work_bytes(n_l, n_t, n_g, min(max(K, 1), 64)))
    arrays["work"] = guarded_work(need, guard, dev)
    ptr = lambda k: None if k in nulls or (k == "table" and not table) else host[k].ctypes.data if k in host else arrays[k].data_ptr()
    torch.cuda.synchronize(dev)
    rc = ctx.lib.mht_trial_hypotheses(ctx.handle, N if nx is None else nx, n_l if L is None else L, n_t if T is None else T, n_g if G is None else G, K, dt, R,
                                      ptr("Phi"), ptr("Q"), ptr("x"), ptr("P"), ptr("cnllr"), ptr("seg"), ptr("sel"), ptr("own"), ptr("Sown"), w, ptr("cand"),
                                      ptr("table"), ptr("fig"), ptr("weight"), ptr("work"), need - short)
    torch.cuda.synchronize(dev)
    assert guard_untouched(arrays["work"], need), "the call wrote behind the work buffer the sizer asks for"
    tab = arrays["table"].cpu().numpy()
    return rc, (tab if table else None), arrays["fig"].cpu().numpy(), arrays["weight"].cpu().numpy(), tab


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("N,K,G,layout", CASES)
def test_segmented_fold_holds_the_properties_and_every_cell_is_written(ctxs, N, K, G, layout, lib_nx):
    """The cases of tests/test_trial_hyp_cpu.py: 600 leaves over three tiles -- segments of 1, 63, 64, 65, 0, one that ends exactly at
    leaf 256 and one of 300 that starts in the middle of a tile; one of 258 over three tiles; everything in one target -- G 1 and 3, K 1
    and 7; a NaN leaf, a segment all NaN, two identical leaves, a NaN and a +inf cnllr, a spread of 800 in cnllr, sel = -1.  Outputs preset
    to a sentinel, none left.  Properties 1, 2, 3, 5, 6 and 8."""
    from test_trial_gpu import _raw as raw_trial
    assert np.finfo(np.longdouble).eps < 1e-18
    x, P, cnllr, seg, sel, own, Sown, Phi, Q = scene(N, layout)
    cand = trial_ref.CANDIDATES[:G]
    args = (Phi, Q, K, DT, RADIUS, own, Sown, trial_ref.TURN_RATE)
    rc, table, fig, weight, _ = _raw(ctxs[lib_nx], x, P, cnllr, seg, sel, *args, cand)
    assert rc == 0 and not (table == SENTINEL).any() and not (fig == SENTINEL).any() and not (weight == SENTINEL).any()
    rc, out, _ = raw_trial(ctxs[lib_nx], x, P, *args, cand)
    assert rc == 0 and np.array_equal(table, out, equal_nan=True)
    check_figures("device N %d K %d G %d %s, %d-state build" % (N, K, G, layout, lib_nx), fig, weight, table, cnllr, seg, sel)
    rc, _, bare, bw, untouched = _raw(ctxs[lib_nx], x, P, cnllr, seg, sel, *args, cand, table=False)
    assert rc == 0 and np.array_equal(bare, fig, equal_nan=True) and np.array_equal(bw, weight, equal_nan=True) and (untouched == SENTINEL).all()
    if G == 3:
        order = np.array([2, 0, 1])
        rc, ptab, pfig, pw, _ = _raw(ctxs[lib_nx], x, P, cnllr, seg, sel, *args, cand[order])
        assert rc == 0 and np.array_equal(ptab, table[:, order], equal_nan=True) and np.array_equal(pfig, fig[:, order], equal_nan=True)
        assert np.array_equal(pw, weight, equal_nan=True)
    assert np.isnan(weight[140]) and weight[141] == 0.0 and (weight == 0.0).sum() >= 15 and np.isnan(table[:, :, 70]).all()
    assert np.array_equal(table[:, :, 130], table[:, :, 131], equal_nan=True)
    if layout == "mixed":
        assert np.isnan(fig[[0, 2, 4]][:, :, ref.NAN_SEGMENT]).all() and (fig[[1, 3]][:, :, ref.NAN_SEGMENT] == -1).all()
        assert np.isnan(fig[[0, 2, 4, 5, 6, 7]][:, :, 4]).all() and (fig[[1, 3]][:, :, 4] == -1).all()      # the empty target
        assert np.isnan(fig[5:, :, ref.NO_SELECTED]).all() and not np.isnan(fig[0, :, ref.NO_SELECTED]).any()
        assert LAYOUTS[layout][0][5] == 63 and seg[6] == 256


@pytest.mark.parametrize("N,lib_nx", [(4, 4), (4, 6), (6, 6), (6, 4)])
def test_one_leaf_per_target_gives_the_cell_bit_for_bit(ctxs, N, lib_nx):
    """Property 4: 300 targets of one leaf each: pcMean == pcWorst == pcSel == the table's pc bit for bit (w = exp(-0.0) = 1), also where
    the cnllr is 1e6 or -1e6; a leaf without a cnllr has no pcMean and keeps the rest."""
    from pymht_amd.models import ca, pv
    model = pv if N == 4 else ca
    L = 300
    x, P, cnllr, target, sel, own, Sown = ref.make_leaves(model, (1,) * L, seed=5, special=False)
    cnllr[7], cnllr[9], cnllr[11] = 1e6, -1e6, np.nan
    Phi, Q = eref.model_matrices(model, DT)
    rc, table, fig, weight, _ = _raw(ctxs[lib_nx], x, P, cnllr, ref.segments(target, L), sel, Phi, Q, 7, DT, RADIUS, own, Sown, trial_ref.TURN_RATE, trial_ref.CANDIDATES[:3])
    assert rc == 0 and not (fig == SENTINEL).any() and not (weight == SENTINEL).any()
    has = np.arange(L) != 11
    assert np.array_equal(fig[4][:, has], table[3][:, has], equal_nan=True) and np.isnan(fig[4][:, 11]).all() and not np.isnan(table[3][:, 11]).any()
    assert np.array_equal(fig[0], table[3], equal_nan=True) and np.array_equal(fig[5], table[3], equal_nan=True)
    assert np.array_equal(fig[2], table[1], equal_nan=True) and np.array_equal(fig[6], table[1], equal_nan=True) and np.array_equal(fig[7], table[0], equal_nan=True)
    assert np.array_equal(fig[1], np.where(np.isnan(table[3]), -1, np.arange(L)[None, :])) and (weight[has] == 1.0).all() and np.isnan(weight[11])
    assert int(np.sum(table[3] > 0)) > 20


def test_raw_abi_errors_and_the_call_behind_them(ctxs):
    """Property 7.  What mht_trial_manoeuvres refuses, a T outside 1 .. L, a seg that does not start at 0, decreases or does not end at
    L, a sel outside its segment, a null array, a work buffer one byte short: MHT_E_INVALID with the sentinels untouched; a null table
    is not an error; a call without leaves is MHT_OK and launches nothing."""
    from pymht_amd import _lib
    ctx = ctxs[4]
    x, P, cnllr, _, _, own, Sown, Phi, Q = scene(4, "mixed")
    x, P, cnllr = x[:6], P[:6], cnllr[:6]
    seg, sel = [0, 1, 1, 6], [0, -1, 3]
    nan, inf = float("nan"), float("inf")
    bad_cand = lambda row: np.vstack([trial_ref.CANDIDATES[:2], [row]])
    for kw in (dict(nx=5), dict(nx=3), dict(K=0), dict(K=65), dict(K=-1), dict(G=0), dict(G=-1), dict(G=4097), dict(L=-1), dict(R=0.0), dict(R=-1.0), dict(R=nan),
               dict(R=inf), dict(dt=0.0), dict(dt=-2.0), dict(dt=nan), dict(dt=inf), dict(w=0.0), dict(w=-0.05), dict(w=nan), dict(w=inf),
               dict(cand=bad_cand([3.2, 1.0, 0.0])), dict(cand=bad_cand([0.1, -0.5, 0.0])), dict(cand=bad_cand([0.1, 1.0, -1.0])), dict(cand=bad_cand([inf, 1.0, 0.0])),
               dict(cand=bad_cand([0.1, inf, 0.0])), dict(cand=bad_cand([0.1, 1.0, inf])), dict(own=[0.0, inf, 1.0, 1.0]), dict(Sown=[1.0, 0.0, inf]),
               dict(T=0), dict(T=-1), dict(L=2), dict(seg=[1, 1, 1, 6]), dict(seg=[0, 1, 1, 5]), dict(seg=[0, 1, 1, 7]), dict(seg=[0, 4, 3, 6]), dict(sel=[1, -1, 3]),
               dict(sel=[0, 1, 3]), dict(sel=[0, -1, 0]), dict(sel=[0, -1, 6]), dict(sel=[-2, -1, 3]),
               dict(nulls=("Phi",)), dict(nulls=("Q",)), dict(nulls=("x",)), dict(nulls=("P",)), dict(nulls=("cnllr",)), dict(nulls=("seg",)), dict(nulls=("sel",)),
               dict(nulls=("own",)), dict(nulls=("Sown",)), dict(nulls=("cand",)), dict(nulls=("fig",)), dict(nulls=("weight",)), dict(nulls=("work",)), dict(short=1)):
        rc, table, fig, weight, _ = _raw(ctx, x, P, cnllr, kw.get("seg", seg), kw.get("sel", sel), Phi, Q, kw.get("K", 3), kw.get("dt", DT), kw.get("R", RADIUS),
                                         kw.get("own", own), kw.get("Sown", Sown), kw.get("w", trial_ref.TURN_RATE), kw.get("cand", trial_ref.CANDIDATES[:3]),
                                         nulls=kw.get("nulls", ()), nx=kw.get("nx"), L=kw.get("L"), T=kw.get("T"), G=kw.get("G"), short=kw.get("short", 0))
        assert rc == _lib.MHT_E_INVALID and ctx.lib.mht_last_error(), kw
        assert (table == SENTINEL).all() and (fig == SENTINEL).all() and (weight == SENTINEL).all(), kw
    assert ctx.lib.mht_trial_hypotheses(ctx.handle, 4, 0, 0, 3, 3, DT, RADIUS, None, None, None, None, None, None, None, None, None, 0.05, None, None, None, None, None,
                                        0) == _lib.MHT_OK
    rc, table, fig, weight, _ = _raw(ctx, x, P, cnllr, seg, sel, Phi, Q, 3, DT, RADIUS, own, Sown, trial_ref.TURN_RATE, trial_ref.CANDIDATES[:3])
    assert rc == _lib.MHT_OK and not (table == SENTINEL).any() and not (fig == SENTINEL).any() and not (weight == SENTINEL).any()
    check_figures("the call behind the refusals", fig, weight, table, cnllr, np.array(seg), np.array(sel))


def test_module_function_gives_the_seams_bits(ctxs):
    """evaluation.trial_hypotheses on a Context and on a device ordinal: the raw call's figures, weights and (on request) table; the
    leaves as int64; nLeaves; selected=None gives NaN Sel rows and the target count of the last leaf's target."""
    from pymht_amd import evaluation
    x, P, cnllr, seg, sel, own, Sown, Phi, Q = scene(6, "mixed")
    target = np.repeat(np.arange(len(sel)), np.diff(seg))
    cand = trial_ref.CANDIDATES[:3]
    rc, table, fig, weight, _ = _raw(ctxs[6], x, P, cnllr, seg, sel, Phi, Q, 7, DT, RADIUS, own, Sown, trial_ref.TURN_RATE, cand)
    assert rc == 0
    cov = np.array([[Sown[0], Sown[1]], [Sown[1], Sown[2]]])
    for kw in (dict(ctx=ctxs[6], leafTable=True), dict(device=0), dict(ctx=ctxs[4])):
        res = evaluation.trial_hypotheses(x, P, cnllr, target, Phi, Q, 7, DT, RADIUS, own, cand, trial_ref.TURN_RATE, selected=sel, ownCovariance=cov, **kw)
        assert sorted(res) == sorted(ref.NAMES + ("weight", "nLeaves", "candidates") + (eref.NAMES if kw.get("leafTable") else ()))
        assert all(np.array_equal(res[k], fig[f], equal_nan=True) for f, k in enumerate(ref.NAMES)) and np.array_equal(res["weight"], weight, equal_nan=True)
        assert res["pcWorstLeaf"].dtype == np.int64 and res["dcpaMinLeaf"].dtype == np.int64 and np.array_equal(res["nLeaves"], np.diff(seg))
        assert not kw.get("leafTable") or all(np.array_equal(res[k], table[f], equal_nan=True) for f, k in enumerate(eref.NAMES))
    res = evaluation.trial_hypotheses(x, P, cnllr, target, Phi, Q, 7, DT, RADIUS, own, cand, trial_ref.TURN_RATE, ownCovariance=cov, ctx=ctxs[6])
    assert res["pcMean"].shape == (3, len(sel)) and np.isnan(res["pcSel"]).all() and np.array_equal(res["pcMean"], fig[4], equal_nan=True)


# ---- through the Tracker --------------------------------------------------------------------------------------------------------------
def test_tracker_holds_the_manoeuvres_against_every_leaf_of_a_cluttered_scene():
    """Two targets, three scans with clutter and P_d = 0.7 (pymht_amd.utils.scenario seed 3: the oracle, run here on the CPU, keeps 8 and 6
    leaves).  nLeaves are leafBatch()'s counts and the oracle's; the weights of a target sum to 1 within nLeaves eps; pcWorst >= pcSel;
    pcMean lies between the smallest and the largest leaf pc; pcWorstLeaf lies inside its segment; the selected leaf is the live track
    node; the host folds over the targets; the table is evaluation.trial_manoeuvres' on the leaves bit for bit."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import mht_oracle as orc
    from pymht_amd import evaluation
    from pymht_amd.models import pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    from pymht_amd.utils.scenario import make_scenario
    sc = make_scenario(T=2, radius=300.0, lambda_phi=2e-5, n_scans=3, P_d=0.7, seed=3)
    ot = orc.OracleTracker(sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=3, eta2=5.99)
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=3, eta2=5.99, useInitiator=False)
    try:
        for x0 in sc["x0"]:
            trk.initiateTarget(Target(sc["t0"], None, x0.copy(), pv.P0))
            ot.initiate_target(sc["t0"], x0.copy(), orc.model_P0())
        for zk, tk in zip(sc["scans"], sc["times"]):
            ot.add_scan(float(tk), zk)
            trk.addMeasurementList(MeasurementList(float(tk), zk))
        lb = trk.leafBatch()
        counts = np.bincount(lb["target"], minlength=2)
        assert counts.tolist() == [len(r.leaves()) for r in ot.targets] and counts.max() >= 2 and counts.tolist() == [8, 6]
        nodes = list(trk.getTrackNodes())
        own = np.array([lb["x"][0, 0] - 300.0, lb["x"][0, 1] + 40.0, 8.0, 0.0])
        deg = np.pi / 180.0
        got = trk.getHypothesisEncounters(60.0, 60.0, own, [0.0, 40.0 * deg, -40.0 * deg], 0.05, speedFactors=(1.0, 0.5), delay=5.0, ownCovariance=np.diag([4.0, 9.0]),
                                          steps=12, leafTable=True)
        G, T, L = 6, 2, len(lb["x"])
        assert got["pcMean"].shape == (G, T) and got["pc"].shape == (G, L) and got["ids"] == [int(n.ID) for n in nodes]
        assert np.array_equal(got["leafIds"], lb["ID"]) and np.array_equal(got["nLeaves"], counts)
        seg = np.concatenate([[0], np.cumsum(counts)])
        eps = np.finfo(np.float64).eps
        for t in range(T):
            s = slice(seg[t], seg[t + 1])
            assert abs(got["weight"][s].sum() - 1.0) <= counts[t] * eps
            assert (got["pcWorst"][:, t] >= got["pcSel"][:, t]).all() and (got["dcpaMin"][:, t] <= got["dcpaSel"][:, t]).all()
            assert (got["pcMean"][:, t] >= got["pc"][:, s].min(axis=1) * (1 - 4 * eps)).all() and (got["pcMean"][:, t] <= got["pc"][:, s].max(axis=1) * (1 + 4 * eps)).all()
            assert ((got["pcWorstLeaf"][:, t] >= seg[t]) & (got["pcWorstLeaf"][:, t] < seg[t + 1])).all()
            sel = int(np.flatnonzero((lb["target"] == t) & (lb["node"] == nodes[t]._node))[0])
            assert np.array_equal(got["pcSel"][:, t], got["pc"][:, sel]) and np.array_equal(got["tcpaSel"][:, t], got["tcpa"][:, sel])
            assert np.allclose(lb["x"][sel], nodes[t].x_0)
        print("pcMean", got["pcMean"], "pcWorst", got["pcWorst"], "pcSel", got["pcSel"], "weights", got["weight"])
        Phi, Q = eref.model_matrices(pv, 5.0)
        flat = evaluation.trial_manoeuvres(lb["x"], np.asarray(lb["P"], dtype=np.float64), Phi, Q, 12, 5.0, 60.0, own, got["candidates"], 0.05, ownCovariance=np.diag([4.0, 9.0]),
                                           ctx=trk._ctx)
        assert all(np.array_equal(got[k], flat[k], equal_nan=True) for k in eref.NAMES)
        assert np.array_equal(got["pcMeanMax"], got["pcMean"].max(axis=1)) and np.array_equal(got["pcMeanMaxTarget"], got["pcMean"].argmax(axis=1))
        assert np.array_equal(got["pcWorstMax"], got["pcWorst"].max(axis=1)) and np.array_equal(got["pcWorstMax"], flat["pcMax"])
        assert np.array_equal(got["dcpaMinAll"], flat["dcpaMin"]) and np.array_equal(got["dcpaMinAllTarget"], lb["target"][flat["dcpaArg"]])
        assert got["best"] == evaluation.trial_best(got["pcMeanMax"], got["dcpaMinAll"]) and got["bestWorstCase"] == evaluation.trial_best(flat["pcMax"], flat["dcpaMin"])
        stand_on = trk.getHypothesisEncounters(60.0, 60.0, own)      # the default: the own ship standing on, no turn rate needed
        assert stand_on["pcMean"].shape == (1, 2) and np.array_equal(stand_on["candidates"], [[0.0, 1.0, 0.0]]) and "pc" not in stand_on
        for bad in (dict(horizon=0.0), dict(radius=-1.0), dict(steps=65), dict(ownShip=np.zeros(3)), dict(ownCovariance=np.eye(3)), dict(courseChanges=[0.0, 0.5]),
                    dict(courseChanges=[0.5], turnRate=0.0), dict(courseChanges=[4.0], turnRate=0.05), dict(courseChanges=[]), dict(speedFactors=[-1.0]), dict(delay=-1.0)):
            kw = dict(horizon=60.0, radius=60.0, ownShip=own)
            kw.update(bad)
            with pytest.raises(ValueError, match="getHypothesisEncounters"):
                trk.getHypothesisEncounters(**kw)
    finally:
        trk.close()


def test_tracker_right_after_initiation_equals_the_best_hypothesis_view():
    """One leaf per target: every figure is evaluation.trial_manoeuvres' on the leaf states bit for bit, pcMean == pcWorst == pcSel, the
    weights are 1."""
    from pymht_amd import evaluation
    from pymht_amd.models import pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    x0 = np.array([[0.0, 0.0, -5.0, 0.0], [2000.0, 2000.0, 6.0, 3.0], [-300.0, 180.0, -7.0, 2.0]])
    trk = Tracker(pv, 2.5, 2e-6, 1e-4, P_d=0.9, N=3, eta2=5.99, useInitiator=False)
    try:
        for s in x0:
            trk.initiateTarget(Target(1000.0, None, s.copy(), pv.P0))
        own = np.array([-400.0, 0.0, 5.0, 0.0])
        got = trk.getHypothesisEncounters(60.0, 50.0, own, [0.0, 0.7], 0.05, steps=12, leafTable=True)
        lb = trk.leafBatch()
        assert got["nLeaves"].tolist() == [1, 1, 1] and (got["weight"] == 1.0).all() and len(lb["x"]) == 3
        Phi, Q = eref.model_matrices(pv, 5.0)
        flat = evaluation.trial_manoeuvres(lb["x"], np.asarray(lb["P"], dtype=np.float64), Phi, Q, 12, 5.0, 50.0, own, got["candidates"], 0.05, ctx=trk._ctx)
        assert all(np.array_equal(got[k], flat[k], equal_nan=True) for k in eref.NAMES) and not np.isnan(flat["pc"]).any()
        for k in ("pcMean", "pcWorst", "pcSel"):
            assert np.array_equal(got[k], flat["pc"]), k
        assert np.array_equal(got["dcpaMin"], flat["dcpa"]) and np.array_equal(got["dcpaSel"], flat["dcpa"]) and np.array_equal(got["tcpaSel"], flat["tcpa"])
        assert np.array_equal(got["pcWorstLeaf"], np.tile(np.arange(3), (2, 1))) and np.array_equal(got["pcWorstMax"], flat["pcMax"])
        assert got["best"] == evaluation.trial_best(flat["pcMax"], flat["dcpaMin"]) == got["bestWorstCase"]
    finally:
        trk.close()


def test_ais_aided_tracker_hands_down_the_forests_float64_covariances(monkeypatch):
    """An AIS-aided tracker after scans with messages: the entries handed to evaluation.trial_hypotheses are leafBatch()'s states and
    float64 covariances -- the AIS updates included, some of them carried in float64 by the forest -- and the call runs."""
    from ais_long_util import long_window_scenario, msgs_of
    from pymht_amd import evaluation
    from pymht_amd.models import pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, ais = long_window_scenario(96, 3, T=3, n_scans=4, msg_every=2, equipped=1.0, p_report=1.0)
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=3, eta2=5.99, radarRange=1.5 * sc["radius"], position=np.asarray(sc["centre"], dtype=np.float64),
                  aisAided=True, maxTargets=32, maxNodes=1 << 16, maxMeasurements=256)
    seen = {}
    inner = evaluation.trial_hypotheses

    def spy(x, P, cnllr, target, *a, **kw):
        seen.update(x=np.array(x), P=np.array(P), cnllr=np.array(cnllr), target=np.array(target))
        return inner(x, P, cnllr, target, *a, **kw)
    try:
        for x in sc["x0"]:
            trk.initiateTarget(Target(sc["t0"], None, x.copy(), pv.P0, status="preinitialized"))
        for z, t, msgs in zip(sc["scans"], sc["times"], ais):
            trk.addMeasurementList(MeasurementList(float(t), z), msgs_of(msgs), aisInitialization=False)
        assert sum(len(m) for m in ais) > 0
        lb = trk.leafBatch()
        monkeypatch.setattr(evaluation, "trial_hypotheses", spy)
        got = trk.getHypothesisEncounters(60.0, 80.0, [0.0, 0.0, 5.0, 2.0])
        assert seen["P"].dtype == np.float64 and lb["P"].dtype == np.float64 and np.array_equal(seen["P"], lb["P"]) and np.array_equal(seen["x"], lb["x"])
        assert lb["Pf64"].any() and (lb["mmsi"] != 0).any() and np.array_equal(seen["cnllr"], lb["cnllr"]) and np.array_equal(seen["target"], lb["target"])
        assert np.array_equal(got["nLeaves"], np.bincount(lb["target"], minlength=trk.nTargets)) and not np.isnan(got["pcMean"]).any()
        assert (got["pcWorst"] >= got["pcSel"]).all() and not np.isnan(got["pcSel"]).any()
    finally:
        trk.close()


def test_constant_turn_tracker_is_refused_and_no_tracks_give_empty_arrays():
    from pymht_amd.models import ct, pv
    from pymht_amd.tracker import Tracker
    turning = Tracker(ct, 2.5, 1e-7, 1e-4, P_d=0.9, N=4, eta2=5.99, useInitiator=False)
    try:
        with pytest.raises(NotImplementedError, match="ct"):
            turning.getHypothesisEncounters(30.0, 50.0, [0.0, 0.0, 1.0, 1.0])
    finally:
        turning.close()
    trk = Tracker(pv, 2.5, 2e-6, 1e-4, P_d=0.9, N=3, eta2=5.99, useInitiator=False)
    try:
        none = trk.getHypothesisEncounters(30.0, 50.0, [0.0, 0.0, 1.0, 1.0], [0.0, 0.5], 0.05, leafTable=True)
        assert none["ids"] == [] and none["best"] is None and none["bestWorstCase"] is None and len(none["leafIds"]) == 0
        assert all(none[k].shape == (2, 0) for k in ref.NAMES + eref.NAMES) and none["weight"].shape == (0,) and none["nLeaves"].shape == (0,)
        assert np.isnan(none["pcMeanMax"]).all() and (none["pcMeanMaxTarget"] == -1).all()
    finally:
        trk.close()
