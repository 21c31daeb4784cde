"""GPU: the device NEES (`mht_nees_nodes`, include/mht_amd.h; pymht_amd.evaluation.nees_nodes) and the drop-in path on top
(Tracker.getNees), against tests/nees_ref.py.

The criterion is the smoothers' (tests/test_smooth_trace_gpu.py), per output family (error, nees2, nees4, nees): with the np.longdouble
evaluation of the reference as the truth, over the cells that are not NaN in it,
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
and e_dev <= 8 * max(e_np, eps64); the NaN cells are the truth's exactly.  The float64 reference sets the scale, never the device: it
factorises the same matrices, so the scale carries cond(P) and no absolute tolerance is named.  The host twin of the same header
measures ratios of 0.44 - 1.03 on cells of the same make (tests/test_nees_cpu.py); every test prints the device's own -- measured on
an MI355X, both builds alike, error / nees2 / nees4 / nees:
    cells N 4 D 4          0.49 / 0.92 / 0.76 / 0.76   (e_np 1.1e-16 / 7.0e-15 / 1.3e-12 / 1.3e-12)
    cells N 6 D 6          0.48 / 1.44 / 0.75 / 1.84   (e_np 1.1e-16 / 1.0e-15 / 1.0e-14 / 5.3e-13); the smaller D: the same leading figures
    filter's outputs       pv 0.42 / 1.38 / 1.41 / 1.41   ca 0.40 / 1.00 / 0.87 / 0.85
    smoother's outputs     pv 0.40 / 1.07 / 1.01 / 1.01   ca 0.32 / 1.21 / 1.00 / 0.91
    getNees                filtered 0.27 / 1.16 / 1.28 / 1.28   smoothed 0.25 / 1.15 / 0.99 / 0.99
-- and tools/nees_cost.py writes them into profiles/nees_cost.txt.  Nothing here is larger than 130 tracks of 60 nodes."""
import numpy as np
import pytest

import filter_ref
import nees_ref as ref
from test_nees_cpu import check_special_cells

pytestmark = pytest.mark.gpu

PERIOD = 2.5
FACTOR = 8.0
SENTINEL = -7.0
N_TRACKS, L_MAX = 130, 60


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


def _raw(ctx, N, D, x, P, truth, present, nulls=(), nx=None):
    """One call of the seam on host arrays in its layouts (or device tensors, for x and P), the output preset to SENTINEL:
    (return code, out [L_max, N + 3, n])"""
    import torch
    dev = ctx.device
    up = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    arrays = dict(x=up(x), P=up(P), truth=up(truth), present=up(np.asarray(present, dtype=np.uint8)))
    L_max, _, n = arrays["x"].shape
    out = torch.full((L_max, N + 3, n), SENTINEL, dtype=torch.float64, device=dev)
    ptr = lambda k: None if k in nulls else arrays[k].data_ptr()
    torch.cuda.synchronize(dev)
    rc = ctx.lib.mht_nees_nodes(ctx.handle, N if nx is None else nx, n, L_max, D, ptr("x"), ptr("P"), ptr("truth"), ptr("present"),
                                None if "out" in nulls else out.data_ptr())
    torch.cuda.synchronize(dev)
    return rc, out.cpu().numpy()


def _hold(label, got, truth, f64):
    res = ref.ratios(got, truth, f64, ref.NAMES)
    print(label + ": " + " | ".join("%s e_dev %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert ref.same_nan(got, truth, ref.NAMES), "the NaN cells are not the truth's"
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, "%s: e_dev %.3g > %g x max(e_np %.3g, eps)" % (k, e, FACTOR, e_np)


@pytest.mark.parametrize("N,D,lib_nx", [(4, 2, 4), (4, 4, 4), (4, 4, 6), (6, 2, 6), (6, 4, 6), (6, 6, 6), (6, 6, 4)])
def test_cell_cases_meet_the_accuracy_criterion_and_every_cell_is_written(ctxs, N, D, lib_nx):
    """nees_ref.cell_batch(N, 130, 60, seed 5), the cases of tests/test_nees_cpu.py at 7800 cells (31 workgroups, the last one partly
    filled, wavefronts that straddle the end of a row): the output preset to a sentinel, none left; the special cells -- a pivot that
    is not positive at component 2, an absent cell, a NaN in x and in P -- as the reference has them; the prefix property against the
    D = N call on the device, bit for bit."""
    assert np.finfo(np.longdouble).eps < 1e-18
    x, P, truth, present = ref.cell_batch(N, N_TRACKS, L_MAX, seed=5)
    rc, out = _raw(ctxs[lib_nx], N, D, x, P, truth, present)
    assert rc == 0 and not (out == SENTINEL).any()
    got = ref.seam_dict(out, N)
    want, f64 = ref.nees_batch(x, P, truth, present, D, np.longdouble), ref.nees_batch(x, P, truth, present, D, np.float64)
    _hold("NEES cells N %d D %d, %d-state build" % (N, D, lib_nx), [got], [want], [f64])
    check_special_cells(got, N, D)
    assert np.array_equal(got["error"], f64["error"], equal_nan=True)
    if D < N:
        t = truth.copy()
        t[:, D:] = np.nan      # (components the truth does not carry are never read)
        rc, part = _raw(ctxs[lib_nx], N, D, x, P, t, present)
        rc2, full = _raw(ctxs[lib_nx], N, N, x, P, truth, present)
        assert rc == 0 and rc2 == 0 and np.array_equal(part, out, equal_nan=True)
        full = ref.seam_dict(full, N)
        assert np.array_equal(got["nees2"], full["nees2"], equal_nan=True) and np.array_equal(got["error"][..., :D], full["error"][..., :D], equal_nan=True)
        assert D < 4 or np.array_equal(got["nees4"], full["nees4"], equal_nan=True)


def _cut_batch(model, seed):
    """nees_ref.simulate, 130 tracks cut to filter_ref's edge lengths 1, 2, 60, 7, 33 in turn: (tracks, states)"""
    tracks, states = ref.simulate(model, PERIOD, N_TRACKS, L_MAX, seed)
    lengths = filter_ref.edge_lengths(N_TRACKS)
    return [(x0, P0, z[:L]) for (x0, P0, z), L in zip(tracks, lengths)], [s[:L] for s, L in zip(states, lengths)]


@pytest.mark.parametrize("name,smooth", [("pv", False), ("pv", True), ("ca", False), ("ca", True)])
def test_nees_of_the_filters_and_the_smoothers_device_outputs(ctxs, name, smooth):
    """mht_nees_nodes reads xf, Pf of mht_filter_tracks (xs, Ps of mht_smooth_tracks) where the seam wrote them: 130 tracks simulated
    from the model, of 1, 2, 60, 7, 33 nodes in turn, every node flagged present -- the rows behind a track's end, NaN in x and P, come
    back NaN.  Against tests/nees_ref.py on the host copies of those outputs; evaluation.nees_nodes on the per-track arrays gives the
    same bits."""
    import importlib
    from pymht_amd import evaluation, smoothing
    model = importlib.import_module("pymht_amd.models." + name)
    N = 4 if name == "pv" else 6
    ctx = ctxs[N]
    tracks, states = _cut_batch(model, seed=21)
    if smooth:
        x_d, P_d, lens, order, L_max = smoothing._smooth(ctx, model, PERIOD, tracks, N, True, False, on_device=True)
    else:
        x_d, P_d, lens, order, L_max = smoothing._filter(ctx, model, PERIOD, tracks, N, False, on_device=True)
    assert L_max == L_MAX and x_d.shape == (L_MAX, N, N_TRACKS) and P_d.shape == (L_MAX, N * (N + 1) // 2, N_TRACKS)
    truth = np.zeros((L_MAX, N, N_TRACKS))
    for j, t in enumerate(order):
        truth[:lens[t], :, j] = states[t]
    present = np.ones((L_MAX, N_TRACKS), dtype=np.uint8)
    rc, out = _raw(ctx, N, N, x_d, P_d, truth, present)
    assert rc == 0 and not (out == SENTINEL).any()
    got = ref.seam_dict(out, N)
    x, P = x_d.cpu().numpy(), P_d.cpu().numpy()
    want, f64 = ref.nees_batch(x, P, truth, present, N, np.longdouble), ref.nees_batch(x, P, truth, present, N, np.float64)
    _hold("NEES of the %s's outputs, models/%s" % ("smoother" if smooth else "filter", name), [got], [want], [f64])
    for j, t in enumerate(order):
        assert np.isnan(out[lens[t]:, :, j]).all() and np.isfinite(out[:lens[t], :, j]).all()
    # the public form on per-track arrays
    run = smoothing.smooth_tracks if smooth else smoothing.filter_tracks
    per = run(model, PERIOD, tracks, ctx=ctx)
    res = evaluation.nees_nodes([a for a, _ in per], [b for _, b in per], states, ctx=ctx)
    for j, t in enumerate(order):
        L = lens[t]
        assert sorted(res[t]) == ["error", "nees", "nees2", "nees4"] and res[t]["error"].shape == (L, N)
        assert np.array_equal(res[t]["error"], got["error"][:L, j]) and all(np.array_equal(res[t][k], got[k][:L, j]) for k in ("nees2", "nees4", "nees"))
    c = evaluation.nees_consistency(res)
    print({d: (f["mean"], f["interval"], f["inside"]) for d, f in c["dims"].items()})
    assert sorted(c["dims"]) == sorted({2, 4, N}) and c["nCells"] == int(lens.sum())
    assert all(0.5 < f["mean"] < 1.5 for f in c["dims"].values())      # (a matched model: near 1; the verdicts are the CPU test's business)


def test_raw_abi_errors_and_the_call_behind_them(ctxs):
    """A bad nx or D, a negative size, a null array: MHT_E_INVALID with the sentinel untouched; an empty batch is MHT_OK."""
    from pymht_amd import _lib
    ctx = ctxs[4]
    x, P, truth, present = ref.cell_batch(4, 5, 6, seed=1)
    for kw in (dict(nx=5), dict(nx=3), dict(D=3), dict(D=6), dict(D=0), dict(nulls=("x",)), dict(nulls=("P",)), dict(nulls=("truth",)),
               dict(nulls=("present",)), dict(nulls=("out",))):
        rc, out = _raw(ctx, 4, kw.get("D", 4), x, P, truth, present, nulls=kw.get("nulls", ()), nx=kw.get("nx"))
        assert rc == _lib.MHT_E_INVALID and ctx.lib.mht_last_error() and (out == SENTINEL).all(), kw
    assert ctx.lib.mht_nees_nodes(ctx.handle, 4, -1, 3, 4, None, None, None, None, None) == _lib.MHT_E_INVALID
    assert ctx.lib.mht_nees_nodes(ctx.handle, 4, 0, 3, 4, None, None, None, None, None) == _lib.MHT_OK
    assert ctx.lib.mht_nees_nodes(ctx.handle, 6, 3, 0, 2, None, None, None, None, None) == _lib.MHT_OK
    rc, out = _raw(ctx, 4, 4, x, P, truth, present)
    assert rc == _lib.MHT_OK and not (out == SENTINEL).any()


def test_tracker_histories_against_the_scenario_truth():
    """Eight targets initiated from the scenario's x0, twenty scans.  getNees, filtered and with smooth=True: the per-node figures are
    tests/nees_ref.py applied to getFilteredTracks (to smoothing.smooth_tracks on the same chains) under the pairing of getGospa,
    collected here from the track nodes; nAssigned is getGospa's; dims=2 gives the same position figures; the refusals."""
    from pymht_amd.models import pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.smoothing import chain_inputs, smooth_tracks
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    from pymht_amd.utils.scenario import make_scenario
    sc = make_scenario(T=8, radius=600, lambda_phi=2e-6, n_scans=20)
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=3, eta2=5.99, useInitiator=False)
    try:
        for x0 in sc["x0"]:
            trk.initiateTarget(Target(sc["t0"], None, x0.copy(), pv.P0))
        for zk, tk in zip(sc["scans"], sc["times"]):
            trk.addMeasurementList(MeasurementList(float(tk), zk))
        truth = (sc["times"], sc["truth"])
        nodes = list(trk.getTrackNodes()) + list(trk.__terminatedTargets__)
        chains = [n.backtrackNodes() for n in nodes]
        assert len(nodes) >= 8 and sc["truth"][0].shape == (8, 4)
        for smooth in (False, True):
            got = trk.getNees(truth, c=20, smooth=smooth)
            gospa = trk.getGospa(truth, c=20, smooth=smooth)
            assert got["dims"] == 4 and len(got["tracks"]) == len(nodes) and len(got["trackIds"]) == len(nodes)
            assert got["nAssigned"] == int(gospa["nAssigned"].sum()) > 100 and got["nIgnored"] == gospa["nIgnored"] > 0
            assert got["nAssigned"] + got["nUnassigned"] + got["nIgnored"] == sum(len(ch) for ch in chains)
            if smooth:
                states = smooth_tracks(pv, trk.radarPeriod, [chain_inputs(n, pv.P0)[1] for n in nodes], ctx=trk._ctx)
            else:
                states = trk.getFilteredTracks(terminated=True)
            paired = [np.full((len(ch), 4), np.nan) for ch in chains]
            seen = [0] * len(sc["times"])
            for i, ch in enumerate(chains):      # getGospa's order of the estimates of a step: history by history, node by node
                for k, nd in enumerate(ch):
                    hit = np.flatnonzero(sc["times"] == float(nd.time))
                    if len(hit):
                        s = int(hit[0])
                        row = int(gospa["match"][s][seen[s]])
                        seen[s] += 1
                        assert got["tracks"][i]["step"][k] == s
                        if row >= 0:
                            paired[i][k] = sc["truth"][s][row]
                    else:
                        assert got["tracks"][i]["step"][k] == -1
            want = [ref.nees_nodes(x, P, t, np.longdouble) for (x, P), t in zip(states, paired)]
            f64 = [ref.nees_nodes(x, P, t, np.float64) for (x, P), t in zip(states, paired)]
            _hold("getNees smooth=%s" % smooth, got["tracks"], want, f64)
            assert sum(int(np.isfinite(d["nees"]).sum()) for d in got["tracks"]) == got["nAssigned"]
            c = got["consistency"]
            print({d: (round(f["mean"], 3), f["interval"], f["inside"], round(f["outlierFraction"], 3)) for d, f in c["dims"].items()},
                  "rms", c["rmsPosition"], c["rmsVelocity"])
            assert sorted(c["dims"]) == [2, 4] and c["nCells"] == got["nAssigned"] and c["alpha"] == 0.05 and np.isfinite(c["rmsVelocity"])
            pos = trk.getNees(truth, c=20, dims=2, smooth=smooth)
            assert pos["dims"] == 2 and pos["nAssigned"] == got["nAssigned"] and sorted(pos["consistency"]["dims"]) == [2]
            for a, b in zip(pos["tracks"], got["tracks"]):
                assert np.array_equal(a["nees2"], b["nees2"], equal_nan=True) and np.isnan(a["nees4"]).all() and np.isnan(a["error"][:, 2:]).all()
        two = (sc["times"], [y[:, :2] for y in sc["truth"]])
        assert trk.getNees(two, c=20)["dims"] == 2
        with pytest.raises(ValueError, match="columns"):
            trk.getNees(two, c=20, dims=4)
        with pytest.raises(ValueError, match="dims"):
            trk.getNees(truth, c=20, dims=3)
        for kw in (dict(constantTurn=True), dict(ais=True)):
            with pytest.raises(ValueError, match="smooth"):
                trk.getNees(truth, c=20, **kw)
        with pytest.raises(ValueError, match="constant-turn"):
            trk.getNees(truth, c=20, smooth=True, constantTurn=True)
        with pytest.raises(ValueError, match="aisAided"):
            trk.getNees(truth, c=20, smooth=True, ais=True)
        with pytest.raises(ValueError, match="cut-off"):
            trk.getNees(truth, c=0.0)
    finally:
        trk.close()
