"""GPU: the device trace of track histories (`mht_trace_tracks`, `mht_trace_tracks_ct`, `mht_trace_tracks_ais`, include/mht_amd.h;
pymht_amd.smoothing.trace_tracks*) and the drop-in path on top (Tracker.getTrackInnovations, getConsistency), against
tests/smooth_trace_ref.py and against the device score of the same batches.

The criterion is the smoothers' (tests/test_smooth_gpu.py), per output family (v, S, nis, ll, and vAis, SAis, nisAis, llAis): with the
np.longdouble evaluation of the reference as the truth, over the cells of a batch that are not NaN in it,
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
and e_dev <= 8 * max(e_np, eps64); the NaN cells are the truth's exactly.  The float64 reference sets the scale, never the device.  The
host twin of the same header measures ratios of 0.42 - 2.31 on these batches (tests/test_smooth_trace_cpu.py); every test prints the
device's own -- measured on an MI355X, both builds alike: pv 1.00 / 0.51 / 1.00 / 1.00 (v / S / nis / ll), ca 0.91 / 2.31 / 0.75 / 1.00,
ct 1.00 / 0.84 / 1.00 / 1.00, AIS 0.81 / 0.45 / 1.19 / 1.05 and 1.11 / 0.42 / 1.00 / 1.28 for its message families -- and
tools/smooth_trace_cost.py writes them into profiles/smooth_trace_cost.txt.  Nothing here is larger than 130 tracks
of 60 nodes."""
import ctypes as C

import numpy as np
import pytest

import smooth_ais_ref as ar
import smooth_ct_ref as cr
import smooth_ref as sr
import smooth_trace_ref as ref

pytestmark = pytest.mark.gpu

PERIOD = 2.5
FACTOR = 8.0
SENTINEL = -7.0
EDGE_LENGTHS = [1, 2, 60, 7, 33]      # cycled over a batch: the shortest tracks next to the longest in every wavefront


@pytest.fixture(scope="module")
def ctxs():
    """One context per library build: the seams take nx at run time, so both builds run every model."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (pymht_amd has no CPU fallback)")
    from pymht_amd.device import Context
    c = {4: Context(0, nx=4), 6: Context(0, nx=6)}
    yield c
    for v in c.values():
        v.close()


def _hold(label, got, truth, f64, names):
    res = ref.ratios(got, truth, f64, names)
    print(label + ": " + " | ".join("%s e_dev %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert ref.same_nan(got, truth, names), "the NaN cells are not the truth's"
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, "%s: e_dev %.3g > %g x max(e_np %.3g, eps)" % (k, e, FACTOR, e_np)


def _sums_are_the_score(traces, scores):
    """Per track, the trace added up in node order (a Python loop; llAis in front of ll at a node with both) against the device
    score's tuple (ll, nis, nObs[, nisAis, nAis]): the same bits."""
    assert len(traces) == len(scores) > 0
    for tr, sc in zip(traces, scores):
        s = ref.resum(tr)
        assert tr["ll"].dtype == np.float64 and tr["nis"].dtype == np.float64
        want = [s["ll"], s["nis"], s["nobs"]] + ([s["nis_ais"], s["nais"]] if "message" in tr else [])
        assert np.array_equal(np.array(want, dtype=np.float64), np.array(sc, dtype=np.float64)), (want, sc)


def _same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_linear_accuracy_and_sums_against_the_score(ctxs, name, lib_nx):
    """smooth_em_ref.accuracy_batch, 33 tracks of 1 .. 60 nodes: v, S, nis, ll against the longdouble truth, and added up against
    score_tracks on the same batch and context, bit for bit."""
    from pymht_amd.models import pv, ca
    from pymht_amd.smoothing import score_tracks, trace_tracks
    assert np.finfo(np.longdouble).eps < 1e-18
    model = {"pv": pv, "ca": ca}[name]
    tracks, truth, f64 = ref.reference("linear", model, PERIOD)
    dev = trace_tracks(model, PERIOD, tracks, ctx=ctxs[lib_nx])
    assert all(sorted(d) == ["S", "ll", "nis", "observed", "v"] and d["observed"].dtype == bool for d in dev)
    _hold("trace accuracy models/%s, %d-state build" % (name, lib_nx), dev, truth, f64, ref.RADAR)
    _sums_are_the_score(dev, score_tracks(model, PERIOD, tracks, ctx=ctxs[lib_nx]))
    assert all(np.array_equal(d["S"], d["S"].transpose(0, 2, 1), equal_nan=True) for d in dev)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_constant_turn_accuracy_and_sums_against_the_score(ctxs, lib_nx):
    """A smooth_ct_ref.make_batch of the linear batch's lengths."""
    from pymht_amd.models import ct
    from pymht_amd.smoothing import score_tracks_ct, trace_tracks_ct
    tracks, truth, f64 = ref.reference("ct", ct, PERIOD)
    dev = trace_tracks_ct(ct, PERIOD, tracks, ctx=ctxs[lib_nx])
    _hold("trace accuracy models/ct, %d-state build" % lib_nx, dev, truth, f64, ref.RADAR)
    _sums_are_the_score(dev, score_tracks_ct(ct, PERIOD, tracks, ctx=ctxs[lib_nx]))


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_ais_accuracy_and_sums_against_the_score(ctxs, lib_nx):
    """smooth_ais_ref.accuracy_batch cut to at most 60 nodes a track: the radar and the message families, and ll, nis, nObs, nisAis,
    nAis added up against score_tracks_ais; without its messages a batch is the linear trace, bit for bit."""
    from pymht_amd.smoothing import score_tracks_ais, trace_tracks, trace_tracks_ais
    model, _ = ref.ais_batch()
    tracks, truth, f64 = ref.reference("ais", model, PERIOD)
    dev = trace_tracks_ais(model, PERIOD, tracks, ctx=ctxs[lib_nx])
    assert all(len(d) == 10 and d["message"].dtype == bool for d in dev)
    _hold("trace accuracy AIS, %d-state build" % lib_nx, dev, truth, f64, ref.RADAR + ref.AIS)
    scores = score_tracks_ais(model, PERIOD, tracks, ctx=ctxs[lib_nx])
    _sums_are_the_score(dev, scores)
    assert sum(s[4] for s in scores) > 300
    assert all(np.array_equal(d["SAis"], d["SAis"].transpose(0, 2, 1), equal_nan=True) for d in dev)
    plain = trace_tracks_ais(model, PERIOD, [t[:3] + ([None] * len(t[2]),) for t in tracks], ctx=ctxs[lib_nx])
    lin = trace_tracks(model, PERIOD, [t[:3] for t in tracks], ctx=ctxs[lib_nx])
    for p, q in zip(plain, lin):
        assert all(np.array_equal(p[k], q[k], equal_nan=True) for k in q)
        assert not p["message"].any() and all(np.isnan(p[k]).all() for k in ref.AIS)


def _raw(ctx, model, tracks, L_max, kind="linear", lens=None, work_bytes=None, nulls=(), model_nx=None, transition=None, seam=None):
    """One call of a trace seam on `tracks` in the order given (no sorting: a track's lane is its index), in arrays of L_max rows, the
    outputs pre-filled with SENTINEL: (return code, radar [L_max, 7, n], ais [L_max, 16, n] or None) as NumPy arrays."""
    import torch
    from pymht_amd.smoothing import _ais_inputs, _model_x
    lib, dev = ctx.lib, ctx.device
    n, nx = len(tracks), len(tracks[0][0])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    zp, hp = np.zeros((L_max, 2, n)), np.zeros((L_max, n), dtype=np.uint8)
    for j, t in enumerate(tracks):
        z = np.asarray(t[2], dtype=np.float64)
        has = sr.detected(z)
        has[0] = False
        zp[:len(z), :, j], hp[:len(z), j] = np.where(has[:, None], z, 0.0), has
    arrays = {"x": up(np.stack([np.asarray(t[0], dtype=np.float64) for t in tracks], axis=1)),
              "P": up(np.stack([np.asarray(t[1], dtype=np.float64).ravel() for t in tracks], axis=1)), "z": up(zp), "h": up(hp)}
    outs = [torch.full((L_max, 7, n), SENTINEL, dtype=torch.float64, device=dev)]
    extra = []
    if kind == "ais":
        per_track, legs = _ais_inputs(model, tracks)
        kp, mp, rp, lp = hp.copy(), np.zeros((L_max, 4, n)), np.ones((L_max, n)), np.zeros((L_max, n), dtype=np.int32)
        for j, (has_m, msg, r, leg) in enumerate(per_track):
            L = len(has_m)
            kp[:L, j] += 2 * has_m.astype(np.uint8)
            mp[:L, :, j], rp[:L, j], lp[:L, j] = msg, r, leg
        arrays.update(kind=up(kp), m=up(mp), r=up(rp), leg=up(lp), legs=up(legs if len(legs) else np.zeros((1, 52))))
        extra = [arrays[k].data_ptr() for k in ("kind", "m", "r", "leg", "legs")] + [len(legs)]
        outs.append(torch.full((L_max, 16, n), SENTINEL, dtype=torch.float64, device=dev))
    need = int(lib.mht_trace_work_bytes(nx, n, L_max))
    work = torch.zeros(max(need, 256), dtype=torch.uint8, device=dev)
    mx, keep = _model_x(model, PERIOD, nx, kind == "ct")
    if model_nx is not None:
        mx.nx = model_nx
    if transition is not None:
        mx.transition = transition
    lens = np.array([len(t[2]) for t in tracks] if lens is None else lens, dtype=np.int32)
    ptr = lambda name: None if name in nulls else arrays[name].data_ptr()
    torch.cuda.synchronize(dev)
    fn = getattr(lib, seam or {"linear": "mht_trace_tracks", "ct": "mht_trace_tracks_ct", "ais": "mht_trace_tracks_ais"}[kind])
    rc = fn(ctx.handle, C.byref(mx), n, L_max, None if "len" in nulls else lens.ctypes.data_as(C.c_void_p), ptr("x"), ptr("P"), ptr("z"), ptr("h"),
            *extra, *(None if "out" in nulls else o.data_ptr() for o in outs), None if "work" in nulls else work.data_ptr(),
            need if work_bytes is None else work_bytes)
    torch.cuda.synchronize(dev)
    got = [o.cpu().numpy() for o in outs]
    return rc, got[0], got[1] if kind == "ais" else None


def _edge_batch(model, n, seed, make=sr.make_batch):
    """n tracks of lengths 1, 2, 60, 7, 33 in turn; every fourth is never detected."""
    lengths = [EDGE_LENGTHS[i % len(EDGE_LENGTHS)] for i in range(n)]
    p_detect = [0.0 if i % 4 == 3 else 0.8 for i in range(n)]
    return make(model, PERIOD, lengths, seed=seed, p_detect=p_detect)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_every_cell_is_written_for_every_batch_size(ctxs, n):
    """One track, a wavefront less one, a wavefront, one more, and two and a bit, lengths 1 and 2 next to 60, tracks never detected, in
    arrays of L_max = 64 > every length filled with a sentinel: no cell keeps it, the rows behind a track's end and of nodes without a
    plot are NaN, and what is there is trace_tracks' bits (which packs the batch sorted by length) and the float64 reference's numbers."""
    from pymht_amd.models import ca, pv
    from pymht_amd.smoothing import trace_tracks, trace_tracks_ais
    for model, kind, lib_nx in ((pv, "linear", 4), (ca, "linear", 6), (pv, "ais", 4)):
        ctx = ctxs[lib_nx]
        tracks = _edge_batch(model, n, seed=40 + n) if kind == "linear" else _edge_batch(model, n, seed=40 + n, make=ar.make_batch)
        rc, radar, ais = _raw(ctx, model, tracks, 64, kind)
        assert rc == 0
        assert not (radar == SENTINEL).any() and (ais is None or not (ais == SENTINEL).any())
        dev = (trace_tracks if kind == "linear" else trace_tracks_ais)(model, PERIOD, tracks, ctx=ctx)
        mats = sr.model_matrices(model, PERIOD)
        for j, (t, d) in enumerate(zip(tracks, dev)):
            L = len(t[2])
            assert np.isnan(radar[L:, :, j]).all() and np.isnan(radar[0, :, j]).all()
            assert np.array_equal(radar[:L, 0:2, j], d["v"], equal_nan=True) and np.array_equal(radar[:L, 5, j], d["nis"], equal_nan=True)
            assert np.array_equal(radar[:L, 6, j], d["ll"], equal_nan=True) and np.array_equal(radar[:L, 2:5, j], d["S"].reshape(L, 4)[:, [0, 1, 3]], equal_nan=True)
            assert np.array_equal(np.isnan(d["nis"]), ~d["observed"]) and np.array_equal(np.isnan(d["v"]).any(axis=1), ~d["observed"])
            if kind == "ais":
                assert np.isnan(ais[L:, :, j]).all() and np.isnan(ais[0, :, j]).all()
                assert np.array_equal(ais[:L, 0:4, j], d["vAis"], equal_nan=True) and np.array_equal(ais[:L, 15, j], d["llAis"], equal_nan=True)
                assert np.array_equal(np.isnan(d["nisAis"]), ~d["message"])
                f = ref.trace_ais(model, PERIOD, *t)
            else:
                f = ref.trace(*mats, *t)
            assert np.array_equal(d["observed"], f["observed"])
            for k in ref.RADAR + (ref.AIS if kind == "ais" else ()):
                assert np.allclose(d[k], f[k], rtol=1e-9, atol=1e-9, equal_nan=True), (j, k)
        assert n < 4 or any(not d["observed"].any() and len(d["ll"]) == 60 for d in dev)      # (a long track never detected)


def test_a_track_gives_the_same_bits_alone_and_anywhere_in_a_batch(ctxs):
    """One track alone and in lanes 0, 63, 64 and 129 of a batch of 130; and a constant-turn and an AIS batch of 70 permuted."""
    from pymht_amd.models import ct, pv
    from pymht_amd.smoothing import trace_tracks_ais, trace_tracks_ct
    ctx = ctxs[4]
    base = _edge_batch(pv, 130, seed=7)
    (mine,) = sr.make_batch(pv, PERIOD, [47], seed=8, p_detect=0.8)
    rc, alone, _ = _raw(ctx, pv, [mine], 60)
    assert rc == 0 and np.isfinite(alone[:47, 6, 0]).sum() > 20
    for lane in (0, 63, 64, 129):
        batch = list(base)
        batch[lane] = mine
        rc, radar, _ = _raw(ctx, pv, batch, 60)
        assert rc == 0 and np.array_equal(radar[:, :, lane], alone[:, :, 0], equal_nan=True), lane
    lengths = [EDGE_LENGTHS[i % 5] for i in range(70)]
    perm = np.random.default_rng(2).permutation(70)
    for trace, model, tracks in ((trace_tracks_ct, ct, cr.make_batch(ct, PERIOD, lengths, seed=31)),
                                 (trace_tracks_ais, pv, ar.make_batch(pv, PERIOD, lengths, seed=37))):
        got = trace(model, PERIOD, tracks, ctx=ctxs[6])
        again = trace(model, PERIOD, [tracks[i] for i in perm], ctx=ctxs[6])
        assert all(_same_bits(again[j], got[i]) for j, i in enumerate(perm))
        assert _same_bits(trace(model, PERIOD, [tracks[69]], ctx=ctxs[6])[0], got[69])


def test_a_model_that_is_no_covariance_poisons_its_nodes_and_no_other(ctxs):
    """R = diag(-1e4, 1) under models/pv: det S is negative exactly where the predicted position variance lies below 1e4.  Track 0
    (P_init = P0, two nodes) is poisoned at its plot; track 1 (position variances of 1e6, three nodes) is fine at node 1 and -- its
    update there, with that R, leaves a variance near -1e4 -- poisoned at node 2; track 2 (the same P_init, two nodes) is fine.  v and S are finite
    at every plot; nis and ll are NaN where det S <= 0 and nowhere else; the score of the same batch is NaN for tracks 0 and 1 only."""
    from pymht_amd.models import pv
    from pymht_amd.smoothing import score_tracks, trace_tracks

    class Broken:
        __name__ = "broken"
        Phi, C_RADAR, Q, P0 = staticmethod(pv.Phi), pv.C_RADAR, staticmethod(pv.Q), pv.P0
        R_RADAR = staticmethod(lambda: np.diag([-1e4, 1.0]))
    a, b, c = sr.make_batch(pv, PERIOD, [2, 3, 2], seed=5, p_detect=1.0)
    big = np.diag([1e6, 1e6, 1.875, 1.875])
    tracks = [a, (b[0], big, b[2]), (c[0], big, c[2])]
    dev = trace_tracks(Broken, PERIOD, tracks, ctx=ctxs[4])
    for d in dev:
        obs = d["observed"]
        assert obs[1:].all() and np.isfinite(d["v"][obs]).all() and np.isfinite(d["S"][obs]).all()
        det = d["S"][:, 0, 0] * d["S"][:, 1, 1] - d["S"][:, 0, 1] ** 2
        assert np.array_equal(np.isnan(d["nis"])[obs], (det <= 0)[obs]) and np.array_equal(np.isnan(d["ll"]), np.isnan(d["nis"]))
    assert np.isnan(dev[0]["nis"][1]) and np.isfinite(dev[1]["nis"][1]) and np.isnan(dev[1]["nis"][2]) and np.isfinite(dev[2]["ll"][1])
    scores = score_tracks(Broken, PERIOD, tracks, ctx=ctxs[4])
    assert np.isnan(scores[0][0]) and np.isnan(scores[1][0]) and np.isfinite(scores[2][0])
    assert scores[2][0] == dev[2]["ll"][1] and scores[2][1] == dev[2]["nis"][1]


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_raw_abi_errors_and_the_calls_behind_them(ctxs, lib_nx):
    """A null array, a length outside 1 .. L_max, a short workspace, a wrong nx or transition for the seam: MHT_E_INVALID each, with the
    sentinel in the outputs untouched; an empty batch is MHT_OK and writes nothing; the call behind them on the same context is right."""
    from pymht_amd import _lib
    from pymht_amd.models import ct, pv
    from pymht_amd.smoothing import _model_x, trace_tracks
    ctx = ctxs[lib_nx]
    lib = ctx.lib
    tracks = sr.make_batch(pv, PERIOD, [4, 3, 1], seed=2, p_detect=1.0)
    ais_tracks = [t + ([None] * len(t[2]),) for t in tracks]
    ct_tracks = cr.make_batch(ct, PERIOD, [4, 3, 1], seed=2)
    need = int(lib.mht_trace_work_bytes(4, 3, 4))
    assert need == 256
    bad = [dict(nulls=("len",)), dict(nulls=("x",)), dict(nulls=("z",)), dict(nulls=("h",)), dict(nulls=("out",)), dict(nulls=("work",)),
           dict(lens=[4, 0, 1]), dict(lens=[4, 5, 1]), dict(work_bytes=need - 1), dict(model_nx=5), dict(transition=1),
           dict(seam="mht_trace_tracks_ct"), dict(seam="mht_trace_tracks_ct", transition=1)]      # (ct: nx 4 is not its model)
    for kw in bad:
        rc, radar, _ = _raw(ctx, pv, tracks, 4, **kw)
        assert rc == _lib.MHT_E_INVALID and lib.mht_last_error(), kw
        assert (radar == SENTINEL).all(), kw
    for kw in (dict(model_nx=6), dict(transition=1), dict(nulls=("out",)), dict(work_bytes=need - 1)):
        rc, radar, ais = _raw(ctx, pv, ais_tracks, 4, "ais", **kw)
        assert rc == _lib.MHT_E_INVALID and (radar == SENTINEL).all() and (ais == SENTINEL).all(), kw
    for kw in (dict(transition=0), dict(lens=[4, 3, 9])):
        rc, radar, _ = _raw(ctx, ct, ct_tracks, 4, "ct", **kw)
        assert rc == _lib.MHT_E_INVALID and (radar == SENTINEL).all(), kw
    # an empty batch: nothing to do, nothing touched -- the arrays of the call are not read
    import torch
    mx, keep = _model_x(pv, PERIOD, 4, False)
    torch.cuda.synchronize(ctx.device)
    assert lib.mht_trace_tracks(ctx.handle, C.byref(mx), 0, 4, None, None, None, None, None, None, None, 0) == _lib.MHT_OK
    rc, radar, _ = _raw(ctx, pv, tracks, 4)
    assert rc == _lib.MHT_OK and not (radar == SENTINEL).any()
    want = trace_tracks(pv, PERIOD, tracks, ctx=ctx)
    for j, d in enumerate(want):
        L = len(d["ll"])
        assert np.array_equal(radar[:L, 6, j], d["ll"], equal_nan=True) and np.isnan(radar[L:, :, j]).all()
    assert want[0]["observed"].tolist() == [False, True, True, True] and len(want[2]["ll"]) == 1


def test_drop_in_path_traces_the_tracks_of_a_run():
    """A dozen scans over six preinitialised targets on models/pv: getTrackInnovations is trace_nodes on the tracker's nodes, adds up
    to getTrackLikelihoods bit for bit, and getConsistency gives finite statistics; a constant-turn tracker refuses without its switch."""
    from pymht_amd.models import ct, pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.smoothing import consistency, trace_nodes
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    from pymht_amd.utils.scenario import make_scenario
    sc = make_scenario(T=6, radius=2000.0, lambda_phi=2e-6, n_scans=12, P_d=0.9, seed=4711)
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=5, eta2=5.99, useInitiator=False)
    try:
        for x in sc["x0"]:
            trk.initiateTarget(Target(sc["t0"], None, x.copy(), pv.P0, status="preinitialized"))
        for zk, tk in zip(sc["scans"], sc["times"]):
            trk.addMeasurementList(MeasurementList(float(tk), zk))
        live = list(trk.getTrackNodes())
        nodes = live + list(trk.__terminatedTargets__)
        got = trk.getTrackInnovations(terminated=True)
        assert len(got) == len(nodes) and len(live) > 0 and len(trk.getTrackInnovations()) == len(live)
        direct = trace_nodes(pv, trk.radarPeriod, nodes, ctx=trk._ctx)
        assert all(_same_bits(g, d) for g, d in zip(got, direct))
        assert all(len(g["ll"]) == len(node.backtrackNodes()) for g, node in zip(got, nodes))
        _sums_are_the_score(got, trk.getTrackLikelihoods(terminated=True))
        assert sum(int(g["observed"].sum()) for g in got) >= 30
        i = max(range(len(nodes)), key=lambda j: len(got[j]["ll"]))
        assert _same_bits(nodes[i].getTrackInnovations(trk.radarPeriod), got[i])
        c = trk.getConsistency(terminated=True)
        assert c == consistency(got) and c["nObs"] >= 30 and c["nPairs"] > 0
        assert all(np.isfinite(c[k]) for k in ("nisMean", "outlierFraction", "rho1", "rho1Bound")) and np.isfinite(c["nisInterval"]).all()
        assert c["nisInside"] in (True, False) and c["white"] in (True, False)
        with pytest.raises(ValueError, match="constant-turn"):
            trk.getTrackInnovations(constantTurn=True)
        with pytest.raises(ValueError, match="aisAided"):
            trk.getConsistency(ais=True)
    finally:
        trk.close()
    turning = Tracker(ct, PERIOD, 1e-7, 1e-4, P_d=0.9, N=4, eta2=5.99, useInitiator=False)
    try:
        with pytest.raises(NotImplementedError, match="ct"):
            turning.getTrackInnovations()
        with pytest.raises(NotImplementedError, match="ct"):
            turning.getConsistency()
        assert turning.getTrackInnovations(constantTurn=True) == []
    finally:
        turning.close()
