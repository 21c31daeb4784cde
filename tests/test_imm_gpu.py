"""GPU: the interacting-multiple-model filter of track histories (`mht_imm_tracks`, `mht_imm_tracks_ct`, include/mht_amd.h;
pymht_amd.smoothing.imm_tracks*) and the drop-in path on top (Tracker.getModeProbabilities), against tests/imm_ref.py and against the
device filter and score of the same batches.

The criterion is the smoothers' (tests/test_filter_gpu.py), per output family (mu, x, P, ll): with the np.longdouble evaluation of the
reference as the truth, over the cells of a batch that are not NaN in it,
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
and e_dev <= 8 * max(e_np, eps64); the NaN cells are the truth's exactly and nObs is exact.  The float64 reference sets the scale, never
the device.  The host twin of the same header measures ratios of 0.49 - 1.80 on these batches (tests/test_imm_cpu.py); every test prints
the device's own, and tools/imm_cost.py writes them into profiles/imm_cost.txt.  Nothing here is larger than 35 tracks of 60 nodes,
except the 130 tracks of the place test.

The shapes: 35 tracks are two full wavefronts of sixteen quads and one of three; r < 4 leaves idle lanes in every quad; lengths 1 and 2
sit next to 60 in one wavefront; every fourth track is never detected and takes mu_j = cbar_j at every node; the three-mode Pi has
zeros, and the "blocked" chain a mode that is never entered."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as fr
import imm_ref as ref
import smooth_ref as sr

pytestmark = pytest.mark.gpu

PERIOD = 2.5
FACTOR = 8.0
SENTINEL = -7.0
N_TRACKS = 35
L_MAX = 64          # rows of the raw calls' arrays, more than any track has
SEED = 11


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


def _model(name):
    import importlib
    return importlib.import_module("pymht_amd.models." + name)


def _raw(ctx, model, tracks, L_max, modes, kind="linear", lens=None, work_bytes=None, nulls=(), model_nx=None, transition=None, seam=None, r=None):
    """One call of an IMM seam on `tracks` in the order given (no sorting: a track's quad is its index), in arrays of L_max rows, the
    outputs pre-filled with SENTINEL: (return code, dict mu [L_max, r, n], x [L_max, nx, n], P [L_max, ns, n], ll [n], nobs [n])."""
    import torch
    from pymht_amd.smoothing import _model_x
    lib, dev = ctx.lib, ctx.device
    Q, R, Pi, mu0 = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in modes]
    n, nx, nr = len(tracks), len(tracks[0][0]), len(Q)
    ns = nx * (nx + 1) // 2
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    zp, hp = np.zeros((L_max, 2, n)), np.zeros((L_max, n), dtype=np.uint8)
    for j, t in enumerate(tracks):
        z = np.asarray(t[2], dtype=np.float64)
        has = sr.detected(z)
        has[0] = False
        zp[:len(z), :, j], hp[:len(z), j] = np.where(has[:, None], z, 0.0), has
    arrays = {"x_init": up(np.stack([np.asarray(t[0], dtype=np.float64) for t in tracks], axis=1)),
              "P_init": up(np.stack([np.asarray(t[1], dtype=np.float64).ravel() for t in tracks], axis=1)), "z": up(zp), "h": up(hp)}
    full = lambda *shape, dtype=torch.float64: torch.full(shape, SENTINEL, dtype=dtype, device=dev)
    outs = {"mu": full(L_max, nr, n), "x": full(L_max, nx, n), "P": full(L_max, ns, n), "ll": full(n), "nobs": full(n, dtype=torch.int32)}
    host = {"Q": Q, "R": R, "Pi": Pi, "mu0": mu0}
    need = int(lib.mht_imm_work_bytes(nx, n, L_max, nr))
    work = torch.zeros(max(need, 512), dtype=torch.uint8, device=dev)
    mx, keep = _model_x(model, PERIOD, nx, kind == "ct")
    if model_nx is not None:
        mx.nx = model_nx
    if transition is not None:
        mx.transition = transition
    lens = np.array([len(t[2]) for t in tracks] if lens is None else lens, dtype=np.int32)
    ptr = lambda name: None if name in nulls else arrays[name].data_ptr()
    hp_ = lambda name: None if name in nulls else host[name].ctypes.data_as(C.c_void_p)
    op = lambda name: None if name in nulls else outs[name].data_ptr()
    torch.cuda.synchronize(dev)
    fn = getattr(lib, seam or {"linear": "mht_imm_tracks", "ct": "mht_imm_tracks_ct"}[kind])
    rc = fn(ctx.handle, C.byref(mx), n, L_max, None if "len" in nulls else lens.ctypes.data_as(C.c_void_p), ptr("x_init"), ptr("P_init"), ptr("z"),
            ptr("h"), nr if r is None else r, hp_("Q"), hp_("R"), hp_("Pi"), hp_("mu0"), op("mu"), op("x"), op("P"), op("ll"), op("nobs"),
            None if "work" in nulls else work.data_ptr(), need if work_bytes is None else work_bytes)
    torch.cuda.synchronize(dev)
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}


def _untouched(out):
    return all((v == SENTINEL).all() for v in out.values())


def _as_dicts(per, ll, nobs):
    return [dict(mu=m, x=x, P=P, ll=np.asarray(a), nobs=int(b)) for (m, x, P), a, b in zip(per, ll, nobs)]


def _hold(label, got, truth, f64):
    res = ref.ratios(got, truth, f64, ref.NAMES)
    print(label + ": " + " | ".join("%s e_dev %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert ref.same_nan(got, truth, ref.NAMES), "the NaN cells are not the truth's"
    assert [g["nobs"] for g in got] == [t["nobs"] for t in truth], "nObs is not the truth's"
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, "%s: e_dev %.3g > %g x max(e_np %.3g, eps)" % (k, e, FACTOR, e_np)


def _same_bits(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


CASES = [("linear", "pv", 1, 4), ("linear", "pv", 2, 4), ("linear", "pv", 3, 4), ("linear", "pv", 4, 4), ("linear", "pv", 2, 6), ("linear", "pv", 4, 6),
         ("linear", "pv", "blocked", 4), ("linear", "ca", 4, 4), ("linear", "ca", 4, 6), ("ct", "ct", 2, 4), ("ct", "ct", 2, 6)]


@pytest.mark.parametrize("kind,name,key,lib_nx", CASES)
def test_imm_accuracy_every_cell_written_and_the_python_layer_gives_the_raw_bits(ctxs, kind, name, key, lib_nx):
    """filter_ref.edge_batch: 35 tracks of 1, 2, 60, 7, 33 nodes in turn, every fourth never detected, under imm_ref.SETUPS[key].
    - the raw seam on arrays of 64 rows preset to a sentinel, the tracks in the order given: no cell keeps the sentinel, the rows behind
      a track's end are NaN, node 0 is (mu0, x_init, P_init), and the criterion holds against tests/imm_ref.py
    - the Python layer (which packs the batch sorted by length: other quads, other wavefronts) gives the raw call's bits per track
    Measured on an MI355X, both builds alike, ratios mu / x / P / ll:
        pv r=1 0 / 0.98 / 0.81 / 1.00       pv r=2 0.76 / 0.59 / 1.58 / 0.68    pv r=3 1.48 / 1.00 / 1.33 / 1.35
        pv r=4 1.16 / 1.50 / 1.40 / 1.00    pv blocked 0 / 0.98 / 0.81 / 1.00   ca r=4 2.35 / 1.64 / 0.68 / 0.70
        ct r=2 0.65 / 0.85 / 0.56 / 1.13    (profiles/imm_cost.txt has them with their e_np)"""
    from pymht_amd import smoothing
    assert np.finfo(np.longdouble).eps < 1e-18
    model, ctx = _model(name), ctxs[lib_nx]
    tracks, truth, f64 = ref.reference(kind, model, PERIOD, N_TRACKS, SEED, key)
    modes = ref.setup(model, PERIOD, key)
    nx, r = len(tracks[0][0]), len(modes[0])
    rc, out = _raw(ctx, model, tracks, L_MAX, modes, kind)
    assert rc == 0 and not any((v == SENTINEL).any() for v in out.values())
    got = []
    for j, t in enumerate(tracks):
        L = len(t[2])
        assert np.isnan(out["mu"][L:, :, j]).all() and np.isnan(out["x"][L:, :, j]).all() and np.isnan(out["P"][L:, :, j]).all()
        got.append(dict(mu=out["mu"][:L, :, j], x=out["x"][:L, :, j], P=fr.full(out["P"][:L, :, j], nx), ll=np.asarray(out["ll"][j]), nobs=int(out["nobs"][j])))
        assert np.array_equal(got[-1]["mu"][0], modes[3]) and np.array_equal(got[-1]["x"][0], t[0]) and np.array_equal(got[-1]["P"][0], t[1])
        assert L > 1 or (out["ll"][j] == 0.0 and not np.signbit(out["ll"][j]) and out["nobs"][j] == 0)
    _hold("IMM accuracy %s models/%s modes %s, %d-state build" % (kind, name, key, lib_nx), got, truth, f64)
    run = smoothing.imm_tracks_ct if kind == "ct" else smoothing.imm_tracks
    per, ll, nobs = run(model, PERIOD, tracks, *modes[:3], mu0=modes[3], ctx=ctx)
    assert ll.shape == (N_TRACKS,) and nobs.dtype == np.int32 and np.array_equal(ll, out["ll"]) and np.array_equal(nobs, out["nobs"])
    for g, (mu, x, P) in zip(got, per):
        assert mu.shape == g["mu"].shape and mu.dtype == x.dtype == P.dtype == np.float64
        assert _same_bits((mu, x, P), (g["mu"], g["x"], g["P"]))
    if key == "blocked":
        assert all((g["mu"][1:, 1] == 0.0).all() and np.isfinite(g["x"]).all() for g in got)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_place_in_the_batch_does_not_matter(ctxs, lib_nx):
    """130 tracks under three modes, and the same batch permuted: the same bits per track -- a track's figures do not depend on its
    quad, its wavefront or its neighbours; nor on being alone in a launch."""
    from pymht_amd.models import pv
    from pymht_amd.smoothing import imm_tracks
    ctx = ctxs[lib_nx]
    tracks = fr.edge_batch("linear", pv, PERIOD, 130, SEED)
    Q, R, Pi, mu0 = ref.setup(pv, PERIOD, 3)
    per, ll, nobs = imm_tracks(pv, PERIOD, tracks, Q, R, Pi, mu0=mu0, ctx=ctx)
    perm = np.random.default_rng(2).permutation(130)
    per2, ll2, nobs2 = imm_tracks(pv, PERIOD, [tracks[i] for i in perm], Q, R, Pi, mu0=mu0, ctx=ctx)
    assert all(_same_bits(per2[j], per[i]) for j, i in enumerate(perm))
    assert np.array_equal(ll2, ll[perm]) and np.array_equal(nobs2, nobs[perm]) and np.isfinite(ll).all() and nobs.sum() > 1000
    one, ll1, nobs1 = imm_tracks(pv, PERIOD, [tracks[127]], Q, R, Pi, mu0=mu0, ctx=ctx)
    assert _same_bits(one[0], per[127]) and ll1[0] == ll[127] and nobs1[0] == nobs[127]
    assert all(np.abs(p[0].sum(axis=1) - 1.0).max() < 1e-12 for p in per)


@pytest.mark.parametrize("name,kind,lib_nx", [("pv", "linear", 4), ("pv", "linear", 6), ("ca", "linear", 6), ("ct", "ct", 6)])
def test_one_mode_is_the_filter_and_the_score_bit_for_bit(ctxs, name, kind, lib_nx):
    """Pi = [[1]] with the model's own Q and R: mu is all ones, x and P are filter_tracks' bits, ll and nObs score_tracks', on the same
    context."""
    from pymht_amd import smoothing
    model, ctx = _model(name), ctxs[lib_nx]
    tracks = fr.edge_batch(kind, model, PERIOD, N_TRACKS, SEED)
    Q, R, Pi, mu0 = smoothing.imm_modes(model, PERIOD, (1.0,))
    imm, filt, score = ((smoothing.imm_tracks_ct, smoothing.filter_tracks_ct, smoothing.score_tracks_ct) if kind == "ct" else
                        (smoothing.imm_tracks, smoothing.filter_tracks, smoothing.score_tracks))
    per, ll, nobs = imm(model, PERIOD, tracks, Q, R, Pi, ctx=ctx)
    want, sc = filt(model, PERIOD, tracks, ctx=ctx), score(model, PERIOD, tracks, ctx=ctx)
    for (mu, x, P), (xf, Pf), a, b, s in zip(per, want, ll, nobs, sc):
        assert (mu == 1.0).all() and np.array_equal(x, xf) and np.array_equal(P, Pf)
        assert a == s[0] and b == s[2]
    assert nobs.sum() > 200


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_a_mode_that_is_no_covariance_poisons_its_tracks_only(ctxs, lib_nx):
    """Mode 1 with an indefinite R (det S < 0 at every plot): NaN ll for the tracks with a plot; never-detected tracks, and tracks of
    one node, keep ll = 0.0 exactly.  The same call with mode 1 repaired is finite everywhere."""
    from pymht_amd.models import pv
    from pymht_amd.smoothing import imm_tracks
    ctx = ctxs[lib_nx]
    tracks = fr.edge_batch("linear", pv, PERIOD, N_TRACKS, SEED)
    Q, R, Pi, mu0 = ref.setup(pv, PERIOD, 2)
    bad = R.copy()
    bad[1] = np.diag([-1e9, 1.0])
    per, ll, nobs = imm_tracks(pv, PERIOD, tracks, Q, bad, Pi, mu0=mu0, ctx=ctx)
    scored = nobs > 0
    assert scored.sum() >= 15 and (~scored).sum() >= 10 and np.isnan(ll[scored]).all()
    assert (ll[~scored] == 0.0).all() and not np.signbit(ll[~scored]).any()
    assert all(np.isfinite(p[1]).all() for p, s in zip(per, scored) if not s)
    per, ll, nobs2 = imm_tracks(pv, PERIOD, tracks, Q, R, Pi, mu0=mu0, ctx=ctx)
    assert np.isfinite(ll).all() and np.array_equal(nobs, nobs2) and all(np.isfinite(p[0]).all() for p in per)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_raw_abi_errors_and_the_calls_behind_them(ctxs, lib_nx):
    """A null array, n_modes outside 1 .. 4, a length outside 1 .. L_max, a short workspace, a wrong nx or transition for the seam, an entry
    of Pi or mu0 outside [0, 1], a row that does not add up to 1: MHT_E_INVALID each, with the sentinel in the outputs untouched; an empty
    batch is MHT_OK and writes nothing; the call behind them on the same context is right."""
    import torch
    from pymht_amd import _lib
    from pymht_amd.models import ct, pv
    from pymht_amd.smoothing import _model_x, imm_tracks
    import smooth_ct_ref as cr
    ctx = ctxs[lib_nx]
    lib = ctx.lib
    tracks = sr.make_batch(pv, PERIOD, [4, 3, 1], seed=2, p_detect=1.0)
    ct_tracks = cr.make_batch(ct, PERIOD, [4, 3, 1], seed=2)
    modes = ref.setup(pv, PERIOD, 2)
    ct_modes = ref.setup(ct, PERIOD, 2)
    need = int(lib.mht_imm_work_bytes(4, 3, 4, 2))
    assert need == 512
    Q, R, Pi, mu0 = modes
    bad = [dict(nulls=(k,)) for k in ("len", "x_init", "P_init", "z", "h", "Q", "R", "Pi", "mu0", "mu", "x", "P", "ll", "nobs", "work")]
    bad += [dict(r=0), dict(r=5), dict(r=-1), dict(lens=[4, 0, 1]), dict(lens=[4, 5, 1]), dict(work_bytes=need - 1), dict(model_nx=5),
            dict(transition=1), dict(seam="mht_imm_tracks_ct"), dict(seam="mht_imm_tracks_ct", transition=1)]      # (ct: nx 4 is not its model)
    for kw in bad:
        rc, out = _raw(ctx, pv, tracks, 4, modes, **kw)
        assert rc == _lib.MHT_E_INVALID and lib.mht_last_error(), kw
        assert _untouched(out), kw
    for Pi_bad, mu_bad in (([[0.5, 0.6], [0.5, 0.5]], mu0), ([[1.5, -0.5], [0.5, 0.5]], mu0), ([[0.5, 0.5], [np.nan, 1.0]], mu0),
                           ([[0.5, 0.5], [0.5, 0.5 - 1e-8]], mu0), (Pi, [0.5, 0.6]), (Pi, [1.5, -0.5]), (Pi, [np.nan, 1.0])):
        rc, out = _raw(ctx, pv, tracks, 4, (Q, R, Pi_bad, mu_bad))
        assert rc == _lib.MHT_E_INVALID and lib.mht_last_error() and _untouched(out), (Pi_bad, mu_bad)
    for kw in (dict(transition=0), dict(lens=[4, 3, 9]), dict(r=5)):
        rc, out = _raw(ctx, ct, ct_tracks, 4, ct_modes, "ct", **kw)
        assert rc == _lib.MHT_E_INVALID and _untouched(out), kw
    mx, keep = _model_x(pv, PERIOD, 4, False)
    torch.cuda.synchronize(ctx.device)
    assert lib.mht_imm_tracks(ctx.handle, C.byref(mx), 0, 4, *([None] * 5), 2, *([None] * 10), 0) == _lib.MHT_OK
    rc, out = _raw(ctx, pv, tracks, 4, (Q, R, [[0.5, 0.5], [0.5, 0.5 - 1e-10]], mu0))      # (within 1e-9 of 1: taken)
    assert rc == _lib.MHT_OK
    rc, out = _raw(ctx, pv, tracks, 4, modes)
    assert rc == _lib.MHT_OK and not any((v == SENTINEL).any() for v in out.values())
    per, ll, nobs = imm_tracks(pv, PERIOD, tracks, Q, R, Pi, mu0=mu0, ctx=ctx)
    for j, (mu, x, P) in enumerate(per):
        L = len(mu)
        assert np.array_equal(out["mu"][:L, :, j], mu) and np.array_equal(out["x"][:L, :, j], x) and np.array_equal(fr.full(out["P"][:L, :, j], 4), P)
        assert np.isnan(out["x"][L:, :, j]).all()
    assert np.array_equal(out["ll"], ll) and np.array_equal(out["nobs"], nobs) and nobs.tolist() == [3, 2, 0]


def test_drop_in_path_gives_the_mode_probabilities_of_a_run():
    """A dozen scans over six preinitialised targets on models/pv: getModeProbabilities has one entry per track with a row per node of
    its history, the rows of mu add up to 1 within 1e-12 (the NumPy prototype's worst: 3.5e-15); with the one scale (1.0,) it is
    getFilteredTracks and getTrackLikelihoods bit for bit; a node's own call is its entry; a constant-turn tracker refuses without its
    switch."""
    from pymht_amd.models import ct, pv
    from pymht_amd.pyTarget import Target
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
        got = trk.getModeProbabilities(terminated=True)
        assert len(got) == len(nodes) and len(live) > 0 and len(trk.getModeProbabilities()) == len(live)
        worst = 0.0
        for d, node in zip(got, nodes):
            L = len(node.backtrackNodes())
            assert sorted(d) == ["P", "logLikelihood", "mu", "nObs", "x"]
            assert d["mu"].shape == (L, 2) and d["x"].shape == (L, 4) and d["P"].shape == (L, 4, 4)
            assert np.isfinite(d["mu"]).all() and np.isfinite(d["x"]).all() and np.isfinite(d["P"]).all() and np.isfinite(d["logLikelihood"])
            worst = max(worst, float(np.abs(d["mu"].sum(axis=1) - 1.0).max()))
        print("rows of mu add up to 1 within %.3g" % worst)
        assert worst < 1e-12
        three = trk.getModeProbabilities(qScales=(0.25, 1.0, 16.0), stay=0.9)
        assert all(d["mu"].shape[1] == 3 for d in three)
        one = trk.getModeProbabilities(qScales=(1.0,), terminated=True)
        filt, score = trk.getFilteredTracks(terminated=True), trk.getTrackLikelihoods(terminated=True)
        for d, (xf, Pf), s in zip(one, filt, score):
            assert (d["mu"] == 1.0).all() and np.array_equal(d["x"], xf) and np.array_equal(d["P"], Pf)
            assert d["logLikelihood"] == s[0] and d["nObs"] == s[2]
        i = max(range(len(nodes)), key=lambda j: len(got[j]["mu"]))
        own = nodes[i].getModeProbabilities(trk.radarPeriod)
        assert len(got[i]["mu"]) >= 10 and all(np.array_equal(own[k], got[i][k]) for k in ("mu", "x", "P"))
        assert own["logLikelihood"] == got[i]["logLikelihood"] and own["nObs"] == got[i]["nObs"]
        with pytest.raises(ValueError, match="constant-turn"):
            trk.getModeProbabilities(constantTurn=True)
        with pytest.raises(ValueError):
            trk.getModeProbabilities(qScales=(1.0, 2.0, 3.0, 4.0, 5.0))
    finally:
        trk.close()
    turning = Tracker(ct, PERIOD, 1e-7, 1e-4, P_d=0.9, N=4, eta2=5.99, useInitiator=False)
    try:
        with pytest.raises(NotImplementedError, match="ct"):
            turning.getModeProbabilities()
        assert turning.getModeProbabilities(constantTurn=True) == []
    finally:
        turning.close()
