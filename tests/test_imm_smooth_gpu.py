"""GPU: the fixed-interval IMM smoother of track histories (`mht_imm_smooth_tracks`, `mht_imm_smooth_tracks_ct`, include/mht_amd.h;
pymht_amd.smoothing.imm_smooth_tracks*) and the drop-in path on top (Tracker.getSmoothModeProbabilities, getSmoothTracks(imm=..)),
against tests/imm_smooth_ref.py and against the device's own IMM filter and smoothers on the same batches.

The criterion is tests/test_imm_gpu.py's, per output family (mus, muf, xs, Ps, ll): with the np.longdouble evaluation of the reference as
the truth, over the cells of a batch that are not NaN in it,
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
and e_dev <= 8 * max(e_np, eps64); the NaN cells are the truth's exactly and nObs is exact.  The float64 reference sets the scale, never
the device.  The host twin of the same header measures ratios of 0.43 - 2.42 on these batches (tests/test_imm_smooth_cpu.py); every test
prints the device's own.  The shapes are tests/test_imm_gpu.py's: 35 tracks are two full wavefronts of sixteen quads and one of three;
r < 4 leaves idle lanes in every quad; lengths 1 and 2 sit next to 60 in one wavefront; every fourth track is never detected; the
three-mode Pi has zeros, and the "blocked" chain a mode that is never entered.

The bit properties are claims about the arithmetic: with one mode the smoother's own bits; the filter's bits going forward and at the
last node; with an identity chain from a certain mode the smoother's bits under that mode; no dependence on the place in the batch."""
import ctypes as C
import types

import numpy as np
import pytest

import filter_ref as fr
import imm_ref as ir
import imm_smooth_ref as ref
import smooth_ref as sr

pytestmark = pytest.mark.gpu

PERIOD = 2.5
FACTOR = 8.0
SENTINEL = -7.0
N_TRACKS = 35
L_MAX = 64          # rows of the raw calls' arrays, more than any track has
SEED = 11
KEYS = ("mu", "muFiltered", "x", "P")


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
    """One call of an IMM smoother seam on `tracks` in the order given (no sorting: a track's quad is its index), in arrays of L_max rows,
    the outputs pre-filled with SENTINEL: (return code, dict mus, muf [L_max, r, n], xs [L_max, nx, n], Ps [L_max, ns, n], ll [n], nobs [n])."""
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
    outs = {"mus": full(L_max, nr, n), "xs": full(L_max, nx, n), "Ps": full(L_max, ns, n), "muf": full(L_max, nr, n), "ll": full(n),
            "nobs": full(n, dtype=torch.int32)}
    host = {"Q": Q, "R": R, "Pi": Pi, "mu0": mu0}
    need = int(lib.mht_imm_smooth_work_bytes(nx, n, L_max, nr))
    assert need == int(lib.mht_imm_work_bytes(nx, n, L_max, nr)) + (L_max * nr * (nx + ns + 1) * n * 8 + 255) // 256 * 256
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
    fn = getattr(lib, seam or {"linear": "mht_imm_smooth_tracks", "ct": "mht_imm_smooth_tracks_ct"}[kind])
    rc = fn(ctx.handle, C.byref(mx), n, L_max, None if "len" in nulls else lens.ctypes.data_as(C.c_void_p), ptr("x_init"), ptr("P_init"), ptr("z"),
            ptr("h"), nr if r is None else r, hp_("Q"), hp_("R"), hp_("Pi"), hp_("mu0"), op("mus"), op("xs"), op("Ps"), op("muf"), op("ll"),
            op("nobs"), None if "work" in nulls else work.data_ptr(), need if work_bytes is None else work_bytes)
    torch.cuda.synchronize(dev)
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}, need


def _untouched(out):
    return all((v == SENTINEL).all() for v in out.values())


def _hold(label, got, truth, f64):
    res = ref.ratios(got, truth, f64, ref.NAMES)
    print(label + ": " + " | ".join("%s e_dev %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert ref.same_nan(got, truth, ref.NAMES), "the NaN cells are not the truth's"
    assert [g["nobs"] for g in got] == [t["nobs"] for t in truth], "nObs is not the truth's"
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, "%s: e_dev %.3g > %g x max(e_np %.3g, eps)" % (k, e, FACTOR, e_np)


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys) and (a["nObs"] == b["nObs"]) and (
        a["logLikelihood"] == b["logLikelihood"] or (np.isnan(a["logLikelihood"]) and np.isnan(b["logLikelihood"])))


CASES = [("linear", "pv", 1, 4), ("linear", "pv", 2, 4), ("linear", "pv", 3, 4), ("linear", "pv", 4, 4), ("linear", "pv", 2, 6), ("linear", "pv", 4, 6),
         ("linear", "pv", "blocked", 4), ("linear", "ca", 4, 4), ("linear", "ca", 4, 6), ("ct", "ct", 2, 4), ("ct", "ct", 2, 6)]


@pytest.mark.parametrize("kind,name,key,lib_nx", CASES)
def test_accuracy_every_cell_written_the_filter_bits_and_the_python_layer(ctxs, kind, name, key, lib_nx):
    """filter_ref.edge_batch: 35 tracks of 1, 2, 60, 7, 33 nodes in turn, every fourth never detected, under imm_ref.SETUPS[key].
    - the raw seam on arrays of 64 rows preset to a sentinel, the tracks in the order given: no cell keeps the sentinel, the rows behind
      a track's end are NaN, and the criterion holds against tests/imm_smooth_ref.py (the ratios are printed)
    - muf, ll, nObs are imm_tracks' bits on the same context, and at each track's last node so are mus, xs, Ps
    - the Python layer (which packs the batch sorted by length: other quads, other wavefronts) gives the raw call's bits per track
    Measured on an MI355X, both builds alike, ratios mus / muf / xs / Ps / ll:
        pv r=1 0 / 0 / 1.00 / 0.43 / 1.00            pv r=2 0.98 / 0.76 / 1.17 / 1.95 / 0.68    pv r=3 1.45 / 1.48 / 1.50 / 2.17 / 1.35
        pv r=4 1.32 / 1.16 / 0.92 / 0.94 / 1.00      pv blocked 0 / 0 / 1.00 / 0.83 / 1.00      ca r=4 1.90 / 2.35 / 1.08 / 0.53 / 0.70
        ct r=2 1.19 / 0.65 / 0.87 / 0.74 / 1.13      (profiles/imm_smooth_cost.txt has them with their e_np)"""
    from pymht_amd import smoothing
    assert np.finfo(np.longdouble).eps < 1e-18
    model, ctx = _model(name), ctxs[lib_nx]
    tracks, truth, f64 = ref.reference(kind, model, PERIOD, N_TRACKS, SEED, key)
    modes = ir.setup(model, PERIOD, key)
    nx = len(tracks[0][0])
    rc, out, _ = _raw(ctx, model, tracks, L_MAX, modes, kind)
    assert rc == 0 and not any((v == SENTINEL).any() for v in out.values())
    got = []
    for j, t in enumerate(tracks):
        L = len(t[2])
        assert all(np.isnan(out[k][L:, :, j]).all() for k in ("mus", "muf", "xs", "Ps"))
        got.append(dict(mus=out["mus"][:L, :, j], muf=out["muf"][:L, :, j], xs=out["xs"][:L, :, j], Ps=fr.full(out["Ps"][:L, :, j], nx),
                        ll=np.asarray(out["ll"][j]), nobs=int(out["nobs"][j])))
        assert np.array_equal(got[-1]["muf"][0], modes[3])
        assert L > 1 or (out["ll"][j] == 0.0 and not np.signbit(out["ll"][j]) and out["nobs"][j] == 0)
        assert np.abs(got[-1]["mus"].sum(axis=1) - 1.0).max() < 1e-12
    _hold("IMM smoother accuracy %s models/%s modes %s, %d-state build" % (kind, name, key, lib_nx), got, truth, f64)
    filt = smoothing.imm_tracks_ct if kind == "ct" else smoothing.imm_tracks
    per, ll, nobs = filt(model, PERIOD, tracks, *modes[:3], mu0=modes[3], ctx=ctx)
    assert np.array_equal(ll, out["ll"]) and np.array_equal(nobs, out["nobs"])
    for g, (mu, x, P) in zip(got, per):
        assert np.array_equal(g["muf"], mu)
        assert np.array_equal(g["mus"][-1], mu[-1]) and np.array_equal(g["xs"][-1], x[-1]) and np.array_equal(g["Ps"][-1], P[-1])
    run = smoothing.imm_smooth_tracks_ct if kind == "ct" else smoothing.imm_smooth_tracks
    res = run(model, PERIOD, tracks, *modes[:3], mu0=modes[3], ctx=ctx)
    for g, d in zip(got, res):
        assert sorted(d) == ["P", "logLikelihood", "mu", "muFiltered", "nObs", "x"] and d["mu"].dtype == d["x"].dtype == d["P"].dtype == np.float64
        assert _same(d, dict(mu=g["mus"], muFiltered=g["muf"], x=g["xs"], P=g["Ps"], logLikelihood=float(g["ll"]), nObs=g["nobs"]))
    if key == "blocked":
        assert all((g["mus"][1:, 1] == 0.0).all() and np.isfinite(g["xs"]).all() for g in got)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_place_in_the_batch_does_not_matter(ctxs, lib_nx):
    """130 tracks under three modes with one track at two places, 5 and 122 -- another quad, another wavefront, other neighbours --:
    the same bits at both, in the same batch permuted, and alone in a launch."""
    from pymht_amd.models import pv
    from pymht_amd.smoothing import imm_smooth_tracks
    ctx = ctxs[lib_nx]
    tracks = fr.edge_batch("linear", pv, PERIOD, 130, SEED)
    assert len(tracks[122][2]) == 60 and sr.detected(tracks[122][2])[1:].sum() > 20
    tracks[5] = tracks[122]
    Q, R, Pi, mu0 = ir.setup(pv, PERIOD, 3)
    res = imm_smooth_tracks(pv, PERIOD, tracks, Q, R, Pi, mu0=mu0, ctx=ctx)
    assert _same(res[5], res[122]) and np.isfinite(res[5]["x"]).all() and res[5]["nObs"] > 20
    rc, out, _ = _raw(ctx, pv, tracks, 60, (Q, R, Pi, mu0))      # (unsorted: the two sit in lanes 20 .. 23 of wavefront 0 and 40 .. 43 of wavefront 7)
    assert rc == 0 and all(np.array_equal(out[k][:, :, 5], out[k][:, :, 122]) for k in ("mus", "muf", "xs", "Ps"))
    assert np.array_equal(out["mus"][:, :, 5], res[5]["mu"])
    perm = np.random.default_rng(2).permutation(130)
    res2 = imm_smooth_tracks(pv, PERIOD, [tracks[i] for i in perm], Q, R, Pi, mu0=mu0, ctx=ctx)
    assert all(_same(res2[j], res[i]) for j, i in enumerate(perm))
    one, = imm_smooth_tracks(pv, PERIOD, [tracks[122]], Q, R, Pi, mu0=mu0, ctx=ctx)
    assert _same(one, res[122])


@pytest.mark.parametrize("name,kind,lib_nx", [("pv", "linear", 4), ("pv", "linear", 6), ("ca", "linear", 6), ("ct", "ct", 6)])
def test_one_mode_is_the_smoother_bit_for_bit(ctxs, name, kind, lib_nx):
    """Pi = [[1]] with the model's own Q and R: mus is all ones, xs and Ps on the rows of a track are smooth_tracks' (smooth_tracks_ct's)
    bits on the same context."""
    from pymht_amd import smoothing
    model, ctx = _model(name), ctxs[lib_nx]
    tracks = fr.edge_batch(kind, model, PERIOD, N_TRACKS, SEED)
    Q, R, Pi, mu0 = smoothing.imm_modes(model, PERIOD, (1.0,))
    run, smooth = ((smoothing.imm_smooth_tracks_ct, smoothing.smooth_tracks_ct) if kind == "ct" else (smoothing.imm_smooth_tracks, smoothing.smooth_tracks))
    res, want = run(model, PERIOD, tracks, Q, R, Pi, ctx=ctx), smooth(model, PERIOD, tracks, ctx=ctx)
    for d, (xs, Ps) in zip(res, want):
        assert (d["mu"] == 1.0).all() and (d["muFiltered"] == 1.0).all() and np.array_equal(d["x"], xs) and np.array_equal(d["P"], Ps)
    assert sum(d["nObs"] for d in res) > 200


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_identity_chain_from_a_certain_mode_is_the_smoother_under_that_mode(ctxs, lib_nx):
    """r = 2, Pi = I, mu0 = (0, 1), Q = (Q, 16 Q) on imm_ref.manoeuvre_batch, where both modes stay finite: xs and Ps are smooth_tracks'
    bits under a model whose Q is 16 x the tracker's (16 is exact in float32) and mus = (0, 1) at every node.  Mode 0 has probability
    0 throughout and never produces a 0 * inf: that is what the selects of the walk are for."""
    from pymht_amd import smoothing
    from pymht_amd.models import pv
    ctx = ctxs[lib_nx]
    tracks = ir.manoeuvre_batch(pv, PERIOD, 20, 60, seed=5)
    Q, R, _, _ = smoothing.imm_modes(pv, PERIOD, (1.0, 16.0))
    loud = types.ModuleType("pv_16q")
    loud.__dict__.update({k: v for k, v in vars(pv).items() if not k.startswith("__")})
    loud.Q = lambda T: np.float32(16.0) * np.asarray(pv.Q(T), dtype=np.float32)
    assert np.array_equal(np.asarray(loud.Q(PERIOD), dtype=np.float64).reshape(4, 4), Q[1])
    res = smoothing.imm_smooth_tracks(pv, PERIOD, tracks, Q, R, np.eye(2), mu0=[0.0, 1.0], ctx=ctx)
    want = smoothing.smooth_tracks(loud, PERIOD, tracks, ctx=ctx)
    for d, (xs, Ps) in zip(res, want):
        assert np.array_equal(d["x"], xs) and np.array_equal(d["P"], Ps)
        assert (d["mu"][:, 0] == 0.0).all() and (d["mu"][:, 1] == 1.0).all() and (d["muFiltered"][:, 0] == 0.0).all()


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_a_mode_that_is_no_covariance_poisons_the_tracks_it_scores_only(ctxs, lib_nx):
    """Mode 1 with an indefinite R (det S < 0 at every plot; the modes are the call's, so the poison reaches every track that has a plot).
    - a batch in which ONE track has plots, the others being never detected: that track's ll is NaN, every other track is bit-equal to
      the same batch without the poison
    - the whole edge batch: NaN ll for the tracks with a plot; the never-detected tracks and those of one node -- in the same
      wavefronts -- are bit-equal to the clean call, ll = 0.0 exactly"""
    from pymht_amd.models import pv
    ctx = ctxs[lib_nx]
    tracks = fr.edge_batch("linear", pv, PERIOD, N_TRACKS, SEED)
    Q, R, Pi, mu0 = ir.setup(pv, PERIOD, 2)
    bad = R.copy()
    bad[1] = np.diag([-1e9, 1.0])
    fams = ("mus", "muf", "xs", "Ps", "ll", "nobs")
    victim = next(j for j, t in enumerate(tracks) if len(t[2]) == 60 and sr.detected(t[2])[1:].sum() > 20)
    lone = [t if j == victim else (t[0], t[1], np.full((len(t[2]), 2), np.nan)) for j, t in enumerate(tracks)]
    rc, clean, _ = _raw(ctx, pv, lone, L_MAX, (Q, R, Pi, mu0))
    rc2, hurt, _ = _raw(ctx, pv, lone, L_MAX, (Q, bad, Pi, mu0))
    others = [j for j in range(N_TRACKS) if j != victim]
    assert rc == 0 and rc2 == 0 and np.isnan(hurt["ll"][victim]) and np.isfinite(clean["ll"]).all() and clean["nobs"][victim] > 20
    assert all(np.array_equal(hurt[k][..., others], clean[k][..., others], equal_nan=True) for k in fams)
    rc, clean, _ = _raw(ctx, pv, tracks, L_MAX, (Q, R, Pi, mu0))
    rc2, hurt, _ = _raw(ctx, pv, tracks, L_MAX, (Q, bad, Pi, mu0))
    scored = clean["nobs"] > 0
    assert rc == 0 and rc2 == 0 and scored.sum() >= 15 and (~scored).sum() >= 10
    assert np.isnan(hurt["ll"][scored]).all() and (hurt["ll"][~scored] == 0.0).all() and not np.signbit(hurt["ll"][~scored]).any()
    assert all(np.array_equal(hurt[k][..., ~scored], clean[k][..., ~scored], equal_nan=True) for k in fams)
    assert np.isfinite(clean["ll"]).all() and np.array_equal(hurt["nobs"], clean["nobs"])


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_raw_abi_errors_and_the_calls_behind_them(ctxs, lib_nx):
    """A null array (muf, and ll with nobs, may be null), n_modes outside 1 .. 4, a length outside 1 .. L_max, a short workspace, a wrong nx
    or transition for the seam, a row of Pi or a mu0 that is no distribution: MHT_E_INVALID each, with the sentinel in the outputs
    untouched; an empty batch is MHT_OK and writes nothing; the call behind them on the same context is right."""
    import torch
    from pymht_amd import _lib
    from pymht_amd.models import ct, pv
    from pymht_amd.smoothing import _model_x, imm_smooth_tracks
    import smooth_ct_ref as cr
    ctx = ctxs[lib_nx]
    lib = ctx.lib
    tracks = sr.make_batch(pv, PERIOD, [4, 3, 1], seed=2, p_detect=1.0)
    ct_tracks = cr.make_batch(ct, PERIOD, [4, 3, 1], seed=2)
    modes = ir.setup(pv, PERIOD, 2)
    ct_modes = ir.setup(ct, PERIOD, 2)
    need = int(lib.mht_imm_smooth_work_bytes(4, 3, 4, 2))
    assert need == 512 + 3072      # mht_imm_work_bytes' 512, and 4 rows x 2 modes x 15 doubles x 3 tracks x 8 = 2880 bytes rounded up to 256
    Q, R, Pi, mu0 = modes
    bad = [dict(nulls=(k,)) for k in ("len", "x_init", "P_init", "z", "h", "Q", "R", "Pi", "mu0", "mus", "xs", "Ps", "work", "ll", "nobs")]
    bad += [dict(r=0), dict(r=5), dict(r=-1), dict(lens=[4, 0, 1]), dict(lens=[4, 5, 1]), dict(work_bytes=need - 1), dict(model_nx=5),
            dict(transition=1), dict(seam="mht_imm_smooth_tracks_ct"), dict(seam="mht_imm_smooth_tracks_ct", transition=1)]
    for kw in bad:
        rc, out, _ = _raw(ctx, pv, tracks, 4, modes, **kw)
        assert rc == _lib.MHT_E_INVALID and lib.mht_last_error(), kw
        assert _untouched(out), kw
    for Pi_bad, mu_bad in (([[0.5, 0.6], [0.5, 0.5]], mu0), ([[1.5, -0.5], [0.5, 0.5]], mu0), ([[0.5, 0.5], [np.nan, 1.0]], mu0),
                           (Pi, [0.5, 0.6]), (Pi, [np.nan, 1.0])):
        rc, out, _ = _raw(ctx, pv, tracks, 4, (Q, R, Pi_bad, mu_bad))
        assert rc == _lib.MHT_E_INVALID and lib.mht_last_error() and _untouched(out), (Pi_bad, mu_bad)
    for kw in (dict(transition=0), dict(lens=[4, 3, 9]), dict(r=5)):
        rc, out, _ = _raw(ctx, ct, ct_tracks, 4, ct_modes, "ct", **kw)
        assert rc == _lib.MHT_E_INVALID and _untouched(out), kw
    mx, keep = _model_x(pv, PERIOD, 4, False)
    torch.cuda.synchronize(ctx.device)
    assert lib.mht_imm_smooth_tracks(ctx.handle, C.byref(mx), 0, 4, *([None] * 5), 2, *([None] * 11), 0) == _lib.MHT_OK
    rc, full, _ = _raw(ctx, pv, tracks, 4, modes)
    assert rc == _lib.MHT_OK and not any((v == SENTINEL).any() for v in full.values())
    rc, part, _ = _raw(ctx, pv, tracks, 4, modes, nulls=("muf", "ll", "nobs"))      # the optional outputs left out: the others' bits stay
    assert rc == _lib.MHT_OK and all((part[k] == SENTINEL).all() for k in ("muf", "ll", "nobs"))
    assert all(np.array_equal(part[k], full[k], equal_nan=True) for k in ("mus", "xs", "Ps"))
    res = imm_smooth_tracks(pv, PERIOD, tracks, Q, R, Pi, mu0=mu0, ctx=ctx)
    for j, d in enumerate(res):
        L = len(d["mu"])
        assert np.array_equal(full["mus"][:L, :, j], d["mu"]) and np.array_equal(full["xs"][:L, :, j], d["x"])
        assert np.array_equal(fr.full(full["Ps"][:L, :, j], 4), d["P"]) and np.isnan(full["xs"][L:, :, j]).all()
    assert [d["nObs"] for d in res] == [3, 2, 0] == full["nobs"].tolist()


def test_drop_in_path_gives_the_smoothed_mode_probabilities_of_a_run():
    """A dozen scans over six preinitialised targets on models/pv: getSmoothModeProbabilities has one entry per track with a row per
    node of its history; muFiltered, logLikelihood and nObs are getModeProbabilities' bits and so is the last node; the rows of mu add up
    to 1 within 1e-12; with the one scale (1.0,) x is getSmoothTracks' positions and velocities bit for bit, and so is
    getSmoothTracks(imm=(1.0,)); a node's own call is its entry; the refusals are getModeProbabilities', and imm excludes ais and em."""
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
        got = trk.getSmoothModeProbabilities(terminated=True)
        filt = trk.getModeProbabilities(terminated=True)
        assert len(got) == len(nodes) and len(live) > 0 and len(trk.getSmoothModeProbabilities()) == len(live)
        for d, f, node in zip(got, filt, nodes):
            L = len(node.backtrackNodes())
            assert sorted(d) == ["P", "logLikelihood", "mu", "muFiltered", "nObs", "x"]
            assert d["mu"].shape == (L, 2) and d["x"].shape == (L, 4) and d["P"].shape == (L, 4, 4)
            assert all(np.isfinite(d[k]).all() for k in KEYS) and np.abs(d["mu"].sum(axis=1) - 1.0).max() < 1e-12
            assert np.array_equal(d["muFiltered"], f["mu"]) and d["logLikelihood"] == f["logLikelihood"] and d["nObs"] == f["nObs"]
            assert all(np.array_equal(d[k][-1], f[k][-1]) for k in ("mu", "x", "P"))
        assert all(d["mu"].shape[1] == 3 for d in trk.getSmoothModeProbabilities(qScales=(0.25, 1.0, 16.0), stay=0.9))
        one = trk.getSmoothModeProbabilities(qScales=(1.0,), terminated=True)
        plain, via = trk.getSmoothTracks(terminated=True), trk.getSmoothTracks(terminated=True, imm=(1.0,))
        for d, (pos, vel, ok), (pos2, vel2, ok2) in zip(one, plain, via):
            assert (d["mu"] == 1.0).all() and np.array_equal(pos2, pos, equal_nan=True) and np.array_equal(vel2, vel, equal_nan=True) and ok2 == ok
            assert len(d["x"]) < 2 or (np.array_equal(d["x"][:, 0:2], pos) and np.array_equal(d["x"][:, 2:4], vel))
        two = trk.getSmoothTracks(terminated=True, imm=(1.0, 16.0))
        for d, (pos, vel, ok) in zip(got, two):
            assert len(d["x"]) < 2 or (ok and np.array_equal(pos, d["x"][:, 0:2]) and np.array_equal(vel, d["x"][:, 2:4]))
        i = max(range(len(nodes)), key=lambda j: len(got[j]["mu"]))
        own = nodes[i].getSmoothModeProbabilities(trk.radarPeriod)
        assert len(got[i]["mu"]) >= 10 and all(np.array_equal(own[k], got[i][k]) for k in KEYS) and own["nObs"] == got[i]["nObs"]
        with pytest.raises(ValueError, match="constant-turn"):
            trk.getSmoothModeProbabilities(constantTurn=True)
        with pytest.raises(ValueError):
            trk.getSmoothModeProbabilities(qScales=(1.0, 2.0, 3.0, 4.0, 5.0))
        with pytest.raises(ValueError, match="imm"):
            trk.getSmoothTracks(imm=(1.0, 16.0), em=3)
        with pytest.raises(ValueError, match="imm"):
            trk.getSmoothTracks(imm=(1.0, 16.0), ais=True)
    finally:
        trk.close()
    turning = Tracker(ct, PERIOD, 1e-7, 1e-4, P_d=0.9, N=4, eta2=5.99, useInitiator=False)
    try:
        with pytest.raises(NotImplementedError, match="ct"):
            turning.getSmoothModeProbabilities()
        assert turning.getSmoothModeProbabilities(constantTurn=True) == []
        assert turning.getSmoothTracks(constantTurn=True, imm=(1.0, 16.0)) == []
    finally:
        turning.close()
