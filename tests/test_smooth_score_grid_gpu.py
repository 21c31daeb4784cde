"""GPU: the score seams under a grid of candidate noise models in one launch (`mht_score_tracks_grid`, `mht_score_tracks_ct_grid`,
include/mht_amd.h; pymht_amd.smoothing.score_tracks_grid, score_tracks_ct_grid, score_nodes_grid) and the drop-in path on top
(Tracker.getLikelihoodSurface).

A candidate a model can carry -- a power-of-two scaling of its float32 Q and R -- must give the bits of `score_tracks` /
`score_tracks_ct` under a stand-in model with those matrices: the grid walk is that walk.  No (track, candidate) depends on its
neighbours: a candidate alone, the candidates reversed and the tracks reversed give the same bits.  A candidate no float32 holds is held
to the project's criterion against the np.longdouble evaluation of tests/smooth_score_ref.py under the candidate's float64 matrices,
e_dev <= 8 max(e_np, eps64) per candidate row, counts exactly (tests/smooth_score_grid_ref.py); every test prints what it measured."""
import ctypes as C

import numpy as np
import pytest

import smooth_ref as sr
import smooth_score_grid_ref as gref
import smooth_score_ref as ref
from test_smooth_score_gpu import LENGTHS

pytestmark = pytest.mark.gpu

PERIOD = 2.5


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


def _case(name):
    """(model, the plain seam's function, the grid's, the batch of test_smooth_score_gpu.py for it)"""
    from pymht_amd import smoothing
    from pymht_amd.models import ca, ct, pv
    if name == "ct":
        return ct, smoothing.score_tracks_ct, smoothing.score_tracks_ct_grid, ref.ct_batch(ct, PERIOD)[0]
    model = {"pv": pv, "ca": ca}[name]
    return model, smoothing.score_tracks, smoothing.score_tracks_grid, sr.make_batch(model, PERIOD, LENGTHS, seed=23, p_detect=0.8)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("name", ["pv", "ca", "ct"])
def test_a_row_is_the_plain_seam_under_that_candidate(ctxs, name, lib_nx):
    """The 5 x 5 power-of-two grid: 130 tracks of 1 .. 300 nodes (three workgroups a candidate, the last partial) for pv and ca, the
    33 tracks of smooth_score_ref.ct_batch for ct; 25 plain calls against one grid call."""
    from pymht_amd.smoothing import noise_grid
    model, plain, grid, tracks = _case(name)
    assert name == "ct" or len(tracks) == 130
    ctx = ctxs[lib_nx]
    Q, R = noise_grid(model, PERIOD, gref.POW2, gref.POW2)
    ll, nis, nobs = grid(model, PERIOD, tracks, Q, R, ctx=ctx)
    assert ll.shape == nis.shape == (25, len(tracks)) and nobs.shape == (len(tracks),) and ll.dtype == nis.dtype == np.float64 and nobs.dtype == np.int32
    for g in range(25):
        want = plain(gref.stand_in(model, Q[g], R[g]), PERIOD, tracks, ctx=ctx)
        assert np.array_equal(ll[g], np.array([w[0] for w in want])) and np.array_equal(nis[g], np.array([w[1] for w in want])), g
        assert nobs.tolist() == [w[2] for w in want]
    assert np.isfinite(ll).all() and np.isfinite(nis).all() and nobs.sum() > 500
    assert len({ll[g].tobytes() for g in range(25)}) == 25


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("name", ["pv", "ca", "ct"])
def test_no_cell_depends_on_its_neighbours(ctxs, name, lib_nx):
    """A candidate alone gives its row's bits; the candidates reversed reverse the rows; the tracks reversed permute the columns."""
    from pymht_amd.smoothing import noise_grid
    model, _, grid, tracks = _case(name)
    ctx = ctxs[lib_nx]
    Q, R = noise_grid(model, PERIOD, gref.ODD + (1.0,), gref.ODD)
    got = grid(model, PERIOD, tracks, Q, R, ctx=ctx)
    for g in (0, 3, 5):
        ll, nis, nobs = grid(model, PERIOD, tracks, Q[g:g + 1], R[g:g + 1], ctx=ctx)
        assert ll.shape == (1, len(tracks)) and _same((ll[0], nis[0], nobs), (got[0][g], got[1][g], got[2]))
    rev = grid(model, PERIOD, tracks, Q[::-1], R[::-1], ctx=ctx)
    assert _same((rev[0][::-1], rev[1][::-1], rev[2]), got)
    back = grid(model, PERIOD, tracks[::-1], Q, R, ctx=ctx)
    assert _same((back[0][:, ::-1], back[1][:, ::-1], back[2][::-1]), got)
    assert np.isfinite(got[0]).all() and len({got[0][g].tobytes() for g in range(6)}) == 6


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("name", ["pv", "ca", "ct"])
def test_accuracy_against_the_longdouble_truth(ctxs, name, lib_nx):
    """Scales {0.3, 1.7}^2 on smooth_score_ref's accuracy batches (33 tracks of 1 .. 60 nodes), each candidate row against the reference
    under that candidate's float64 matrices.  The host twin of the same header measures largest ratios e / max(e_np, eps64) of
    1.00 - 1.20 here (tests/test_smooth_score_grid_cpu.py); the device's own are printed by this test."""
    assert np.finfo(np.longdouble).eps < 1e-18
    model, _, grid, _ = _case(name)
    tracks, Q, R, truth, f64 = gref.reference("ct" if name == "ct" else "linear", model, PERIOD)
    ll, nis, nobs = grid(model, PERIOD, tracks, Q, R, ctx=ctxs[lib_nx])
    worst = gref.hold("grid score accuracy models/%s, %d-state build" % (name, lib_nx), gref.rows_as_dicts(ll, nis, nobs), truth, f64)
    print("models/%s, %d-state build: worst ratio ll %.3g nis %.3g" % (name, lib_nx, worst["ll"], worst["nis"]))


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_edges(ctxs, lib_nx):
    """Nothing to explain is exactly +0.0 in every row; an indefinite R poisons its own row only; one track, one full wavefront, one
    lane more than a wavefront."""
    from pymht_amd.models import pv
    from pymht_amd.smoothing import noise_grid, score_tracks, score_tracks_grid
    ctx = ctxs[lib_nx]
    tracks, one, never, always = ref.linear_batch(pv, PERIOD)
    Q, R = noise_grid(pv, PERIOD, [0.5, 1.0, 2.0], [1.0])
    R[1] = np.diag([-1e9, 1.0])
    ll, nis, nobs = score_tracks_grid(pv, PERIOD, tracks, Q, R, ctx=ctx)
    for t in (one, never):
        assert nobs[t] == 0 and not ll[:, t].any() and not nis[:, t].any() and not np.signbit(ll[:, t]).any() and not np.signbit(nis[:, t]).any()
    scored = nobs > 0
    assert scored.sum() >= 20 and np.isnan(ll[1, scored]).all() and np.isnan(nis[1, scored]).all()
    assert np.isfinite(ll[[0, 2]]).all() and np.isfinite(nis[[0, 2]]).all() and nobs[always] == len(tracks[always][2]) - 1
    Q, R = noise_grid(pv, PERIOD, [1.0, 2.0], [1.0])
    batch = sr.make_batch(pv, PERIOD, LENGTHS[:65], seed=23, p_detect=0.8)
    for n in (1, 64, 65):
        part = batch[2:3] if n == 1 else batch[:n]      # (alone: the track of 300 nodes)
        ll, nis, nobs = score_tracks_grid(pv, PERIOD, part, Q, R, ctx=ctx)
        want = score_tracks(pv, PERIOD, part, ctx=ctx)
        assert ll.shape == (2, n) and np.array_equal(ll[0], np.array([w[0] for w in want])) and np.array_equal(nis[0], np.array([w[1] for w in want]))
        assert nobs.tolist() == [w[2] for w in want] and nobs.sum() > 0 and np.isfinite(ll).all() and not np.array_equal(ll[0], ll[1])


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_raw_abi_refusals_launch_nothing_and_a_valid_call_follows(ctxs, lib_nx):
    """n_cand 0 and 4097, a null Q_cand, a short workspace, a wrong transition (either seam): MHT_E_INVALID, outputs untouched."""
    import torch
    from pymht_amd import _lib
    from pymht_amd.models import pv
    from pymht_amd.smoothing import noise_grid, score_tracks_grid
    ctx = ctxs[lib_nx]
    lib, dev = ctx.lib, ctx.device
    n, L, nx, G = 3, 4, 4, 2
    keep = [np.ascontiguousarray(np.asarray(m, dtype=np.float32).ravel()) for m in (pv.Phi(PERIOD), pv.Q(PERIOD), pv.C_RADAR, pv.R_RADAR())]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    tracks = sr.make_batch(pv, PERIOD, [4, 3, 1], seed=2, p_detect=1.0)
    Q, R = noise_grid(pv, PERIOD, [1.0, 2.0], [1.0])
    Qbig, Rbig = np.ascontiguousarray(np.repeat(Q[:1], 4097, axis=0)), np.ascontiguousarray(np.repeat(R[:1], 4097, axis=0))
    need = int(lib.mht_score_grid_work_bytes(nx, n, L, G))
    assert need == 512
    x0 = torch.from_numpy(np.stack([t[0] for t in tracks], axis=1)).to(dev).contiguous()
    P0 = torch.from_numpy(np.stack([np.asarray(t[1]).ravel() for t in tracks], axis=1)).to(dev).contiguous()
    zp, hp = np.zeros((L, 2, n)), np.zeros((L, n), dtype=np.uint8)
    for j, (_, _, z) in enumerate(tracks):
        zp[1:len(z), :, j], hp[1:len(z), j] = z[1:], 1
    zz, hz = torch.from_numpy(zp).to(dev), torch.from_numpy(hp).to(dev)
    # (room for 4097 rows, so that a refusal that did launch would not write out of bounds)
    outs = [torch.full((4097, n), -7, dtype=torch.float64, device=dev) for _ in range(2)] + [torch.full((n,), -7, dtype=torch.int32, device=dev)]
    work = torch.zeros(int(lib.mht_score_grid_work_bytes(nx, n, L, 4096)) + 4096, dtype=torch.uint8, device=dev)
    lens = np.array([4, 3, 1], dtype=np.int32)

    def call(transition, n_cand, q, r, work_bytes, seam="mht_score_tracks_grid", model_nx=4):
        mx = _lib.MhtModelX(model_nx, fp(keep[0]), fp(keep[1]), fp(keep[2]), fp(keep[3]), 0.0, 0.0, transition, PERIOD)
        torch.cuda.synchronize(dev)
        return getattr(lib, seam)(ctx.handle, C.byref(mx), n, L, lens.ctypes.data_as(C.c_void_p), x0.data_ptr(), P0.data_ptr(), zz.data_ptr(),
                                  hz.data_ptr(), n_cand, None if q is None else q.ctypes.data_as(C.c_void_p),
                                  None if r is None else r.ctypes.data_as(C.c_void_p), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                  work.data_ptr(), work_bytes)
    for args in ((0, 0, Q, R, need), (0, 4097, Qbig, Rbig, work.numel()), (0, G, None, R, need), (0, G, Q, None, need), (0, G, Q, R, need - 1),
                 (1, G, Q, R, need), (0, G, Q, R, need, "mht_score_tracks_ct_grid"), (0, G, Q, R, need, "mht_score_tracks_ct_grid", 6),
                 (0, G, Q, R, need, "mht_score_tracks_grid", 5)):
        assert call(*args) == _lib.MHT_E_INVALID, args[:2] + args[4:]
        assert lib.mht_last_error()
        torch.cuda.synchronize(dev)
        assert all(bool((o == -7).all()) for o in outs)
    assert call(0, G, Q, R, need) == _lib.MHT_OK
    torch.cuda.synchronize(dev)
    ll, nis, nobs = score_tracks_grid(pv, PERIOD, tracks, Q, R, ctx=ctx)
    assert np.array_equal(outs[0][:G].cpu().numpy(), ll) and np.array_equal(outs[1][:G].cpu().numpy(), nis) and outs[2].cpu().tolist() == nobs.tolist()
    assert bool((outs[0][G:] == -7).all()) and bool((outs[1][G:] == -7).all())
    assert nobs.tolist() == [3, 2, 0] and not ll[:, 2].any()
    A, _, Cm, _ = sr.model_matrices(pv, PERIOD)
    for g in range(G):
        f64 = [ref.score(A, Q[g], Cm, R[g], *t) for t in tracks]
        assert all(abs(ll[g, t] - f["ll"]) <= 1e-9 * (1 + abs(f["ll"])) for t, f in enumerate(f64))


def test_the_surface_of_a_run():
    """A tracker stepped over test_smooth_em_gpu.py's seeded scene (25 scans): the centre of a 3 x 3 surface is getTrackLikelihoods, bit
    for bit; the totals are the tracks' sums; best is the argmax."""
    from pymht_amd.smoothing import best_cell
    from test_smooth_em_gpu import _run_scenario
    trk, sc, pv = _run_scenario()
    try:
        want = trk.getTrackLikelihoods(terminated=True)
        s = trk.getLikelihoodSurface([0.5, 1, 2], [0.5, 1, 2], terminated=True)
        n = len(want)
        assert n >= 5 and s["trackLl"].shape == s["trackNis"].shape == (3, 3, n) and s["trackNObs"].shape == (n,) and s["ll"].shape == s["nis"].shape == (3, 3)
        assert s["trackLl"][1, 1].tolist() == [w[0] for w in want] and s["trackNis"][1, 1].tolist() == [w[1] for w in want]
        assert s["trackNObs"].tolist() == [w[2] for w in want] and s["nObs"] == sum(w[2] for w in want) >= 10 and type(s["nObs"]) is int
        assert np.array_equal(s["ll"], np.sum(s["trackLl"], axis=2)) and np.array_equal(s["nis"], np.sum(s["trackNis"], axis=2))
        assert s["qScales"].tolist() == [0.5, 1.0, 2.0] == s["rScales"].tolist()
        assert np.isfinite(s["ll"]).all() and s["best"] == tuple(int(i) for i in np.unravel_index(np.argmax(s["ll"]), (3, 3)))
        assert best_cell(np.array([[np.nan, 1.0], [1.0, -np.inf]])) == (0, 1) and best_cell(np.full((2, 2), np.nan)) is None
        assert len(set(s["ll"].ravel().tolist())) == 9
        live = trk.getLikelihoodSurface([1.0], [1.0])
        assert live["trackLl"][0, 0].tolist() == [w[0] for w in trk.getTrackLikelihoods()] and live["best"] == (0, 0)
        with pytest.raises(ValueError, match="constant-turn"):
            trk.getLikelihoodSurface([1.0], [1.0], constantTurn=True)
        with pytest.raises(ValueError, match="qScales"):
            trk.getLikelihoodSurface([0.0], [1.0])
    finally:
        trk.close()


def test_the_surface_of_a_constant_turn_run():
    from pymht_amd.models import ct
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    from test_smooth_ct_gpu import _turning_scene
    x0, scans, times = _turning_scene()
    trk = Tracker(ct, PERIOD, 1e-7, 1e-4, P_d=0.9, N=4, eta2=5.99, useInitiator=False)
    try:
        for x in x0:
            trk.initiateTarget(Target(1000.0, None, x.copy(), ct.P0, status="preinitialized"))
        for zk, tk in zip(scans, times):
            trk.addMeasurementList(MeasurementList(float(tk), zk))
        with pytest.raises(NotImplementedError, match="ct"):
            trk.getLikelihoodSurface([1.0], [1.0])
        want = trk.getTrackLikelihoods(terminated=True, constantTurn=True)
        s = trk.getLikelihoodSurface([1, 2], [0.5, 1], terminated=True, constantTurn=True)
        assert s["trackLl"][0, 1].tolist() == [w[0] for w in want] and s["trackNObs"].tolist() == [w[2] for w in want] and s["nObs"] >= 15
        assert s["best"] == tuple(int(i) for i in np.unravel_index(np.argmax(s["ll"]), (2, 2)))
    finally:
        trk.close()


def test_the_surface_recovers_the_noise_the_plots_were_made_with(ctxs):
    """60 tracks of 30 nodes simulated from pv with Q_true = 4 Q and R_true = R / 4 (seed 11), over {1/4, 1, 4}^2.  On the float64
    reference alone: the pooled argmax is the true cell, -12521.38, and the runner-up lies 34.27 below it, against a rounding allowance
    of 1e-6 (1 + |ll|) = 0.0125.  Then the device's best is that cell."""
    from pymht_amd.models import pv
    from pymht_amd.smoothing import best_cell, noise_grid, score_tracks_grid
    tracks, surface = gref.recovery_batch(pv, PERIOD)
    true = gref.RECOVERY_TRUE
    assert gref.RECOVERY_SCALES[true[0]] == 4.0 and gref.RECOVERY_SCALES[true[1]] == 0.25
    assert np.isfinite(surface).all() and tuple(int(i) for i in np.unravel_index(np.argmax(surface), (3, 3))) == true
    order = np.sort(surface.ravel())
    print("reference: true cell %.6f, runner-up %.6f below, allowance %.3g" % (order[-1], order[-1] - order[-2], 1e-6 * (1 + abs(order[-1]))))
    assert order[-1] - order[-2] > 1e-6 * (1 + abs(order[-1]))
    Q, R = noise_grid(pv, PERIOD, gref.RECOVERY_SCALES, gref.RECOVERY_SCALES)
    ll, nis, nobs = score_tracks_grid(pv, PERIOD, tracks, Q, R, ctx=ctxs[4])
    dev = np.sum(ll, axis=1).reshape(3, 3)
    print("device surface:", dev.tolist())
    assert best_cell(dev) == true      # (the rule behind getLikelihoodSurface()['best'])
    assert np.max(np.abs(dev - surface) / (1 + np.abs(surface))) < 1e-9
