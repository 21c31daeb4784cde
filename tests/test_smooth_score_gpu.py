"""GPU: the device score of track histories (`mht_score_tracks`, `mht_score_tracks_ct`, `mht_score_tracks_ais`, include/mht_amd.h seam
(vi); pymht_amd.smoothing.score_tracks*), the EM trace of log-likelihoods (`mht_smooth_tracks_em_ll`; smooth_tracks_em(likelihoods=True))
and the drop-in path on top (Tracker.getTrackLikelihoods, Target.getTrackLikelihood), against tests/smooth_score_ref.py.

The criterion is the smoothers' (tests/test_smooth_gpu.py): with the np.longdouble evaluation of the reference as the truth, over a batch
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
and e_dev <= 8 * max(e_np, eps64), for ll, nis, nisAis and each row of the trace separately; counts exactly.  The float64 reference
sets the scale, never the device.  Every test prints the ratios it measured; tools/smooth_score_cost.py writes them into
profiles/smooth_score_cost.txt, which until its first device run holds the host twin's (0.99 - 1.67 over the four models)."""
import ctypes as C

import numpy as np
import pytest

import smooth_ais_ref as ar
import smooth_ct_ref as cr
import smooth_em_ref as er
import smooth_ref as sr
import smooth_score_ref as ref

pytestmark = pytest.mark.gpu

PERIOD = 2.5
FACTOR = 8.0
EPS = float(np.finfo(np.float64).eps)
LENGTHS = [1, 2, 300, 1, 2, 3, 250] + [int(v) for v in np.random.default_rng(5).integers(1, 90, 123)]      # (test_smooth_em_gpu.py's)


def _model(name):
    from pymht_amd.models import pv, ca
    return {"pv": pv, "ca": ca}[name]


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


def _dicts(dev):
    keys = ("ll", "nis", "nobs", "nis_ais", "nais")
    return [dict(zip(keys, d)) for d in dev]


def _hold(label, got, truth, f64, names):
    res = ref.ratios(got, truth, f64, names)
    print(label + ": " + " | ".join("%s e_dev %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, "%s: e_dev %.3g > %g x max(e_np %.3g, eps)" % (k, e, FACTOR, e_np)
    for g, t in zip(got, truth):
        assert g["nobs"] == t["nobs"] and g.get("nais", 0) == t["nais"]


def _exact_zero(r):
    assert r[0] == 0.0 and r[1] == 0.0 and r[2] == 0 and not np.signbit(r[0]) and not np.signbit(r[1])


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_linear_accuracy_against_the_longdouble_truth(ctxs, name, lib_nx):
    """smooth_em_ref.accuracy_batch, 33 tracks of 1 .. 60 nodes; ll and nis.  The host twin of the same header measures ratios
    e / max(e_np, eps64) of 1.00 - 1.11 here (tests/test_smooth_score_cpu.py); the device's own are printed by this test and recorded
    by tools/smooth_score_cost.py."""
    from pymht_amd.smoothing import score_tracks
    assert np.finfo(np.longdouble).eps < 1e-18
    model = _model(name)
    tracks, truth, f64 = ref.reference("linear", model, PERIOD)
    _, one, never, always = ref.linear_batch(model, PERIOD)
    dev = score_tracks(model, PERIOD, tracks, ctx=ctxs[lib_nx])
    assert all(len(d) == 3 and type(d[0]) is float and type(d[1]) is float and type(d[2]) is int for d in dev)
    _hold("score accuracy models/%s, %d-state build" % (name, lib_nx), _dicts(dev), truth, f64, ("ll", "nis"))
    _exact_zero(dev[one])
    _exact_zero(dev[never])
    assert dev[always][2] == len(tracks[always][2]) - 1 and dev[always][0] < 0.0 < dev[always][1]


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_constant_turn_accuracy_against_the_longdouble_truth(ctxs, lib_nx):
    """A smooth_ct_ref.make_batch of the linear batch's lengths; ll and nis."""
    from pymht_amd.models import ct
    from pymht_amd.smoothing import score_tracks_ct
    tracks, truth, f64 = ref.reference("ct", ct, PERIOD)
    _, one, never, always = ref.ct_batch(ct, PERIOD)
    dev = score_tracks_ct(ct, PERIOD, tracks, ctx=ctxs[lib_nx])
    _hold("score accuracy models/ct, %d-state build" % lib_nx, _dicts(dev), truth, f64, ("ll", "nis"))
    _exact_zero(dev[one])
    _exact_zero(dev[never])


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_ais_accuracy_against_the_longdouble_truth(ctxs, lib_nx):
    """smooth_ais_ref.accuracy_batch, 40 tracks of 2 .. 400 nodes; ll, nis and nisAis, nObs and nAis."""
    from pymht_amd.smoothing import score_tracks_ais
    model, _ = ar.accuracy_batch()
    tracks, truth, f64 = ref.reference("ais", model, PERIOD)
    dev = score_tracks_ais(model, PERIOD, tracks, ctx=ctxs[lib_nx])
    assert all(len(d) == 5 for d in dev)
    _hold("score accuracy AIS, %d-state build" % lib_nx, _dicts(dev), truth, f64, ("ll", "nis", "nis_ais"))
    assert sum(d[4] for d in dev) > 1000


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_linear_batch_independence(ctxs, name, lib_nx):
    """130 tracks of 1 .. 300 nodes, more than a wavefront and not a multiple of 64: a permuted batch and a track alone, bit for bit."""
    from pymht_amd.smoothing import score_tracks
    model = _model(name)
    assert len(LENGTHS) == 130
    tracks = sr.make_batch(model, PERIOD, LENGTHS, seed=23, p_detect=0.8)
    ctx = ctxs[lib_nx]
    got = score_tracks(model, PERIOD, tracks, ctx=ctx)
    perm = np.random.default_rng(1).permutation(len(tracks))
    assert score_tracks(model, PERIOD, [tracks[i] for i in perm], ctx=ctx) == [got[i] for i in perm]
    for t in (2, 6, 70, 129):
        assert score_tracks(model, PERIOD, [tracks[t]], ctx=ctx) == [got[t]]
    assert all(np.isfinite(g[0]) and np.isfinite(g[1]) for g in got) and sum(g[2] for g in got) > 3000
    _exact_zero(got[0])


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_ct_and_ais_batch_independence(ctxs, lib_nx):
    """70 tracks each, more than a wavefront."""
    from pymht_amd.models import ct, pv
    from pymht_amd.smoothing import score_tracks_ais, score_tracks_ct
    ctx = ctxs[lib_nx]
    lengths = LENGTHS[:70]
    perm = np.random.default_rng(2).permutation(70)
    for score, model, tracks in ((score_tracks_ct, ct, cr.make_batch(ct, PERIOD, lengths, seed=31)),
                                 (score_tracks_ais, pv, ar.make_batch(pv, PERIOD, lengths, seed=37))):
        got = score(model, PERIOD, tracks, ctx=ctx)
        assert score(model, PERIOD, [tracks[i] for i in perm], ctx=ctx) == [got[i] for i in perm]
        for t in (2, 6, 69):
            assert score(model, PERIOD, [tracks[t]], ctx=ctx) == [got[t]]
        assert all(np.isfinite(g[0]) and np.isfinite(g[1]) for g in got)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_ais_seam_without_messages_is_the_linear_seam_bit_for_bit(ctxs, lib_nx):
    from pymht_amd.models import pv
    from pymht_amd.smoothing import score_tracks, score_tracks_ais
    tracks = sr.make_batch(pv, PERIOD, LENGTHS, seed=23, p_detect=0.8)
    lin = score_tracks(pv, PERIOD, tracks, ctx=ctxs[lib_nx])
    plain = score_tracks_ais(pv, PERIOD, [t + ([None] * len(t[2]),) for t in tracks], ctx=ctxs[lib_nx])
    assert [p[:3] for p in plain] == lin
    assert all(p[3] == 0.0 and p[4] == 0 for p in plain)


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("start", ["model", "reference"])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_em_trace(ctxs, name, start, lib_nx):
    """smooth_em_ref.accuracy_batch, five iterations: the other outputs keep their bits, row 0 is score_tracks', every row meets the
    criterion against the longdouble trace, and the device rows never decrease by more than the criterion's own slack."""
    from pymht_amd.smoothing import score_tracks, smooth_tracks_em
    model = _model(name)
    ctx = ctxs[lib_nx]
    tracks, truth, f64 = ref.trace_reference(model, PERIOD, start)
    _, one, never, always = er.accuracy_batch(model, PERIOD)
    plain = smooth_tracks_em(model, PERIOD, tracks, n_iter=5, start=start, ctx=ctx)
    traced = smooth_tracks_em(model, PERIOD, tracks, n_iter=5, start=start, ctx=ctx, likelihoods=True)
    for p, t in zip(plain, traced):
        assert len(p) == 4 and len(t) == 5 and t[4].shape == (6,) and t[4].dtype == np.float64
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(p, t[:4]))
    # row 0: the score under the start values, bit for bit
    started = []
    for x0, P0, z in tracks:
        Q, R, P = er.start_values(model, PERIOD, P0, start)
        started.append((x0, P, z))
    if start == "model":
        base = score_tracks(model, PERIOD, started, ctx=ctx)
    else:
        class Identity:      # the model with identity Q and R: what start="reference" begins at
            __name__ = "identity"
            Phi, C_RADAR, P0 = staticmethod(model.Phi), model.C_RADAR, model.P0
            Q = staticmethod(lambda T: np.eye(model.C_RADAR.shape[1]))
            R_RADAR = staticmethod(lambda: np.eye(2))
        base = score_tracks(Identity, PERIOD, started, ctx=ctx)
    assert [t[4][0] for t in traced] == [b[0] for b in base]
    got = [t[4] for t in traced]
    rows = ref.trace_ratios(got, truth, f64)
    print("EM trace models/%s, start=%s, %d-state build, rows 0 .. 5 ratio: " % (name, start, lib_nx) + " ".join("%.3g" % r[2] for r in rows)
          + " | e_np " + " ".join("%.3g" % r[1] for r in rows))
    for i, (e, e_np, ratio) in enumerate(rows):
        assert np.isfinite(e) and ratio <= FACTOR, "row %d: e_dev %.3g > %g x max(e_np %.3g, eps)" % (i, e, FACTOR, e_np)
    for ll in got:
        for i in range(5):
            assert ll[i + 1] >= ll[i] - FACTOR * max(rows[i][1], EPS) * (1 + abs(ll[i])), (i, ll)
    assert (got[one] == 0.0).all() and (got[never] == 0.0).all()
    assert any(ll[5] > ll[0] for ll in got)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_em_trace_without_an_iteration_is_one_row(ctxs, lib_nx):
    from pymht_amd.models import ca
    from pymht_amd.smoothing import score_tracks, smooth_tracks_em
    tracks = er.accuracy_batch(ca, PERIOD)[0]
    traced = smooth_tracks_em(ca, PERIOD, tracks, n_iter=0, ctx=ctxs[lib_nx], likelihoods=True)
    plain = smooth_tracks_em(ca, PERIOD, tracks, n_iter=0, ctx=ctxs[lib_nx])
    base = score_tracks(ca, PERIOD, tracks, ctx=ctxs[lib_nx])
    for p, t, b in zip(plain, traced, base):
        assert t[4].shape == (1,) and t[4][0] == b[0] and all(np.array_equal(u, v) for u, v in zip(p, t[:4]))


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_raw_abi_errors_and_the_calls_behind_them(ctxs, lib_nx):
    """Bad nx, a wrong transition, a short workspace and a length of 0 each give MHT_E_INVALID with the outputs untouched; the calls on
    the same context afterwards are correct."""
    import torch
    from pymht_amd import _lib
    from pymht_amd.models import pv
    from pymht_amd.smoothing import score_tracks
    ctx = ctxs[lib_nx]
    lib, dev = ctx.lib, ctx.device
    n, L, nx = 3, 4, 4
    keep = [np.ascontiguousarray(np.asarray(m, dtype=np.float32).ravel()) for m in (pv.Phi(PERIOD), pv.Q(PERIOD), pv.C_RADAR, pv.R_RADAR())]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    tracks = sr.make_batch(pv, PERIOD, [4, 3, 1], seed=2, p_detect=1.0)
    need = int(lib.mht_score_work_bytes(nx, n, L))
    assert need == 256 and lib.mht_score_work_bytes(5, n, L) == 0 and lib.mht_score_work_bytes(4, -1, L) == 0 and lib.mht_score_work_bytes(4, n, -1) == 0
    x0 = torch.from_numpy(np.stack([t[0] for t in tracks], axis=1)).to(dev).contiguous()
    P0 = torch.from_numpy(np.stack([np.asarray(t[1]).ravel() for t in tracks], axis=1)).to(dev).contiguous()
    zp, hp = np.zeros((L, 2, n)), np.zeros((L, n), dtype=np.uint8)
    for j, (_, _, z) in enumerate(tracks):
        zp[1:len(z), :, j], hp[1:len(z), j] = z[1:], 1
    zz, hz = torch.from_numpy(zp).to(dev), torch.from_numpy(hp).to(dev)
    outs = [torch.full((n,), -7, dtype=dt, device=dev) for dt in (torch.float64, torch.float64, torch.int32)]
    work = torch.zeros(need, dtype=torch.uint8, device=dev)

    def call(model_nx, transition, lens, work_bytes, seam="mht_score_tracks"):
        mx = _lib.MhtModelX(model_nx, fp(keep[0]), fp(keep[1]), fp(keep[2]), fp(keep[3]), 0.0, 0.0, transition, PERIOD)
        lens = np.array(lens, dtype=np.int32)
        torch.cuda.synchronize(dev)
        return getattr(lib, seam)(ctx.handle, C.byref(mx), n, L, lens.ctypes.data_as(C.c_void_p), x0.data_ptr(), P0.data_ptr(), zz.data_ptr(),
                                  hz.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), work.data_ptr(), work_bytes)
    good = [4, 3, 1]
    for args in ((5, 0, good, need), (4, 1, good, need), (4, 0, good, need - 1), (4, 0, [4, 0, 1], need), (4, 0, [4, 5, 1], need),
                 (4, 0, good, need, "mht_score_tracks_ct"), (6, 0, good, need, "mht_score_tracks_ct")):
        assert call(*args) == _lib.MHT_E_INVALID, args
        assert lib.mht_last_error()
        torch.cuda.synchronize(dev)
        assert all(bool((o == -7).all()) for o in outs)
    assert call(4, 0, good, need) == _lib.MHT_OK
    torch.cuda.synchronize(dev)
    want = score_tracks(pv, PERIOD, tracks, ctx=ctx)
    raw = list(zip(outs[0].cpu().tolist(), outs[1].cpu().tolist(), outs[2].cpu().tolist()))
    assert raw == want and want[2] == (0.0, 0.0, 0) and want[0][2] == 3
    A, Q, Cm, R = sr.model_matrices(pv, PERIOD)
    f64 = [ref.score(A, Q, Cm, R, *t) for t in tracks]
    assert all(abs(w[0] - f["ll"]) <= 1e-9 * (1 + abs(f["ll"])) and w[2] == f["nobs"] for w, f in zip(want, f64))


def _scored_directly(trk, model, nodes, score, extra=lambda chain: ()):
    from pymht_amd.smoothing import chain_inputs
    long_ones = [i for i, node in enumerate(nodes) if len(node.backtrackNodes()) >= 2]
    batch = []
    for i in long_ones:
        chain, inputs = chain_inputs(nodes[i], model.P0)
        batch.append(inputs + extra(chain))
    return long_ones, score(model, trk.radarPeriod, batch, ctx=trk._ctx)


def test_drop_in_path_scores_the_tracks_of_a_run():
    from pymht_amd.smoothing import score_tracks
    from test_smooth_em_gpu import _run_scenario
    trk, sc, pv = _run_scenario()
    try:
        live = list(trk.getTrackNodes())
        nodes = live + list(trk.__terminatedTargets__)
        got = trk.getTrackLikelihoods(terminated=True)
        assert len(got) == len(nodes) and trk.getTrackLikelihoods() == got[:len(live)] and len(nodes) >= len(live) > 0
        long_ones, direct = _scored_directly(trk, pv, nodes, score_tracks)
        assert len(long_ones) >= 5 and [got[i] for i in long_ones] == direct
        assert all(got[i] == (0.0, 0.0, 0) for i in range(len(nodes)) if i not in long_ones)
        assert sum(d[2] for d in direct) >= 10 and all(np.isfinite(d[0]) and d[0] < 0 < d[1] for d in direct if d[2])
        i = max(long_ones, key=lambda j: len(nodes[j].backtrackNodes()))
        assert nodes[i].getTrackLikelihood(trk.radarPeriod) == got[i]
        A, Q, Cm, R = sr.model_matrices(pv, sc["period"])
        from pymht_amd.smoothing import chain_inputs
        f = ref.score(A, Q, Cm, R, *chain_inputs(nodes[i], pv.P0)[1])
        assert abs(got[i][0] - f["ll"]) <= 1e-9 * (1 + abs(f["ll"])) and got[i][2] == f["nobs"]
        with pytest.raises(ValueError, match="constant-turn"):
            trk.getTrackLikelihoods(constantTurn=True)
        with pytest.raises(ValueError, match="aisAided"):
            trk.getTrackLikelihoods(ais=True)
    finally:
        trk.close()


def test_drop_in_path_scores_a_constant_turn_run():
    from pymht_amd.models import ct
    from pymht_amd.pyTarget import Target
    from pymht_amd.smoothing import score_tracks_ct
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
        nodes = list(trk.getTrackNodes()) + list(trk.__terminatedTargets__)
        with pytest.raises(NotImplementedError, match="ct"):
            trk.getTrackLikelihoods()
        with pytest.raises(NotImplementedError, match="ct"):
            nodes[0].getTrackLikelihood(trk.radarPeriod)
        with pytest.raises(ValueError, match="exclude"):
            trk.getTrackLikelihoods(constantTurn=True, ais=True)
        got = trk.getTrackLikelihoods(terminated=True, constantTurn=True)
        long_ones, direct = _scored_directly(trk, ct, nodes, score_tracks_ct)
        assert len(got) == len(nodes) and len(long_ones) >= 5 and [got[i] for i in long_ones] == direct
        assert all(np.isfinite(d[0]) for d in direct) and sum(d[2] for d in direct) >= 15
        assert nodes[long_ones[0]].getTrackLikelihood(trk.radarPeriod, constantTurn=True) == got[long_ones[0]]
    finally:
        trk.close()


def test_drop_in_path_scores_an_ais_aided_run_with_its_messages():
    from pymht_amd.models import pv
    from pymht_amd.smoothing import chain_ais, score_tracks_ais
    from test_smooth_ais_gpu import SCENE, _run_scene
    trk, record, period = _run_scene(**SCENE)
    try:
        nodes = list(trk.getTrackNodes()) + list(trk.__terminatedTargets__)
        radar_only = trk.getTrackLikelihoods(terminated=True)
        got = trk.getTrackLikelihoods(terminated=True, ais=True)
        lookup = trk._ais_lookup()
        long_ones, direct = _scored_directly(trk, pv, nodes, score_tracks_ais, extra=lambda chain: (chain_ais(chain, lookup),))
        assert len(got) == len(nodes) == len(radar_only) and len(long_ones) >= 3 and [got[i] for i in long_ones] == direct
        assert all(len(g) == 5 for g in got) and all(len(g) == 3 for g in radar_only)
        assert sum(d[4] for d in direct) >= 3 and all(np.isfinite(d[0]) and np.isfinite(d[3]) for d in direct)
        assert any(g[:3] != r for g, r in zip(got, radar_only))
        i = max(long_ones, key=lambda j: got[j][4])
        assert nodes[i].getTrackLikelihood(trk.radarPeriod, ais=True) == got[i]
        with pytest.raises(ValueError, match="exclude"):
            trk.getTrackLikelihoods(ais=True, constantTurn=True)
    finally:
        trk.close()
