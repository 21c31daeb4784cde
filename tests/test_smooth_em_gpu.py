"""GPU: the device EM smoother (`mht_smooth_tracks_em`, include/mht_amd.h seam (v), EM; pymht_amd.smoothing.smooth_tracks_em) against its
NumPy restatement tests/smooth_em_ref.py, and the drop-in path on top of it (em= on Target.getSmoothTrack, Tracker.getSmoothTracks and
_storeRun(smooth=True)).

The criterion is the smoothers' (tests/test_smooth_gpu.py): with the np.longdouble evaluation of the algorithm as the truth, over a batch
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
and e_dev <= 8 * max(e_np, eps64), for xs, Ps, Q and R separately.  The float64 reference sets the scale, never the device.  Every
test prints the ratios it measured.

Measured on an MI355X, ratios e_dev / max(e_np, eps64) on the accuracy batch, n_iter = 5, xs / Ps / Q / R (e_np between 5.6e-13 and
1.5e-11; the 4- and the 6-state build give the same figures, and they are the host twin's of tests/test_smooth_em_cpu.py):
    pv, start=model       1.15 / 0.80 / 2.88 / 1.43          pv, start=reference   1.15 / 1.09 / 1.13 / 0.99
    ca, start=model       1.26 / 1.20 / 0.08 / 1.03          ca, start=reference   1.14 / 0.58 / 0.17 / 1.98
The worst is 2.88 (Q, pv from the model's start values): F stays at the smoothers' 8.  Also in profiles/smooth_em_cost.txt."""
import ctypes as C
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import smooth_em_ref as er
import smooth_ref as sr

pytestmark = pytest.mark.gpu

PERIOD = 2.5
FACTOR = 8.0


def _model(name):
    from pymht_amd.models import pv, ca
    return {"pv": pv, "ca": ca}[name]


@pytest.fixture(scope="module")
def ctxs():
    """One context per library build: the seam takes nx at run time, so both builds run both models."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (pymht_amd has no CPU fallback)")
    from pymht_amd.device import Context
    c = {4: Context(0, nx=4), 6: Context(0, nx=6)}
    yield c
    for v in c.values():
        v.close()


def _same(a, b):
    """Two lists of per-track results (xs, Ps, Q, R), bit for bit."""
    return len(a) == len(b) and all(np.array_equal(p, q, equal_nan=True) for u, v in zip(a, b) for p, q in zip(u, v))


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_without_an_iteration_the_output_is_the_linear_smoothers_bit_for_bit(ctxs, name, lib_nx):
    """130 tracks of 1 .. 300 nodes: more than a wavefront and not a multiple of 64."""
    from pymht_amd.smoothing import smooth_tracks, smooth_tracks_em
    model = _model(name)
    lengths = [1, 2, 300, 1, 2, 3, 250] + [int(v) for v in np.random.default_rng(5).integers(1, 90, 123)]
    assert len(lengths) == 130
    tracks = sr.make_batch(model, PERIOD, lengths, seed=23, p_detect=0.8)
    lin = smooth_tracks(model, PERIOD, tracks, ctx=ctxs[lib_nx])
    got = smooth_tracks_em(model, PERIOD, tracks, n_iter=0, ctx=ctxs[lib_nx])
    Q0, R0, _ = er.start_values(model, PERIOD, tracks[0][1], "model")
    for (xs, Ps), (xs_e, Ps_e, Q, R) in zip(lin, got):
        assert np.array_equal(xs, xs_e) and np.array_equal(Ps, Ps_e)
        assert np.array_equal(Q, Q0) and np.array_equal(R, R0)
    means = smooth_tracks_em(model, PERIOD, tracks, n_iter=0, ctx=ctxs[lib_nx], covariances=False)
    assert all(m[1] is None and np.array_equal(m[0], g[0]) for m, g in zip(means, got))


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("start", ["model", "reference"])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_accuracy_against_the_longdouble_truth(ctxs, name, start, lib_nx):
    """33 tracks of 1 .. 60 nodes, five iterations: e_dev <= 8 max(e_np, eps64) for xs, Ps, Q and R."""
    from pymht_amd.smoothing import smooth_tracks_em
    assert np.finfo(np.longdouble).eps < 1e-18
    model = _model(name)
    tracks, truth, f64 = er.accuracy_reference(model, PERIOD, start)
    _, one, never, always = er.accuracy_batch(model, PERIOD)
    dev = smooth_tracks_em(model, PERIOD, tracks, n_iter=5, start=start, ctx=ctxs[lib_nx])
    got = [dict(xs=d[0], Ps=d[1], Q=d[2], R=d[3]) for d in dev]
    res = er.ratios(got, truth, f64)
    print("EM accuracy models/%s, start=%s, %d-state build: " % (name, start, lib_nx)
          + " | ".join("%s e_dev %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert all(np.isfinite(g[k]).all() for g in got for k in ("xs", "Ps", "Q", "R"))
    for k, (e, e_np, ratio) in res.items():
        assert ratio <= FACTOR, "%s: e_dev %.3g > %g x max(e_np %.3g, eps)" % (k, e, FACTOR, e_np)
    Q0, R0, P0 = er.start_values(model, PERIOD, tracks[one][1], start)
    assert np.array_equal(got[one]["xs"][0], tracks[one][0]) and np.array_equal(got[one]["Ps"][0], P0)
    assert np.array_equal(got[one]["Q"], Q0) and np.array_equal(got[one]["R"], R0)
    assert np.array_equal(got[never]["R"], R0)      # nothing seen: R stays, and the smoothed covariance of node 0 is the initial one
    eps64 = float(np.finfo(np.float64).eps)
    e_d, e_n = sr.err(got[never]["Ps"][0], P0), sr.err(f64[never]["Ps"][0], truth[never]["Ps"][0])
    print("  never detected: Ps_0 vs P_init e_dev %.3g, the reference's own error there %.3g" % (e_d, e_n))
    assert e_d <= FACTOR * max(e_n, eps64)
    assert not np.array_equal(got[always]["R"], R0) and not np.array_equal(got[always]["Q"], Q0)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_batch_independence_and_effect(ctxs, lib_nx):
    from pymht_amd.models import ca
    from pymht_amd.smoothing import smooth_tracks_em
    tracks = er.accuracy_batch(ca, PERIOD)[0]
    ctx = ctxs[lib_nx]
    got = smooth_tracks_em(ca, PERIOD, tracks, n_iter=5, start="reference", ctx=ctx)
    perm = np.random.default_rng(1).permutation(len(tracks))
    shuffled = smooth_tracks_em(ca, PERIOD, [tracks[i] for i in perm], n_iter=5, start="reference", ctx=ctx)
    assert _same([got[i] for i in perm], shuffled)
    for t in (7, 29):      # alone = inside the batch
        assert _same(smooth_tracks_em(ca, PERIOD, [tracks[t]], n_iter=5, start="reference", ctx=ctx), [got[t]])
    for xs, Ps, Q, R in got:
        assert np.array_equal(Ps, Ps.transpose(0, 2, 1)) and np.array_equal(Q, Q.T) and np.array_equal(R, R.T)
    one, zero = [smooth_tracks_em(ca, PERIOD, [tracks[29]], n_iter=k, ctx=ctx)[0] for k in (1, 0)]
    assert not np.array_equal(one[0], zero[0]) and not np.array_equal(one[2], zero[2])
    assert not np.array_equal(got[29][2], np.eye(6)) and not np.array_equal(got[29][3], np.eye(2))


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_seam_errors_leave_the_outputs_untouched(ctxs, lib_nx):
    import torch
    from pymht_amd import _lib
    from pymht_amd.models import pv
    ctx = ctxs[lib_nx]
    lib, dev = ctx.lib, ctx.device
    n, L, nx, ns = 3, 4, 4, 10
    keep = [np.ascontiguousarray(np.asarray(m, dtype=np.float32).ravel()) for m in (pv.Phi(PERIOD), pv.Q(PERIOD), pv.C_RADAR, pv.R_RADAR())]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    lens = np.array([4, 3, 1], dtype=np.int32)
    need = int(lib.mht_smooth_em_work_bytes(nx, n, L))
    assert need > 0
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    x0, P0, zz, hz = z(nx, n), torch.eye(nx, dtype=torch.float64, device=dev).reshape(nx * nx, 1).repeat(1, n).contiguous(), z(L, 2, n), torch.zeros((L, n), dtype=torch.uint8, device=dev)
    outs = [torch.full(shape, -7.0, dtype=torch.float64, device=dev) for shape in ((L, nx, n), (L, ns, n), (ns, n), (3, n))]
    work = torch.zeros(need, dtype=torch.uint8, device=dev)

    def call(n_iter, transition, work_bytes):
        mx = _lib.MhtModelX(nx, fp(keep[0]), fp(keep[1]), fp(keep[2]), fp(keep[3]), 0.0, 0.0, transition, PERIOD)
        torch.cuda.synchronize(dev)
        return lib.mht_smooth_tracks_em(ctx.handle, C.byref(mx), n, L, lens.ctypes.data_as(C.c_void_p), x0.data_ptr(), P0.data_ptr(), zz.data_ptr(),
                                        hz.data_ptr(), n_iter, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                        work.data_ptr(), work_bytes)
    for n_iter, transition, work_bytes in ((-1, 0, need), (65, 0, need), (5, 1, need), (5, 0, need - 1)):
        assert call(n_iter, transition, work_bytes) == _lib.MHT_E_INVALID
        assert lib.mht_last_error()
        torch.cuda.synchronize(dev)
        assert all(bool((o == -7.0).all()) for o in outs)
    assert call(64, 0, need) == _lib.MHT_OK      # (the bounds themselves are fine)
    assert not any(bool((o[..., 0] == -7.0).all()) for o in (outs[0][:1], outs[2], outs[3]))


def _run_scenario():
    from pymht_amd.tracker import Tracker
    from pymht_amd.models import pv
    from pymht_amd.utils.classDefinitions import MeasurementList
    from pymht_amd.utils.scenario import make_scenario
    sc = make_scenario(T=30, radius=2000.0, lambda_phi=2e-6, n_scans=25, P_d=0.9, seed=4711)
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=5, eta2=5.99)
    for zk, tk in zip(sc["scans"], sc["times"]):
        trk.addMeasurementList(MeasurementList(float(tk), zk))
    return trk, sc, pv


def test_drop_in_path_learns_and_fills_the_export():
    from pymht_amd.smoothing import chain_inputs, smooth_tracks_em
    trk, sc, pv = _run_scenario()
    try:
        nodes = list(trk.getTrackNodes()) + list(trk.__terminatedTargets__)
        got = trk.getSmoothTracks(terminated=True, em=5)
        assert len(got) == len(nodes)
        long_ones = [i for i, node in enumerate(nodes) if len(node.backtrackNodes()) >= 2]
        assert len(long_ones) >= 5
        direct = smooth_tracks_em(pv, sc["period"], [chain_inputs(nodes[i], pv.P0)[1] for i in long_ones], n_iter=5, ctx=trk._ctx, covariances=False)
        for i, (xs, _, Q, R) in zip(long_ones, direct):
            pos, vel, ok = got[i]
            assert ok == bool(np.isfinite(xs).all())
            assert np.array_equal(pos, xs[:, 0:2], equal_nan=True) and np.array_equal(vel, xs[:, 2:4], equal_nan=True)
        assert sum(got[i][2] for i in long_ones) >= 5
        plain = trk.getSmoothTracks(terminated=True)
        assert any(not np.array_equal(got[i][0], plain[i][0]) for i in long_ones)
        i = max(long_ones, key=lambda j: len(nodes[j].backtrackNodes()))
        pos1, vel1, ok1 = nodes[i].getSmoothTrack(trk.radarPeriod, em=5)
        assert ok1 == got[i][2] and np.array_equal(pos1, got[i][0], equal_nan=True) and np.array_equal(vel1, got[i][1], equal_nan=True)
        # the export: em=0 is byte-identical to a run without the keyword; em=5 fills <SmoothedStates> with the learned smoother's numbers
        a, b, c = trk.getScenarioElement(), trk.getScenarioElement(), trk.getScenarioElement()
        trk._storeRun(a, smooth=True)
        trk._storeRun(b, smooth=True, em=0)
        trk._storeRun(c, smooth=True, em=5, emStart="model")
        assert ET.tostring(a) == ET.tostring(b)
        filled = 0
        for node, (pos, vel, ok), tr_ in zip(nodes, got, c.find("Run").findall("Track")):
            sm = tr_.find("SmoothedStates")
            assert sm.attrib == {"em": "5", "emStart": "model"}
            if len(pos) < 2 or not ok:
                assert len(sm) == 0
                continue
            assert len(sm) == len(pos)
            filled += 1
            for s_el, p, v in zip(sm, pos, vel):
                assert float(s_el.find("P").find("E").text) == round(float(p[0]), 2) and float(s_el.find("P").find("N").text) == round(float(p[1]), 2)
                assert float(s_el.find("V").find("E").text) == round(float(v[0]), 2) and float(s_el.find("V").find("N").text) == round(float(v[1]), 2)
        assert filled >= 5
        assert all(tr_.find("SmoothedStates").attrib == {} for tr_ in a.find("Run").findall("Track"))
        with pytest.raises(ValueError, match="em"):
            trk.getSmoothTracks(em=5, ais=True)
        with pytest.raises(ValueError, match="em"):
            trk._storeRun(trk.getScenarioElement(), smooth=True, em=5, ais=True)
    finally:
        trk.close()
