"""GPU: the device filter of track histories (`mht_filter_tracks`, `mht_filter_tracks_ct`, `mht_filter_tracks_ais`, include/mht_amd.h;
pymht_amd.smoothing.filter_tracks*) and the drop-in path on top (Tracker.getFilteredTracks), against tests/filter_ref.py and against
the device smoother of the same batches.

The criterion is the smoothers' (tests/test_smooth_trace_gpu.py), per output family (xf, Pf): with the np.longdouble evaluation of the
reference as the truth, over the cells of a batch that are not NaN in it,
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
and e_dev <= 8 * max(e_np, eps64); the NaN cells are the truth's exactly.  The float64 reference sets the scale, never the device.  The
host twin of the same header measures ratios of 0.25 - 1.06 on batches of the same make (tests/test_filter_cpu.py); every test prints
the device's own -- measured on an MI355X, both builds alike, xf / Pf: pv 1.23 / 0.55 (e_np 3.9e-13 / 3.5e-14), ca 1.00 / 0.94
(7.4e-13 / 1.1e-13), ct 0.85 / 1.12 (6.8e-13 / 3.2e-10), AIS 0.96 / 0.40 (4.6e-13 / 1.9e-12), AIS without messages 1.00 / 0.53
(3.3e-13 / 8.1e-14) -- and tools/nees_cost.py writes them into profiles/nees_cost.txt.  Nothing here is larger than 130 tracks of 60
nodes."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as ref
import smooth_ref as sr

pytestmark = pytest.mark.gpu

PERIOD = 2.5
FACTOR = 8.0
SENTINEL = -7.0
N_TRACKS = 130      # lengths 1, 2, 60, 7, 33 in turn: two wavefronts and a bit, the shortest tracks next to the longest
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


def _raw(ctx, model, tracks, L_max, kind="linear", lens=None, work_bytes=None, nulls=(), model_nx=None, transition=None, seam=None):
    """One call of a filter seam on `tracks` in the order given (no sorting: a track's lane is its index), in arrays of L_max rows, the
    outputs pre-filled with SENTINEL: (return code, xf [L_max, nx, n], Pf [L_max, ns, n]) as NumPy arrays."""
    import torch
    from pymht_amd.smoothing import _ais_inputs, _model_x
    lib, dev = ctx.lib, ctx.device
    n, nx = len(tracks), len(tracks[0][0])
    ns = nx * (nx + 1) // 2
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    zp, hp = np.zeros((L_max, 2, n)), np.zeros((L_max, n), dtype=np.uint8)
    for j, t in enumerate(tracks):
        z = np.asarray(t[2], dtype=np.float64)
        has = sr.detected(z)
        has[0] = False
        zp[:len(z), :, j], hp[:len(z), j] = np.where(has[:, None], z, 0.0), has
    arrays = {"x": up(np.stack([np.asarray(t[0], dtype=np.float64) for t in tracks], axis=1)),
              "P": up(np.stack([np.asarray(t[1], dtype=np.float64).ravel() for t in tracks], axis=1)), "z": up(zp), "h": up(hp)}
    outs = [torch.full((L_max, nx, n), SENTINEL, dtype=torch.float64, device=dev), torch.full((L_max, ns, n), SENTINEL, dtype=torch.float64, device=dev)]
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
    need = int(lib.mht_filter_work_bytes(nx, n, L_max))
    work = torch.zeros(max(need, 256), dtype=torch.uint8, device=dev)
    mx, keep = _model_x(model, PERIOD, nx, kind == "ct")
    if model_nx is not None:
        mx.nx = model_nx
    if transition is not None:
        mx.transition = transition
    lens = np.array([len(t[2]) for t in tracks] if lens is None else lens, dtype=np.int32)
    ptr = lambda name: None if name in nulls else arrays[name].data_ptr()
    torch.cuda.synchronize(dev)
    fn = getattr(lib, seam or {"linear": "mht_filter_tracks", "ct": "mht_filter_tracks_ct", "ais": "mht_filter_tracks_ais"}[kind])
    rc = fn(ctx.handle, C.byref(mx), n, L_max, None if "len" in nulls else lens.ctypes.data_as(C.c_void_p), ptr("x"), ptr("P"), ptr("z"), ptr("h"),
            *extra, None if "xf" in nulls else outs[0].data_ptr(), None if "Pf" in nulls else outs[1].data_ptr(),
            None if "work" in nulls else work.data_ptr(), need if work_bytes is None else work_bytes)
    torch.cuda.synchronize(dev)
    return rc, outs[0].cpu().numpy(), outs[1].cpu().numpy()


def _hold(label, got, truth, f64):
    res = ref.ratios(got, truth, f64, ref.NAMES)
    print(label + ": " + " | ".join("%s e_dev %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert ref.same_nan(got, truth, ref.NAMES), "the NaN cells are not the truth's"
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, "%s: e_dev %.3g > %g x max(e_np %.3g, eps)" % (k, e, FACTOR, e_np)


def _same_bits(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


CASES = [("linear", "pv", 4), ("linear", "pv", 6), ("linear", "ca", 4), ("linear", "ca", 6), ("ct", "ct", 6), ("ais", "pv", 4), ("ais-none", "pv", 4)]


@pytest.mark.parametrize("kind,name,lib_nx", CASES)
def test_filter_accuracy_every_cell_written_last_node_is_the_smoothers_and_place_does_not_matter(ctxs, kind, name, lib_nx):
    """filter_ref.edge_batch: 130 tracks of 1, 2, 60, 7, 33 nodes in turn, every fourth never detected.
    - the raw seam on arrays of 64 rows preset to a sentinel, the tracks in the order given: no cell keeps the sentinel, the rows behind
      a track's end are NaN, node 0 is (x_init, P_init)
    - the Python layer (which packs the batch sorted by length) gives the raw call's bits, and meets the criterion against
      tests/filter_ref.py
    - every track's last node is the last node of smooth_tracks* on the same batch and context, bit for bit
    - the same batch permuted gives the same bits per track; without its messages an AIS batch is the linear filter, bit for bit"""
    from pymht_amd import smoothing
    assert np.finfo(np.longdouble).eps < 1e-18
    model, ctx = _model(name), ctxs[lib_nx]
    seam_kind = "ais" if kind == "ais-none" else kind
    tracks, truth, f64 = ref.reference(kind, model, PERIOD, N_TRACKS, SEED)
    nx = len(tracks[0][0])
    rc, xf, Pf = _raw(ctx, model, tracks, L_MAX, seam_kind)
    assert rc == 0 and not (xf == SENTINEL).any() and not (Pf == SENTINEL).any()
    run = {"linear": smoothing.filter_tracks, "ct": smoothing.filter_tracks_ct, "ais": smoothing.filter_tracks_ais}[seam_kind]
    smooth = {"linear": smoothing.smooth_tracks, "ct": smoothing.smooth_tracks_ct, "ais": smoothing.smooth_tracks_ais}[seam_kind]
    dev = run(model, PERIOD, tracks, ctx=ctx)
    got = [dict(xf=a, Pf=b) for a, b in dev]
    _hold("filter accuracy %s models/%s, %d-state build" % (kind, name, lib_nx), got, truth, f64)
    sm = smooth(model, PERIOD, tracks, ctx=ctx)
    for j, (t, (a, b), (xs, Ps)) in enumerate(zip(tracks, dev, sm)):
        L = len(t[2])
        assert a.shape == (L, nx) and b.shape == (L, nx, nx) and a.dtype == b.dtype == np.float64
        assert np.isnan(xf[L:, :, j]).all() and np.isnan(Pf[L:, :, j]).all() and np.isfinite(a).all() and np.isfinite(b).all()
        assert np.array_equal(xf[:L, :, j], a) and np.array_equal(ref.full(Pf[:L, :, j], nx), b)
        assert np.array_equal(a[0], t[0]) and np.array_equal(b[0], t[1])
        assert np.array_equal(a[L - 1], xs[L - 1]) and np.array_equal(b[L - 1], Ps[L - 1]), "track %d: the last node is not the smoother's" % j
    perm = np.random.default_rng(2).permutation(N_TRACKS)
    again = run(model, PERIOD, [tracks[i] for i in perm], ctx=ctx)
    assert all(_same_bits(again[j], dev[i]) for j, i in enumerate(perm))
    assert _same_bits(run(model, PERIOD, [tracks[127]], ctx=ctx)[0], dev[127])
    if kind == "ais":
        assert sum(sum(a is not None for a in t[3]) for t in tracks) > 300
    if kind == "ais-none":
        lin = smoothing.filter_tracks(model, PERIOD, [t[:3] for t in tracks], ctx=ctx)
        assert all(_same_bits(p, q) for p, q in zip(dev, lin))


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_every_cell_is_written_around_a_wavefront_boundary(ctxs, n):
    """One track, a wavefront less one, a wavefront, one more (130 is the accuracy test's): no cell keeps the sentinel, and what is
    there is the float64 reference's numbers."""
    from pymht_amd.models import ca
    tracks = ref.edge_batch("linear", ca, PERIOD, n, seed=40 + n)
    rc, xf, Pf = _raw(ctxs[6], ca, tracks, L_MAX)
    assert rc == 0 and not (xf == SENTINEL).any() and not (Pf == SENTINEL).any()
    for j in sorted({0, n // 2, n - 1}):
        L, f = len(tracks[j][2]), ref.run("linear", ca, PERIOD, tracks[j])
        assert np.isnan(xf[L:, :, j]).all() and np.isnan(Pf[L:, :, j]).all()
        assert np.allclose(xf[:L, :, j], f["xf"], rtol=1e-9, atol=1e-9) and np.allclose(ref.full(Pf[:L, :, j], 6), f["Pf"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_raw_abi_errors_and_the_calls_behind_them(ctxs, lib_nx):
    """A null array, a length outside 1 .. L_max, a short workspace, a wrong nx or transition for the seam: MHT_E_INVALID each, with the
    sentinel in the outputs untouched; an empty batch is MHT_OK and writes nothing; the call behind them on the same context is right."""
    from pymht_amd import _lib
    from pymht_amd.models import ct, pv
    from pymht_amd.smoothing import _model_x, filter_tracks
    import smooth_ct_ref as cr
    ctx = ctxs[lib_nx]
    lib = ctx.lib
    tracks = sr.make_batch(pv, PERIOD, [4, 3, 1], seed=2, p_detect=1.0)
    ais_tracks = [t + ([None] * len(t[2]),) for t in tracks]
    ct_tracks = cr.make_batch(ct, PERIOD, [4, 3, 1], seed=2)
    need = int(lib.mht_filter_work_bytes(4, 3, 4))
    assert need == 256
    bad = [dict(nulls=("len",)), dict(nulls=("x",)), dict(nulls=("z",)), dict(nulls=("h",)), dict(nulls=("xf",)), dict(nulls=("Pf",)),
           dict(nulls=("work",)), dict(lens=[4, 0, 1]), dict(lens=[4, 5, 1]), dict(work_bytes=need - 1), dict(model_nx=5), dict(transition=1),
           dict(seam="mht_filter_tracks_ct"), dict(seam="mht_filter_tracks_ct", transition=1)]      # (ct: nx 4 is not its model)
    for kw in bad:
        rc, xf, Pf = _raw(ctx, pv, tracks, 4, **kw)
        assert rc == _lib.MHT_E_INVALID and lib.mht_last_error(), kw
        assert (xf == SENTINEL).all() and (Pf == SENTINEL).all(), kw
    for kw in (dict(model_nx=6), dict(transition=1), dict(nulls=("Pf",)), dict(work_bytes=need - 1)):
        rc, xf, Pf = _raw(ctx, pv, ais_tracks, 4, "ais", **kw)
        assert rc == _lib.MHT_E_INVALID and (xf == SENTINEL).all() and (Pf == SENTINEL).all(), kw
    for kw in (dict(transition=0), dict(lens=[4, 3, 9])):
        rc, xf, Pf = _raw(ctx, ct, ct_tracks, 4, "ct", **kw)
        assert rc == _lib.MHT_E_INVALID and (xf == SENTINEL).all() and (Pf == SENTINEL).all(), kw
    import torch
    mx, keep = _model_x(pv, PERIOD, 4, False)
    torch.cuda.synchronize(ctx.device)
    assert lib.mht_filter_tracks(ctx.handle, C.byref(mx), 0, 4, None, None, None, None, None, None, None, None, 0) == _lib.MHT_OK
    rc, xf, Pf = _raw(ctx, pv, tracks, 4)
    assert rc == _lib.MHT_OK and not (xf == SENTINEL).any() and not (Pf == SENTINEL).any()
    for j, (a, b) in enumerate(filter_tracks(pv, PERIOD, tracks, ctx=ctx)):
        L = len(a)
        assert np.array_equal(xf[:L, :, j], a) and np.array_equal(ref.full(Pf[:L, :, j], 4), b) and np.isnan(xf[L:, :, j]).all()


def test_drop_in_path_filters_the_tracks_of_a_run():
    """A dozen scans over six preinitialised targets on models/pv: getFilteredTracks is filter_nodes on the tracker's nodes, a row per
    node of each history, its last rows the states behind getSmoothTracks' last rows; a node's getFilteredTrack is its entry; a
    constant-turn tracker refuses without its switch."""
    from pymht_amd.models import ct, pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.smoothing import chain_inputs, filter_nodes, smooth_tracks
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
        got = trk.getFilteredTracks(terminated=True)
        assert len(got) == len(nodes) and len(live) > 0 and len(trk.getFilteredTracks()) == len(live)
        direct = filter_nodes(pv, trk.radarPeriod, nodes, ctx=trk._ctx)
        assert all(_same_bits(g, d) for g, d in zip(got, direct))
        sm = smooth_tracks(pv, trk.radarPeriod, [chain_inputs(node, pv.P0)[1] for node in nodes], ctx=trk._ctx)
        for (xf, Pf), node, (xs, Ps) in zip(got, nodes, sm):
            L = len(node.backtrackNodes())
            assert xf.shape == (L, 4) and Pf.shape == (L, 4, 4) and np.isfinite(xf).all() and np.isfinite(Pf).all()
            assert np.array_equal(xf[-1], xs[-1]) and np.array_equal(Pf[-1], Ps[-1])
        i = max(range(len(nodes)), key=lambda j: len(got[j][0]))
        assert len(got[i][0]) >= 10 and _same_bits(nodes[i].getFilteredTrack(trk.radarPeriod), got[i])
        with pytest.raises(ValueError, match="constant-turn"):
            trk.getFilteredTracks(constantTurn=True)
        with pytest.raises(ValueError, match="aisAided"):
            trk.getFilteredTracks(ais=True)
    finally:
        trk.close()
    turning = Tracker(ct, PERIOD, 1e-7, 1e-4, P_d=0.9, N=4, eta2=5.99, useInitiator=False)
    try:
        with pytest.raises(NotImplementedError, match="ct"):
            turning.getFilteredTracks()
        assert turning.getFilteredTracks(constantTurn=True) == []
    finally:
        turning.close()
