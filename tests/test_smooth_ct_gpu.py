"""GPU: the constant-turn Rauch-Tung-Striebel smoother (`mht_smooth_tracks_ct`, include/mht_amd.h; pymht_amd.smoothing.smooth_tracks_ct)
against its NumPy restatement tests/smooth_ct_ref.py, and the opt-in drop-in path on top of it (constantTurn=True of
Target.getSmoothTrack, Tracker.getSmoothTracks and Tracker._storeRun).

The criterion is the linear smoother's (tests/test_smooth_gpu.py), factor unchanged: with the np.longdouble evaluation as the truth,
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
means and covariances separately, and  e_dev <= 8 * e_np.  The transition is rebuilt at every node from the filtered turn rate, so the
device's own float64 sin / cos are part of what is measured.  Every test prints the ratios it measured."""
import ctypes as C
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import smooth_ct_ref as cr
import smooth_ref as sr

pytestmark = pytest.mark.gpu

PERIOD = 2.5
FACTOR = 8.0


@pytest.fixture(scope="module")
def ctxs():
    """One context per library build: the seam does not depend on the build's state dimension."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (pymht_amd has no CPU fallback)")
    from pymht_amd.device import Context
    c = {4: Context(0, nx=4), 6: Context(0, nx=6)}
    yield c
    for v in c.values():
        v.close()


def _truth_is_better_than_float64():
    eps = float(np.finfo(np.longdouble).eps)
    assert eps < 1e-18, "np.longdouble is no wider than float64 here (eps %.3g): the accuracy criterion would be empty" % eps


def _references(model, tracks, period=PERIOD):
    mats = cr.model_matrices(model, period)
    truth = [cr.rts_ct(*mats, x0, P0, z, dtype=np.longdouble) for x0, P0, z in tracks]
    f64 = [cr.rts_ct(*mats, x0, P0, z, dtype=np.float64) for x0, P0, z in tracks]
    return truth, f64


def _worst(got, truth, key):
    return max(sr.err(g, t[key]) for g, t in zip(got, truth))


def _check(label, dev, truth, f64):
    """The criterion of the module docstring over a batch; dev = [(xs, Ps)]."""
    e_dev = (_worst([d[0] for d in dev], truth, "xs"), _worst([d[1] for d in dev], truth, "Ps"))
    e_np = (_worst([f["xs"] for f in f64], truth, "xs"), _worst([f["Ps"] for f in f64], truth, "Ps"))
    print("%s: means e_dev %.3g e_np %.3g ratio %.3g | covariances e_dev %.3g e_np %.3g ratio %.3g"
          % (label, e_dev[0], e_np[0], e_dev[0] / e_np[0] if e_np[0] else 0.0, e_dev[1], e_np[1], e_dev[1] / e_np[1] if e_np[1] else 0.0))
    assert e_dev[0] <= FACTOR * e_np[0], "%s: means: e_dev %.3g > %g x e_np %.3g" % (label, e_dev[0], FACTOR, e_np[0])
    assert e_dev[1] <= FACTOR * e_np[1], "%s: covariances: e_dev %.3g > %g x e_np %.3g" % (label, e_dev[1], FACTOR, e_np[1])
    return e_dev, e_np


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_accuracy_against_the_longdouble_truth(ctxs, lib_nx):
    """40 tracks of 2 .. 400 nodes, 80 % detections, T = 2.5: turn rates from exactly 0 to 0.6 rad/s, half the tracks with a coupled
    P_init so that the filtered turn rate moves with the data (tests/test_smooth_ct_cpu.py asserts that it does)."""
    from pymht_amd.models import ct
    from pymht_amd.smoothing import smooth_tracks_ct
    _truth_is_better_than_float64()
    rng = np.random.default_rng(20240)
    lengths = [int(v) for v in rng.integers(2, 401, 40)]
    tracks = cr.make_batch(ct, PERIOD, lengths, seed=17, p_detect=0.8)
    dev = smooth_tracks_ct(ct, PERIOD, tracks, ctx=ctxs[lib_nx])
    truth, f64 = _references(ct, tracks)
    _check("accuracy models/ct, %d-state build" % lib_nx, dev, truth, f64)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_mixed_batch_shapes_and_properties(ctxs, lib_nx):
    """One call with lengths from 1 to 300, more tracks than a wavefront has lanes and not a multiple of 64; tracks never detected after
    node 0, tracks always detected; plus the properties that need no reference."""
    from pymht_amd.models import ct
    from pymht_amd.smoothing import smooth_tracks_ct
    _truth_is_better_than_float64()
    rng = np.random.default_rng(5)
    lengths = [1, 2, 300, 1, 2, 3, 250] + [int(v) for v in rng.integers(1, 90, 123)]
    n = len(lengths)
    assert n == 130 and n > 64 and n % 64 != 0
    p_detect = np.full(n, 0.8)
    never, always = [1, 5, 9, 20, 40, 70, 100], [2, 6, 10, 21, 41, 71, 101]
    p_detect[never], p_detect[always] = 0.0, 1.0
    tracks = cr.make_batch(ct, PERIOD, lengths, seed=23, p_detect=p_detect)
    dev = smooth_tracks_ct(ct, PERIOD, tracks, ctx=ctxs[lib_nx])
    truth, f64 = _references(ct, tracks)
    label = "mixed models/ct, %d-state build" % lib_nx
    _check(label, dev, truth, f64)
    for (x0, P0, z), (xs, Ps) in zip(tracks, dev):
        assert xs.shape == (len(z), 6) and Ps.shape == (len(z), 6, 6) and xs.dtype == np.float64 and Ps.dtype == np.float64
        if len(z) == 1:      # nothing to smooth: output = input, exactly
            assert np.array_equal(xs[0], x0) and np.array_equal(Ps[0], P0)
        assert np.array_equal(Ps, Ps.transpose(0, 2, 1)), "Ps is not symmetric"
    assert any(len(t[2]) == 1 and not np.array_equal(t[1], ct.P0) for t in tracks)      # (a one-node track with the coupled P_init among them)
    for t in never:
        assert np.isnan(tracks[t][2]).all()
    for t in always:
        assert not np.isnan(tracks[t][2][1:]).any()
    # the last node is the forward filter's last node (same criterion, against the truth's filtered state)
    e_d = (max(sr.err(d[0][-1], t["xf"][-1]) for d, t in zip(dev, truth)), max(sr.err(d[1][-1], t["Pf"][-1]) for d, t in zip(dev, truth)))
    e_n = (max(sr.err(f["xf"][-1], t["xf"][-1]) for f, t in zip(f64, truth)), max(sr.err(f["Pf"][-1], t["Pf"][-1]) for f, t in zip(f64, truth)))
    print("%s: last node vs the filter's: means e_dev %.3g e_np %.3g | covariances e_dev %.3g e_np %.3g" % (label, e_d[0], e_n[0], e_d[1], e_n[1]))
    assert e_d[0] <= FACTOR * e_n[0] and e_d[1] <= FACTOR * e_n[1]
    # smoothing never adds uncertainty: trace(Ps_k) <= trace(Pf_k), Pf from the reference (slack as in tests/test_smooth_gpu.py: 1e-9
    # relative, two orders above the float64 reference's own covariance error, nine below the traces)
    tr = lambda M: np.trace(M, axis1=1, axis2=2)
    for (xs, Ps), f in zip(dev, f64):
        assert np.all(tr(Ps) <= tr(f["Pf"]) * (1 + 1e-9) + 1e-9)
    # a track's result does not depend on its place in the batch or on its neighbours: permuting the batch permutes the outputs bit for bit
    perm = rng.permutation(n)
    dev_p = smooth_tracks_ct(ct, PERIOD, [tracks[i] for i in perm], ctx=ctxs[lib_nx])
    for j, i in enumerate(perm):
        assert np.array_equal(dev_p[j][0], dev[i][0]) and np.array_equal(dev_p[j][1], dev[i][1])
    # ... nor on the others being there at all, nor on whether the covariances are asked for
    alone = smooth_tracks_ct(ct, PERIOD, [tracks[2]], ctx=ctxs[lib_nx])[0]
    assert np.array_equal(alone[0], dev[2][0]) and np.array_equal(alone[1], dev[2][1])
    means = smooth_tracks_ct(ct, PERIOD, tracks, ctx=ctxs[lib_nx], covariances=False)
    for (xs, Ps), (xs_m, none) in zip(dev, means):
        assert none is None and np.array_equal(xs, xs_m)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_raw_abi_error_codes_leave_the_outputs_untouched(ctxs, lib_nx):
    import torch
    from pymht_amd import _lib
    from pymht_amd.models import ct
    ctx = ctxs[lib_nx]
    lib, dev = ctx.lib, ctx.device
    nx, n, L = 6, 3, 5
    keep = [np.ascontiguousarray(np.asarray(m, dtype=np.float32).ravel()) for m in (ct.Q(PERIOD), ct.C_RADAR, ct.R_RADAR())]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    # (A is ignored and may be null)
    model = lambda nx_=6, transition=1, period=PERIOD: _lib.MhtModelX(nx_, None, fp(keep[0]), fp(keep[1]), fp(keep[2]), 0.0, 0.0, transition, period)
    x = torch.zeros((nx, n), dtype=torch.float64, device=dev)
    x[4] = 0.05
    P = torch.eye(nx, dtype=torch.float64, device=dev).reshape(nx * nx, 1).repeat(1, n).contiguous()
    z = torch.zeros((L, 2, n), dtype=torch.float64, device=dev)
    h = torch.ones((L, n), dtype=torch.uint8, device=dev)
    xs = torch.full((L, nx, n), -7.0, dtype=torch.float64, device=dev)
    Ps = torch.full((L, nx * (nx + 1) // 2, n), -7.0, dtype=torch.float64, device=dev)
    need = int(lib.mht_smooth_ct_work_bytes(n, L))
    assert need == 256 + L * 27 * n * 8
    work = torch.zeros(need, dtype=torch.uint8, device=dev)

    def call(m, lens, work_bytes, L_=L):
        lens = np.asarray(lens, dtype=np.int32)
        return lib.mht_smooth_tracks_ct(ctx.handle, C.byref(m), n, L_, lens.ctypes.data_as(C.c_void_p), x.data_ptr(), P.data_ptr(), z.data_ptr(),
                                        h.data_ptr(), xs.data_ptr(), Ps.data_ptr(), work.data_ptr(), work_bytes)

    untouched = lambda: bool((xs == -7.0).all()) and bool((Ps == -7.0).all())
    assert call(model(transition=0), [5, 5, 5], need) == _lib.MHT_E_INVALID and untouched()      # a linear model belongs to mht_smooth_tracks
    assert b"mht_smooth_tracks" in lib.mht_last_error()
    assert call(model(nx_=4), [5, 5, 5], need) == _lib.MHT_E_INVALID and untouched()
    assert call(model(), [5, 5, 5], need, L_=0) == _lib.MHT_E_INVALID and untouched()
    assert call(model(), [5, 0, 5], need) == _lib.MHT_E_INVALID and untouched()
    assert call(model(), [5, 6, 5], need) == _lib.MHT_E_INVALID and untouched()
    assert call(model(), [5, 5, 5], need - 1) == _lib.MHT_E_CAPACITY and untouched()
    assert b"workspace" in lib.mht_last_error()
    assert call(model(), [5, 2, 1], need) == _lib.MHT_OK
    got, got_P = xs.cpu().numpy(), Ps.cpu().numpy()
    for t, length in enumerate([5, 2, 1]):      # exactly the nodes of each track's length
        assert not (got[:length, :, t] == -7.0).any() and (got[length:, :, t] == -7.0).all()
        assert not (got_P[:length, :, t] == -7.0).any() and (got_P[length:, :, t] == -7.0).all()
    # and the linear seam still refuses the model
    lin = model()
    assert lib.mht_smooth_tracks(ctx.handle, C.byref(lin), n, L, np.array([5, 5, 5], dtype=np.int32).ctypes.data_as(C.c_void_p), x.data_ptr(), P.data_ptr(),
                                 z.data_ptr(), h.data_ptr(), xs.data_ptr(), Ps.data_ptr(), work.data_ptr(), need) == _lib.MHT_E_INVALID


def _turning_scene(n_scans=36, seed=77):
    """Eight well separated targets, some turning, one lost half way; scans of float32 detections (P_d 0.9) and a little clutter."""
    rng = np.random.default_rng(seed)
    w0 = [0.0, 0.03, -0.05, 0.0, 0.12, -0.2, 0.008, 0.3]
    a0 = [0.0, 0.0, 0.0004, 0.0, 0.0, 0.0, -0.0001, 0.0]
    x0 = np.array([[-3000.0 + 900.0 * i, 2000.0 - 600.0 * i, rng.uniform(4, 9) * (1 if i % 2 else -1), rng.uniform(-8, 8), w0[i], a0[i]] for i in range(8)])
    x, scans, times = x0.copy(), [], []
    for k in range(n_scans):
        for i in range(8):
            x[i] = cr.phi(PERIOD, x[i, 4], np.float64) @ x[i]
        x[:, 2:4] += rng.normal(0.0, 0.05, (8, 2))
        seen = rng.uniform(size=8) <= 0.9
        seen[3] &= k < n_scans // 2
        det = x[seen, 0:2] + rng.normal(0.0, 2.5, (int(seen.sum()), 2))
        clutter = rng.uniform(-4000.0, 4000.0, (rng.poisson(2.0), 2))
        z = np.concatenate([det, clutter], axis=0)
        rng.shuffle(z, axis=0)
        scans.append(np.ascontiguousarray(z, dtype=np.float32).reshape(-1, 2))
        times.append(1000.0 + (k + 1) * PERIOD)
    return x0, scans, times


def test_drop_in_path_smooths_a_constant_turn_run_and_fills_the_export():
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import ct, pv
    from pymht_amd.utils.classDefinitions import MeasurementList
    _truth_is_better_than_float64()
    x0, scans, times = _turning_scene()
    trk = Tracker(ct, PERIOD, 1e-7, 1e-4, P_d=0.9, N=4, eta2=5.99, useInitiator=False)
    try:
        for x in x0:
            trk.initiateTarget(Target(1000.0, None, x.copy(), ct.P0, status="preinitialized"))
        for zk, tk in zip(scans, times):
            trk.addMeasurementList(MeasurementList(float(tk), zk))
        nodes = list(trk.getTrackNodes()) + list(trk.__terminatedTargets__)
        assert len(trk.getTrackNodes()) >= 5
        # the default calls still refuse
        with pytest.raises(NotImplementedError, match="ct"):
            trk.getSmoothTracks()
        with pytest.raises(NotImplementedError, match="ct"):
            trk._storeRun(trk.getScenarioElement(), smooth=True)
        with pytest.raises(NotImplementedError, match="ct"):
            nodes[0].getSmoothTrack(trk.radarPeriod)
        got = trk.getSmoothTracks(terminated=True, constantTurn=True)
        assert len(got) == len(nodes) and len(trk.getSmoothTracks(constantTurn=True)) == len(trk.getTrackNodes())
        mats = cr.model_matrices(ct, PERIOD)
        dev, truth, f64, longest, turning = [], [], [], 0, 0
        for i, (node, (pos, vel, ok)) in enumerate(zip(nodes, got)):
            chain = node.backtrackNodes()
            zs = node.backtrackMeasurement()
            assert len(zs) == len(chain) == len(pos) == len(vel)
            if len(chain) < 2:
                assert not ok and np.isnan(vel).all()
                continue
            assert ok
            first = chain[0]
            args = (first.x_0, ct.P0 if first.P_0 is None else first.P_0, zs)
            turning += bool(np.asarray(first.x_0)[4] != 0)
            truth.append(cr.rts_ct(*mats, *args, dtype=np.longdouble))
            f64.append(cr.rts_ct(*mats, *args, dtype=np.float64))
            dev.append(np.concatenate([pos, vel], axis=1))
            if len(chain) > len(nodes[longest].backtrackNodes()):
                longest = i
        assert len(dev) >= 5 and turning >= 3 and max(len(d) for d in dev) >= 20
        e_dev = max(sr.err(d, t["xs"][:, :4]) for d, t in zip(dev, truth))
        e_np = max(sr.err(f["xs"][:, :4], t["xs"][:, :4]) for f, t in zip(f64, truth))
        print("drop-in models/ct: %d tracks, longest %d nodes: means e_dev %.3g e_np %.3g ratio %.3g" % (len(dev), max(len(d) for d in dev), e_dev, e_np, e_dev / e_np))
        assert e_dev <= FACTOR * e_np
        # one node on its own: the same numbers as its row of the batch, bit for bit
        pos1, vel1, ok1 = nodes[longest].getSmoothTrack(trk.radarPeriod, constantTurn=True)
        assert ok1 and np.array_equal(pos1, got[longest][0]) and np.array_equal(vel1, got[longest][1])
        # the export: one <S> per node with smooth=True and constantTurn=True, in the layout and at the precision of <States>
        scen = trk.getScenarioElement()
        trk._storeRun(scen)
        trk._storeRun(scen, smooth=True, constantTurn=True)
        plain, smooth = scen.findall("Run")
        assert len(plain.findall("Track")) == len(smooth.findall("Track")) == len(nodes)
        for tr_ in plain.findall("Track"):
            assert len(tr_.find("SmoothedStates")) == 0
        filled = 0
        for node, (pos, vel, ok), tr_ in zip(nodes, got, smooth.findall("Track")):
            states, sm = tr_.find("States"), tr_.find("SmoothedStates")
            assert len(states) == int(tr_.attrib["length"]) == len(pos)
            if len(states) < 2:
                assert len(sm) == 0
                continue
            assert len(sm) == len(states)
            filled += 1
            for s_el, f_el, p, v in zip(sm, states, pos, vel):
                assert s_el.tag == "S" and s_el.attrib["t"] == f_el.attrib["t"]
                assert [c.tag for c in s_el] == ["P", "V"] and [c.tag for c in s_el.find("P")] == ["N", "E"] == [c.tag for c in s_el.find("V")]
                assert float(s_el.find("P").find("E").text) == round(float(p[0]), 2) and float(s_el.find("P").find("N").text) == round(float(p[1]), 2)
                assert float(s_el.find("V").find("E").text) == round(float(v[0]), 2) and float(s_el.find("V").find("N").text) == round(float(v[1]), 2)
        assert filled >= 5
        ET.fromstring(ET.tostring(scen))      # (well-formed)
    finally:
        trk.close()
    # a tracker on a linear model has no turn rate to read
    trk = Tracker(pv, PERIOD, 1e-7, 1e-4, P_d=0.9, N=3, useInitiator=False)
    try:
        tgt = Target(1000.0, None, np.array([10.0, 20.0, 3.0, -2.0]), pv.P0, status="preinitialized")
        trk.initiateTarget(tgt)
        with pytest.raises(ValueError, match="turn"):
            trk.getSmoothTracks(constantTurn=True)
        with pytest.raises(ValueError, match="turn"):
            trk._storeRun(trk.getScenarioElement(), smooth=True, constantTurn=True)
        with pytest.raises(ValueError, match="turn"):
            tgt.getSmoothTrack(PERIOD, constantTurn=True)
    finally:
        trk.close()
