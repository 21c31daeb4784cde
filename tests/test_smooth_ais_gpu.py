"""GPU: the AIS-aware Rauch-Tung-Striebel smoother (`mht_smooth_tracks_ais`, include/mht_amd.h; pymht_amd.smoothing.smooth_tracks_ais)
against its NumPy restatement tests/smooth_ais_ref.py, and the opt-in drop-in path on top of it (ais=True of Target.getSmoothTrack,
Tracker.getSmoothTracks and Tracker._storeRun).

The criterion is the linear smoother's (tests/test_smooth_gpu.py), factor unchanged: with the np.longdouble evaluation as the truth,
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
means and covariances separately, and  e_dev <= 8 * e_np.  Every test prints the ratios it measured."""
import ctypes as C
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import smooth_ais_ref as sa
import smooth_ref as sr

pytestmark = pytest.mark.gpu

PERIOD = sa.ACCURACY_PERIOD
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


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_accuracy_against_the_longdouble_truth(ctxs, lib_nx):
    """The batch of tests/test_smooth_ais_cpu.py (which asserts what it covers): 40 tracks of 2 .. 400 nodes, 30 % of the nodes with a
    message of either accuracy class, with and without a plot behind it."""
    from pymht_amd.smoothing import smooth_tracks_ais
    _truth_is_better_than_float64()
    pv, tracks = sa.accuracy_batch()
    dev = smooth_tracks_ais(pv, PERIOD, tracks, ctx=ctxs[lib_nx])
    truth, f64 = sa.references(pv, PERIOD, tracks)
    _check("accuracy models/pv with AIS, %d-state build" % lib_nx, dev, truth, f64)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_mixed_batch_shapes_and_properties(ctxs, lib_nx):
    """One call with lengths from 1 to 300, more tracks than a wavefront has lanes and not a multiple of 64; tracks whose every node took
    a message, tracks without any; plus the properties that need no reference."""
    from pymht_amd.models import pv
    from pymht_amd.smoothing import smooth_tracks_ais
    _truth_is_better_than_float64()
    rng = np.random.default_rng(6)
    lengths = [1, 2, 300, 1, 2, 3, 250] + [int(v) for v in rng.integers(1, 90, 123)]
    n = len(lengths)
    assert n == 130 and n > 64 and n % 64 != 0
    p_ais = np.full(n, 0.3)
    every, none = [2, 5, 9, 20, 40, 70, 100], [6, 10, 21, 41, 71, 101]
    p_ais[every], p_ais[none] = 1.0, 0.0
    p_detect = np.full(n, 0.8)
    p_detect[[9, 20]] = 0.0      # (messages only: never a plot)
    tracks = sa.make_batch(pv, PERIOD, lengths, seed=31, p_detect=p_detect, p_ais=p_ais)
    for t in every:
        assert all(a is not None for a in tracks[t][3][1:])
    for t in none:
        assert all(a is None for a in tracks[t][3])
    assert np.isnan(tracks[9][2]).all() and len(tracks[9][2]) > 2
    dev = smooth_tracks_ais(pv, PERIOD, tracks, ctx=ctxs[lib_nx])
    truth, f64 = sa.references(pv, PERIOD, tracks)
    label = "mixed models/pv with AIS, %d-state build" % lib_nx
    _check(label, dev, truth, f64)
    for (x0, P0, z, ais), (xs, Ps) in zip(tracks, dev):
        assert xs.shape == (len(z), 4) and Ps.shape == (len(z), 4, 4) and xs.dtype == np.float64 and Ps.dtype == np.float64
        if len(z) == 1:      # nothing to smooth: output = input, exactly
            assert np.array_equal(xs[0], x0) and np.array_equal(Ps[0], P0)
        assert np.array_equal(Ps, Ps.transpose(0, 2, 1)), "Ps is not symmetric"
    # a track's result does not depend on its place in the batch or on its neighbours: permuting the batch permutes the outputs bit for bit
    perm = rng.permutation(n)
    dev_p = smooth_tracks_ais(pv, PERIOD, [tracks[i] for i in perm], ctx=ctxs[lib_nx])
    for j, i in enumerate(perm):
        assert np.array_equal(dev_p[j][0], dev[i][0]) and np.array_equal(dev_p[j][1], dev[i][1])
    # ... nor on the others being there at all, nor on whether the covariances are asked for
    alone = smooth_tracks_ais(pv, PERIOD, [tracks[2]], ctx=ctxs[lib_nx])[0]
    assert np.array_equal(alone[0], dev[2][0]) and np.array_equal(alone[1], dev[2][1])
    means = smooth_tracks_ais(pv, PERIOD, tracks, ctx=ctxs[lib_nx], covariances=False)
    for (xs, Ps), (xs_m, nothing) in zip(dev, means):
        assert nothing is None and np.array_equal(xs, xs_m)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_without_a_message_the_output_is_the_linear_smoothers_bit_for_bit(ctxs, lib_nx):
    """The plain step is mht_smooth_tracks' step, the same arithmetic in the same order under -ffp-contract=off."""
    from pymht_amd.models import pv
    from pymht_amd.smoothing import smooth_tracks, smooth_tracks_ais
    rng = np.random.default_rng(8)
    lengths = [1, 2, 200] + [int(v) for v in rng.integers(1, 120, 97)]
    tracks = sr.make_batch(pv, PERIOD, lengths, seed=12, p_detect=0.8)
    for cov in (True, False):
        lin = smooth_tracks(pv, PERIOD, tracks, ctx=ctxs[lib_nx], covariances=cov)
        ais = smooth_tracks_ais(pv, PERIOD, [t + ([None] * len(t[2]),) for t in tracks], ctx=ctxs[lib_nx], covariances=cov)
        for (xs, Ps), (xs_a, Ps_a) in zip(lin, ais):
            assert np.array_equal(xs, xs_a) and (np.array_equal(Ps, Ps_a) if cov else Ps is None and Ps_a is None)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_raw_abi_error_codes_leave_the_outputs_untouched(ctxs, lib_nx):
    import torch
    from pymht_amd import _lib
    from pymht_amd.models import pv
    ctx = ctxs[lib_nx]
    lib, dev = ctx.lib, ctx.device
    nx, n, L = 4, 3, 5
    keep = [np.ascontiguousarray(np.asarray(m, dtype=np.float32).ravel()) for m in (pv.Phi(PERIOD), pv.Q(PERIOD), pv.C_RADAR, pv.R_RADAR())]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    model = lambda nx_=4, transition=0: _lib.MhtModelX(nx_, fp(keep[0]), fp(keep[1]), fp(keep[2]), fp(keep[3]), 0.0, 0.0, transition, PERIOD)
    x = torch.zeros((nx, n), dtype=torch.float64, device=dev)
    P = torch.eye(nx, dtype=torch.float64, device=dev).reshape(nx * nx, 1).repeat(1, n).contiguous()
    z = torch.zeros((L, 2, n), dtype=torch.float64, device=dev)
    h = torch.ones((L, n), dtype=torch.uint8, device=dev)
    kind = torch.ones((L, n), dtype=torch.uint8, device=dev)
    kind[2] = 3      # node 2 of every track took a message
    m = torch.zeros((L, 4, n), dtype=torch.float64, device=dev)
    r = torch.ones((L, n), dtype=torch.float64, device=dev)
    leg = torch.zeros((L, n), dtype=torch.int32, device=dev)
    iu = np.triu_indices(4)
    f = lambda a: np.asarray(a, dtype=np.float64)
    legs = torch.from_numpy(np.concatenate([f(pv.Phi(1.0)).ravel(), f(pv.Q(1.0))[iu], f(pv.Phi(1.5)).ravel(), f(pv.Q(1.5))[iu]]).reshape(1, 52)).to(dev)
    xs = torch.full((L, nx, n), -7.0, dtype=torch.float64, device=dev)
    Ps = torch.full((L, 10, n), -7.0, dtype=torch.float64, device=dev)
    need = int(lib.mht_smooth_ais_work_bytes(n, L))
    assert need == 256 + L * 2 * 14 * n * 8
    work = torch.zeros(need, dtype=torch.uint8, device=dev)
    ptr = dict(x=x, P=P, z=z, h=h, kind=kind, m=m, r=r, leg=leg, legs=legs, xs=xs, work=work)

    def call(mdl, lens, work_bytes, L_=L, n_=n, null=None):
        lens = np.asarray(lens, dtype=np.int32)
        p = {k: (None if k == null else v.data_ptr()) for k, v in ptr.items()}
        return lib.mht_smooth_tracks_ais(ctx.handle, C.byref(mdl), n_, L_, None if null == "len" else lens.ctypes.data_as(C.c_void_p), p["x"], p["P"],
                                         p["z"], p["h"], p["kind"], p["m"], p["r"], p["leg"], p["legs"], 1, p["xs"], Ps.data_ptr(), p["work"], work_bytes)

    untouched = lambda: bool((xs == -7.0).all()) and bool((Ps == -7.0).all())
    assert call(model(transition=1), [5, 5, 5], need) == _lib.MHT_E_INVALID and untouched()
    assert b"mht_smooth_tracks_ais" in lib.mht_last_error()
    assert call(model(nx_=6), [5, 5, 5], need) == _lib.MHT_E_INVALID and untouched()
    for name in ("len", "x", "P", "z", "h", "kind", "m", "r", "leg", "legs", "xs", "work"):
        assert call(model(), [5, 5, 5], need, null=name) == _lib.MHT_E_INVALID and untouched(), name
    assert call(model(), [5, 5, 5], need, L_=0) == _lib.MHT_E_INVALID and untouched()
    assert call(model(), [5, 0, 5], need) == _lib.MHT_E_INVALID and untouched()
    assert call(model(), [5, 6, 5], need) == _lib.MHT_E_INVALID and untouched()
    assert call(model(), [5, 5, 5], need - 1) == _lib.MHT_E_CAPACITY and untouched()
    assert b"workspace" in lib.mht_last_error()
    assert call(model(), [], need, n_=0) == _lib.MHT_OK and untouched()      # an empty batch: nothing is launched
    assert call(model(), [5, 2, 1], need) == _lib.MHT_OK
    got, got_P = xs.cpu().numpy(), Ps.cpu().numpy()
    for t, length in enumerate([5, 2, 1]):      # exactly the nodes of each track's length
        assert not (got[:length, :, t] == -7.0).any() and (got[length:, :, t] == -7.0).all()
        assert not (got_P[:length, :, t] == -7.0).any() and (got_P[length:, :, t] == -7.0).all()


# ---- the drop-in path -----------------------------------------------------------------------------------------------------------------
SCENE = dict(seed=96, N=5, T=6, n_scans=30, msg_every=2, equipped=0.67, p_report=0.6)


def _run_scene(seed, N, **scene):
    """An AIS-aided Tracker (device initiator, AIS initialisation) over a scene of tests/ais_long_util.py; half of the ships have no
    track at the start.  Returns the open tracker and the test's OWN record of every scan's messages: scan time -> {mmsi: message}."""
    from ais_long_util import long_window_scenario, msgs_of
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import pv
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, ais = long_window_scenario(seed, N, **scene)
    sc["x0"] = sc["x0"][::2].copy()
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=N, eta2=5.99, radarRange=1.5 * sc["radius"],
                  position=np.asarray(sc["centre"], dtype=np.float64), aisAided=True, maxTargets=32, maxNodes=1 << 18, maxMeasurements=256)
    record = {}
    try:
        for x in sc["x0"]:
            trk.initiateTarget(Target(sc["t0"], None, x.copy(), pv.P0, status="preinitialized"))
        for z, t, msgs in zip(sc["scans"], sc["times"], ais):
            record[float(t)] = {int(m[2]): m for m in msgs}
            trk.addMeasurementList(MeasurementList(float(t), z), msgs_of(msgs), aisInitialization=True)
    except BaseException:
        trk.close()
        raise
    return trk, record, sc["period"]


def _chain_inputs(node, record):
    """(x_init, P_init, measurements, ais) of the chain that ends in `node`, from backtrackNodes(), the nodes' mmsi and `record`."""
    from pymht_amd.models import pv
    chain = node.backtrackNodes()
    ais = [None] * len(chain)
    for k in range(1, len(chain)):
        c = chain[k]
        if c.mmsi is not None:
            tm, state, mmsi, high = record[float(c.time)][int(c.mmsi)]
            ais[k] = (float(tm) - float(chain[k - 1].time), float(c.time) - float(tm), np.asarray(state, dtype=np.float64), bool(high))
    first = chain[0]
    # P_init as the seam defines it: the smoother seams read the UPPER TRIANGLE of P_init (include/mht_amd.h), and the initial covariance
    # of a track the initiator started from AIS messages is a float32 product that is symmetric to rounding only (1e-6 absolute here)
    P = np.asarray(pv.P0 if first.P_0 is None else first.P_0, dtype=np.float64)
    P = np.triu(P) + np.triu(P, 1).T
    return chain, (np.asarray(first.x_0, dtype=np.float64), P, [c.measurement for c in chain], ais)


def test_drop_in_path_smooths_an_ais_aided_run_with_its_messages_and_fills_the_export():
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import pv
    _truth_is_better_than_float64()
    trk, record, period = _run_scene(**SCENE)
    try:
        nodes = list(trk.getTrackNodes()) + list(trk.__terminatedTargets__)
        before = trk.getSmoothTracks(terminated=True)
        got = trk.getSmoothTracks(terminated=True, ais=True)
        after = trk.getSmoothTracks(terminated=True)
        assert len(got) == len(before) == len(nodes) and len(trk.getSmoothTracks(ais=True)) == len(trk.getTrackNodes())
        # the default call is untouched by the flag: the same bits before and after, and they are the radar-only smoother's
        for (p0, v0, ok0), (p1, v1, ok1) in zip(before, after):
            assert ok0 == ok1 and np.array_equal(p0, p1, equal_nan=True) and np.array_equal(v0, v1, equal_nan=True)
        mats = sr.model_matrices(pv, period)
        dev, truth, f64, lin, ends, kinds, with_ais, longest = [], [], [], [], [], [], 0, 0
        for i, (node, (pos, vel, ok)) in enumerate(zip(nodes, got)):
            chain, args = _chain_inputs(node, record)
            assert len(chain) == len(pos) == len(vel)
            if len(chain) < 2:
                assert not ok and np.isnan(vel).all()
                continue
            assert ok
            truth.append(sa.rts_ais(pv, period, *args, dtype=np.longdouble))
            f64.append(sa.rts_ais(pv, period, *args, dtype=np.float64))
            lin.append(sr.rts(*mats, *args[:3], dtype=np.float64))
            dev.append(np.concatenate([pos, vel], axis=1))
            ends.append(node)
            k = sa.kinds(args[2], args[3])
            kinds.append(k)
            with_ais += bool((k >= 2).any())
            if len(chain) > len(nodes[longest].backtrackNodes()):
                longest = i
        allk = np.concatenate(kinds)
        print("drop-in: %d tracks, %d with an AIS node, nodes per kind 0..3: %s" % (len(dev), with_ais, [int((allk == v).sum()) for v in range(4)]))
        # the scene: conditions on the inputs
        assert with_ais >= 3 and (allk == 2).sum() >= 1 and (allk == 3).sum() >= 1
        # accuracy
        e_dev = max(sr.err(d, t["xs"]) for d, t in zip(dev, truth))
        e_np = max(sr.err(f["xs"], t["xs"]) for f, t in zip(f64, truth))
        print("drop-in models/pv with AIS: longest %d nodes: means e_dev %.3g e_np %.3g ratio %.3g" % (max(len(d) for d in dev), e_dev, e_np, e_dev / e_np))
        assert e_dev <= FACTOR * e_np
        # the forward model is the forest's: the last node's smoothed state is its filtered state, which the forest holds as x_0
        late = [j for j, k in enumerate(kinds) if (k[-3:] >= 2).any()]
        assert len(late) >= 1
        for j in late:
            x_0 = np.asarray(ends[j].x_0, dtype=np.float64)
            d_dev, d_ref, d_lin = [float(np.linalg.norm(v - x_0)) for v in (dev[j][-1], f64[j]["xs"][-1], lin[j]["xs"][-1])]
            print("drop-in track %d (%d nodes): last node against the forest's x_0: device %.3g, float64 reference %.3g, radar-only reference %.3g"
                  % (j, len(dev[j]), d_dev, d_ref, d_lin))
            assert d_lin >= 10 * d_ref, "the scene does not exercise the difference (a condition on the inputs)"
            assert d_dev <= 2 * d_ref
        # one node on its own: the same numbers as its row of the batch, bit for bit
        pos1, vel1, ok1 = nodes[longest].getSmoothTrack(trk.radarPeriod, ais=True)
        assert ok1 and np.array_equal(pos1, got[longest][0]) and np.array_equal(vel1, got[longest][1])
        # the export: one <S> per node with smooth=True and ais=True, the AIS-aware numbers at the precision of <States>
        scen = trk.getScenarioElement()
        trk._storeRun(scen, smooth=True)
        trk._storeRun(scen, smooth=True, ais=True)
        plain, smooth = scen.findall("Run")
        assert len(plain.findall("Track")) == len(smooth.findall("Track")) == len(nodes)
        filled = differs = 0
        for (pos, vel, ok), (pos_r, vel_r, _), tr_, tr_r in zip(got, before, smooth.findall("Track"), plain.findall("Track")):
            states, sm = tr_.find("States"), tr_.find("SmoothedStates")
            assert len(states) == int(tr_.attrib["length"]) == len(pos)
            if len(states) < 2:
                assert len(sm) == 0
                continue
            assert len(sm) == len(states) == len(tr_r.find("SmoothedStates"))
            filled += 1
            for s_el, f_el, p, v in zip(sm, states, pos, vel):
                assert s_el.tag == "S" and s_el.attrib["t"] == f_el.attrib["t"]
                assert float(s_el.find("P").find("E").text) == round(float(p[0]), 2) and float(s_el.find("P").find("N").text) == round(float(p[1]), 2)
                assert float(s_el.find("V").find("E").text) == round(float(v[0]), 2) and float(s_el.find("V").find("N").text) == round(float(v[1]), 2)
            for s_el, p, v in zip(tr_r.find("SmoothedStates"), pos_r, vel_r):      # (the run without the flag holds the radar-only numbers)
                assert float(s_el.find("P").find("E").text) == round(float(p[0]), 2) and float(s_el.find("V").find("N").text) == round(float(v[1]), 2)
            differs += ET.tostring(sm) != ET.tostring(tr_r.find("SmoothedStates"))
        assert filled >= 3 and differs >= 3
        ET.fromstring(ET.tostring(scen))      # (well-formed)
        with pytest.raises(ValueError, match="constantTurn"):
            trk.getSmoothTracks(ais=True, constantTurn=True)
        # a message that is not in the history is an error, not a radar-only node
        hist = trk.__aisHistory__
        scan_no = next(c.scanNumber for j in late for c in ends[j].backtrackNodes()[1:] if c.mmsi is not None)
        saved, hist[scan_no - 1] = hist[scan_no - 1], None
        with pytest.raises(RuntimeError, match="AIS history"):
            trk.getSmoothTracks(terminated=True, ais=True)
        hist[scan_no - 1] = saved
    finally:
        trk.close()
    # a radar-only tracker has no AIS history
    trk = Tracker(pv, PERIOD, 1e-7, 1e-4, P_d=0.9, N=3, useInitiator=False)
    try:
        tgt = Target(1000.0, None, np.array([10.0, 20.0, 3.0, -2.0]), pv.P0, status="preinitialized")
        trk.initiateTarget(tgt)
        with pytest.raises(ValueError, match="aisAided"):
            trk.getSmoothTracks(ais=True)
        with pytest.raises(ValueError, match="aisAided"):
            trk._storeRun(trk.getScenarioElement(), smooth=True, ais=True)
    finally:
        trk.close()
