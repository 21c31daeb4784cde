"""Live-oracle helpers for AIS-aided forests with long N-scan windows (N = 8..12: 32-int path / ancestor records, two halves of 16
levels).  Small scenes -- a handful of ships, low clutter, high P_d -- run long enough for the window to fill and the roots to advance
several times; every scan is compared the way fuzz_util.run_case_ais compares its cases.  An N-scan window of 12 keeps up to 2^12 leaves
per target, and every AIS message multiplies the leaves of its ship: the scenes have three ships, about two of them equipped, messages on every
third scan and similar-state pruning on two scans of three, which keeps the live oracle at a few seconds per trace."""
import ctypes as C
import time

import numpy as np

AIS_SCORE_ATOL = 2e-5


def long_window_scenario(seed, N, T=3, n_scans=None, lambda_phi=1e-6, P_d=0.9, radius=600.0, period=2.5, equipped=0.67, p_report=0.6, msg_every=3):
    """A scene for an N-scan window of N: N + 6 scans unless given; AIS traffic from make_ais on the scans k with k % msg_every == 1."""
    from pymht_amd.utils.scenario import make_scenario, make_ais
    sc = make_scenario(T=T, radius=radius, lambda_phi=lambda_phi, n_scans=(N + 6) if n_scans is None else n_scans, P_d=P_d, period=period, seed=seed)
    ais = make_ais(sc, seed=seed + 5, equipped=equipped, p_report=p_report)
    ais = [a if k % msg_every == 1 else [] for k, a in enumerate(ais)]
    return sc, ais


def prune_on(k):
    """Similar-state pruning on two scans of three."""
    return k % 3 != 0


def make_pair(sc, N, ais_init, eta2=5.99, max_nodes=1 << 18, max_meas=256, max_targets=32):
    """(tracker, oracle) on the same preinitialised targets (the M-of-N initiator on both sides).  Few target slots and a large layer: one
    target's children can run into thousands, more than its static block and one region of the node index space of a smaller pool take."""
    from trace_util import make_oracle_ais
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import pv
    rr = 1.5 * sc["radius"]
    pos = np.asarray(sc["centre"], dtype=np.float64)
    g = dict(period=sc["period"], lambda_phi=sc["lambda_phi"], lambda_nu=1e-4, P_d=sc["P_d"], N=N, eta2=eta2, eta2_ais=9.45, x0=sc["x0"], t0=sc["t0"],
             radar_range=rr, position=pos, with_initiator=True, accepted=None)
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=N, eta2=eta2, radarRange=rr, position=pos, aisAided=True,
                  maxTargets=max_targets, maxNodes=max_nodes, maxMeasurements=max_meas)
    acc = []
    for x in sc["x0"]:
        n0 = trk.nTargets
        trk.initiateTarget(Target(sc["t0"], None, x.copy(), pv.P0, status="preinitialized"))
        acc.append(trk.nTargets > n0)
    g["accepted"] = acc
    return trk, make_oracle_ais(g)


def msgs_of(ais_k):
    from pymht_amd.ais import AisMessage, AisMessageList
    return AisMessageList([AisMessage(*m) for m in ais_k])


def oracle_msgs_of(ais_k):
    import mht_oracle as orc
    return [orc.AisMessage(m[0], m[1].copy(), m[2], m[3]) for m in ais_k]


def _same():
    from util import live_numpy_f64_is_pinned
    # (float64 LAPACK order of THIS host's numpy = the one csrc/mht_la64.h restates; elsewhere 1e-12 relative, as fuzz_util does)
    if live_numpy_f64_is_pinned():
        return np.array_equal
    return lambda a, b: np.shape(a) == np.shape(b) and np.allclose(a, b, rtol=1e-12, atol=1e-12)


def compare_scan(trk, o, info, what):
    """Everything fuzz_util.run_case_ais compares after a scan: decisions exact, leaf states / covariances in the reference's dtypes,
    cumulative scores to AIS_SCORE_ATOL.  Raises AssertionError naming the first field that differs."""
    from trace_util import oracle_rows
    same = _same()
    st = trk.lastScanStats
    nodes = list(trk.getTrackNodes())
    tb = trk.leafBatch()
    lb = oracle_rows([l for r in o.targets for l in r.leaves()])
    os_ = oracle_rows(o.track_nodes)
    t_mmsi = np.array([0 if n.mmsi is None else n.mmsi for n in nodes], dtype=np.int64)
    t_meas = np.array([(-1 if n.mmsi is not None else 0) if n.measurementNumber is None else n.measurementNumber for n in nodes], dtype=np.int64)
    o_meas = np.where((os_["meas"] == -1) & (os_["mmsi"] == 0), 0, os_["meas"])
    t_x = np.array([np.asarray(n.x_0, dtype=np.float64) for n in nodes]).reshape(-1, 4)
    assert st["L"] == info["L"], (what, "L", st["L"], info["L"])
    assert np.array_equal(st["unused"], info["unused"]), (what, "unused")
    assert [r.ID for r in o.targets] == [r.ID for r in trk.__targetList__], (what, "target IDs")
    assert np.array_equal(os_["ID"], [n.ID for n in nodes]), (what, "selected IDs")
    assert np.array_equal(o_meas, t_meas), (what, "selected measurements")
    assert np.array_equal(os_["mmsi"], t_mmsi), (what, "selected identities")
    assert same(os_["x"], t_x), (what, "selected states")
    assert np.allclose(os_["cnllr"], [float(n.cumulativeNLLR) for n in nodes], rtol=0, atol=AIS_SCORE_ATOL), (what, "selected scores")
    assert len(o.clusters) == len(trk.__clusterList__) and all(np.array_equal(a, np.asarray(b)) for a, b in zip(o.clusters, trk.__clusterList__)), (what, "clusters")
    assert np.array_equal(lb["ID"], tb["ID"]), (what, "leaf IDs")
    assert np.array_equal(lb["meas"], tb["meas"]), (what, "leaf measurements")
    assert np.array_equal(lb["mmsi"], tb["mmsi"]), (what, "leaf identities")
    assert same(lb["x"], tb["x"]), (what, "leaf states")
    assert np.array_equal(lb["Pf64"], tb["Pf64"]) and same(lb["P"], tb["P"]), (what, "leaf covariances")
    assert np.allclose(lb["cnllr"], tb["cnllr"], rtol=0, atol=AIS_SCORE_ATOL), (what, "leaf scores")
    assert o.n_ilp == trk.nOptimSolved, (what, "ILPs", o.n_ilp, trk.nOptimSolved)


def record_depth(trk):
    """(most non-negative entries in one leaf's path record, deepest radar-half level with an entry) over the newest layer's leaves."""
    from pymht_amd import _lib
    cap = int(trk._cfg.max_nodes)
    buf = np.full(32 * cap, -1, dtype=np.int32)
    _lib.check(trk._lib.mht_forest_debug_read(trk._ctx.handle, b"path", buf.ctypes.data_as(C.c_void_p), buf.nbytes))
    nodes = np.asarray(trk.leafBatch()["node"], dtype=np.int64)
    if len(nodes) == 0:
        return 0, -1
    rec = buf.reshape(cap, 32)[nodes]
    most = int((rec >= 0).sum(axis=1).max())
    radar = np.where((rec[:, :16] >= 0).any(axis=0))[0]
    return most, int(radar.max()) if len(radar) else -1


def run_trace(seed, N, ais_init, max_leaves=30000, budget_s=None, **scene):
    """Scan by scan against the live oracle.  Returns (scans run, deepest record seen as record_depth gives it, messages fused, why it
    stopped early: None, "leaf cap" or "time budget").  budget_s (wall-clock seconds, none by default) is for the fuzz campaign only."""
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, ais = long_window_scenario(seed, N, **scene)
    if ais_init:
        sc["x0"] = sc["x0"][::2].copy()      # (half of the ships have no track at the start: messages start theirs)
    trk, o = make_pair(sc, N, ais_init)
    t0 = time.time()
    deepest, n_fused, k, stop = (0, -1), 0, 0, None
    try:
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            on, msgs = prune_on(k), ais[k]
            info = o.add_scan(float(t), z, prune_similar=on, ais=oracle_msgs_of(msgs), ais_initialization=ais_init)
            trk.addMeasurementList(MeasurementList(float(t), z), msgs_of(msgs), aisInitialization=ais_init, pruneSimilar=on)
            compare_scan(trk, o, info, "seed %d N %d scan %d" % (seed, N, k))
            n_fused += info["n_fused"]
            d = record_depth(trk)
            deepest = (max(deepest[0], d[0]), max(deepest[1], d[1]))
            if info["L"] > max_leaves:
                stop = "leaf cap"
            elif budget_s is not None and time.time() - t0 > budget_s:
                stop = "time budget"
            if stop and k + 1 < len(sc["scans"]):
                break
            stop = None
        return k + 1, deepest, n_fused, stop
    finally:
        trk.close()
