"""GPU: six-state trackers that start their own tracks.  The M-of-N initiator stays the reference's 4-state one (m_of_n.py imports models/pv);
its births enter the six-state forest LIFTED (Tracker(..., useInitiator=True, liftBirths=True); mht_initiator_set_lift):
x = [x4, t], P = [[P4, 0], [0, Pt]], (t, Pt) = zeros and model.P0[4:, 4:] unless birthTail says otherwise.

Every scene starts EMPTY -- every track is born on the device -- and is compared scan by scan with the oracle tracker whose step 7 is the
oracle's M-of-N initiator with the same lift (LiftedInitiator below): decisions exactly, states and covariances to 1e-6 relative."""
import ctypes as C

import numpy as np
import pytest

from test_tracker_gpu import SCORE_ATOL, states_close, tracker_selected

pytestmark = pytest.mark.gpu
M_REQ, N_CHK, V_MAX = 2, 3, 20      # Tracker's defaults (tracker.py:61-72)


class LiftedInitiator:
    """The oracle's 4-state M-of-N initiator behind trace_util's adapter, its births lifted into the six-state space; it keeps what it offered."""

    def __init__(self, model, tail=None):
        from m_of_n_oracle import Initiator
        from trace_util import OracleInitiatorAdapter
        from pymht_amd.models import pv
        from pymht_amd.utils.classDefinitions import MeasurementList
        self.inner = OracleInitiatorAdapter(Initiator(M_REQ, N_CHK, V_MAX, pv.C_RADAR, pv.R_RADAR(), 4 * model.sigmaR_RADAR_tracker ** 2), MeasurementList)
        t, Pt = tail if tail is not None else (np.zeros(2), np.asarray(model.P0)[4:, 4:])
        self.t, self.Pt = np.asarray(t, np.float32), np.asarray(Pt, np.float32)
        self.offered = []      # per scan: list of (x6, P6, meas)

    def processMeasurements(self, time_, z, ais=()):
        out = []
        for x4, P4, meas, zz in self.inner.processMeasurements(time_, z, ais):
            x6 = np.concatenate([np.asarray(x4, np.float32), self.t]).astype(np.float32)
            P6 = np.zeros((6, 6), np.float32)
            P6[:4, :4], P6[4:, 4:] = P4, self.Pt
            out.append((x6, P6, meas, zz))
        self.offered.append([(x, P, 0 if m is None else int(m)) for x, P, m, _ in out])
        return out


def _scene(seed, T=24, n_scans=20, radius=600.0, lam=1e-5, P_d=0.9, period=2.5, n_turn=6):
    """make_scenario's constant-velocity targets and clutter, plus n_turn targets on circles (|w| 0.03-0.08 rad/s) and a pair that moves
    side by side 8 m apart (its two candidates are confirmed in the same scan and merged, m_of_n.py:107-154)."""
    from pymht_amd.utils.scenario import make_scenario
    sc = make_scenario(T=T, radius=radius, lambda_phi=lam, n_scans=n_scans, P_d=P_d, period=period, seed=seed)
    rng = np.random.default_rng(seed + 99)
    p0 = rng.uniform(-0.5 * radius, 0.5 * radius, (n_turn, 2))
    spd, hd = rng.uniform(5.0, 12.0, n_turn), rng.uniform(0.0, 2 * np.pi, n_turn)
    w = rng.choice([-1.0, 1.0], n_turn) * rng.uniform(0.03, 0.08, n_turn)
    pair0, pair_v = rng.uniform(-0.3 * radius, 0.3 * radius, 2), rng.normal(0.0, 5.0, 2)
    scans = []
    for k, z in enumerate(sc["scans"]):
        tk = (k + 1) * period
        h = hd + w * tk
        p = p0 + (spd / w)[:, None] * np.stack([np.sin(h) - np.sin(hd), np.cos(hd) - np.cos(h)], axis=1)
        pr = pair0 + pair_v * tk
        p = np.concatenate([p, [pr, pr + np.array([8.0, 0.0])]])
        seen = rng.uniform(size=len(p)) <= P_d
        zz = np.concatenate([np.asarray(z, np.float64).reshape(-1, 2), p[seen] + rng.normal(0.0, 2.5, (int(seen.sum()), 2))])
        rng.shuffle(zz, axis=0)
        scans.append(np.ascontiguousarray(zz, dtype=np.float32))
    return sc, scans


def _tracker(model, sc, N=3, **kw):
    from pymht_amd.tracker import Tracker
    return Tracker(model, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=N, useInitiator=True, liftBirths=True,
                   maxTargets=256, maxNodes=1 << 18, maxMeasurements=512, **kw)


def _capture(trk):
    """The births block and the target rows of every folded report, by scan number (without changing when the tracker folds)."""
    births, rows = {}, {}
    ab, ar = trk._apply_births, trk._apply_report

    def cap_births(b, scanTime, scanNumber, *a):
        births[scanNumber] = np.array(b)
        return ab(b, scanTime, scanNumber, *a)

    def cap_report(recs, scanTime, scanNumber, *a):
        rows[scanNumber] = np.array(recs)
        return ar(recs, scanTime, scanNumber, *a)
    trk._apply_births, trk._apply_report = cap_births, cap_report
    return births, rows


def _run_against_oracle(model, seed, N=3):
    import mht_oracle as orc
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, scans = _scene(seed)
    trk = _tracker(model, sc, N=N)
    births, _ = _capture(trk)
    init = LiftedInitiator(model)
    o = orc.OracleTracker(sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=N, initiator=init, model=model)
    tail = np.asarray(model.P0, np.float32)[4:, 4:]
    n_born = n_refused = n_merged = 0
    bit_equal = True
    try:
        for k, (z, t) in enumerate(zip(scans, sc["times"])):
            info = o.add_scan(float(t), z)
            trk.addMeasurementList(MeasurementList(float(t), z))
            st = trk.lastScanStats
            s = k + 1
            # step 7: the candidates, their fate, their lifted states and covariances
            offered = init.offered[k]
            b = births.get(s, np.zeros(0, dtype=trk._BIRTH_DTYPE))
            assert len(b) == len(offered), (s, len(b), len(offered))
            assert b["meas"].tolist() == [m for _, _, m in offered], s
            assert b["id"][b["id"] >= 0].tolist() == list(info["new_ids"]), s
            if len(b):
                assert np.all(b["x0"][:, 4:] == 0.0), s
                P = b["P0"].reshape(-1, 6, 6)
                assert np.all(P[:, :4, 4:] == 0.0) and np.all(P[:, 4:, :4] == 0.0), s
                assert np.all(P[:, 4:, 4:] == tail), s
                assert states_close(b["x0"], np.array([x for x, _, _ in offered], np.float64)), s
                assert states_close(P.reshape(-1, 36), np.array([Pc for _, Pc, _ in offered], np.float64).reshape(-1, 36)), s
                bit_equal &= np.array_equal(b["x0"], np.array([x for x, _, _ in offered], np.float64))
            n_born += len(info["new_ids"])
            n_refused += int((b["id"] < 0).sum())
            n_merged += sum(1 for _, _, m in offered if m == 0)
            # steps 1-6 with the newborn tracks in the forest
            assert (st["L"], st["G"]) == (info["L"], info["G"]), s
            assert np.array_equal(st["unused"], info["unused"]), s
            assert [r.ID for r in o.targets] == [r.ID for r in trk.__targetList__], s
            os_, ts = o.selected(), tracker_selected(trk, 6)
            assert np.array_equal(os_["ID"], ts["ID"]) and np.array_equal(os_["meas"], ts["meas"]), s
            assert states_close(os_["x"], ts["x"]) and np.allclose(os_["cnllr"], ts["cnllr"], rtol=0, atol=SCORE_ATOL), s
            assert len(o.clusters) == len(trk.__clusterList__) and all(np.array_equal(a, np.asarray(c)) for a, c in zip(o.clusters, trk.__clusterList__)), s
            assert o.n_ilp == trk.nOptimSolved, s
            lb, tb = o.leaf_batch(), trk.leafBatch()
            assert np.array_equal(lb["ID"], tb["ID"]) and np.array_equal(lb["meas"], tb["meas"]), s
            assert states_close(lb["x"], tb["x"]), s
            assert states_close(lb["P"].reshape(-1, 36), np.asarray(tb["P"], np.float64).reshape(-1, 36)), s
            bit_equal &= np.array_equal(lb["x"], tb["x"]) and np.array_equal(np.asarray(lb["P"], np.float32), np.asarray(tb["P"], np.float32))
    finally:
        trk.close()
    return n_born, n_refused, n_merged, bit_equal


@pytest.mark.parametrize("seed", [3, 11])
def test_constant_turn_tracker_starts_its_own_tracks_like_the_oracle(seed):
    from pymht_amd.models import ct
    n_born, n_refused, n_merged, bit_equal = _run_against_oracle(ct, seed)
    print("CT seed %d: %d births, %d refused by the neighbour test, %d merged, bit-equal %s" % (seed, n_born, n_refused, n_merged, bit_equal))
    assert n_born >= 10
    assert n_refused + n_merged >= 1


def test_constant_acceleration_tracker_starts_its_own_tracks_like_the_oracle():
    from pymht_amd.models import ca
    n_born, n_refused, n_merged, bit_equal = _run_against_oracle(ca, 5)
    print("CA: %d births, %d refused by the neighbour test, %d merged, bit-equal %s" % (n_born, n_refused, n_merged, bit_equal))
    assert n_born >= 10
    assert n_refused + n_merged >= 1


def _step_stepwise(trk, sl):
    """The _after_step route: mht_forest_step_host, then mht_forest_initiate on the scan it staged."""
    from pymht_amd import _lib
    z = trk._accept_scan(sl, None, {})
    trk._staged, trk._staged_np = None, z
    _lib.check(trk._lib.mht_forest_step_host(trk._ctx.handle, z.__array_interface__['data'][0], z.shape[0]))
    trk._leaf_time = float(sl.time)
    trk._after_step(sl, z, None)


def test_streamed_and_stepwise_routes_give_identical_reports():
    from pymht_amd.models import ct
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, scans = _scene(29)
    a, b = _tracker(ct, sc), _tracker(ct, sc)
    ba, ra = _capture(a)
    bb, rb = _capture(b)
    try:
        for z, t in zip(scans, sc["times"]):      # (the streamed tracker is not looked at in between: the route as a real-time host drives it)
            a.addMeasurementList(MeasurementList(float(t), z))
            _step_stepwise(b, MeasurementList(float(t), z))
            b._drain()      # (the stepwise route's report has left the device behind mht_forest_report_begin: it is folded scan by scan)
        la, lb = a.leafBatch(), b.leafBatch()
        assert sorted(ba) == sorted(bb) and sum(int((x["id"] >= 0).sum()) for x in ba.values()) >= 10
        for s in ba:
            assert np.array_equal(ba[s], bb[s]), "scan %d births" % s
        assert sorted(ra) == sorted(rb) == list(range(1, len(scans) + 1))
        for s in ra:
            assert np.array_equal(ra[s], rb[s]), "scan %d report rows" % s
        for key in la:
            assert np.array_equal(la[key], lb[key]), key
    finally:
        a.close()
        b.close()


def test_raw_abi_lift():
    """mht_forest_initiate refuses an initiator without a lift in the six-state library; with mht_initiator_set_lift the report's birth rows
    carry x0 = [x4, tail], P0 = [[P4, 0], [0, P_tail]] with x4 / P4 what mht_initiator_born hands out.  The 4-state library refuses the call."""
    from pymht_amd import _lib
    from pymht_amd.device import Context
    from pymht_amd.initiators import m_of_n
    from pymht_amd.models import ct, pv
    from pymht_amd.tracker import Tracker, _report_dtypes
    trk = Tracker(ct, 2.5, 1e-6, 1e-4, N=3, useInitiator=False, maxTargets=64, maxNodes=1 << 16, maxMeasurements=64)
    lib, h = trk._lib, trk._ctx.handle
    init = m_of_n.Initiator(2, 3, 20, pv.C_RADAR, pv.R_RADAR(), 25.0, ctx=trk._ctx, maxMeasurements=64)
    born_dt = _report_dtypes(6)[1]
    p0 = np.array([[x, y] for y in (-150.0, 150.0) for x in (-180.0, 0.0, 180.0)], np.float32)
    v = np.array([4.0, -3.0], np.float32)
    tail_x, tail_P = np.array([0.01, -0.002], np.float32), np.array([[2e-4, 1e-7], [1e-7, 3e-6]], np.float32)
    seen = 0
    try:
        z = np.ascontiguousarray(p0)
        _lib.check(lib.mht_forest_step_host(h, z.ctypes.data_as(C.c_void_p), len(z)))
        assert lib.mht_forest_initiate(h, init.handle, None, len(z), 2.5) == _lib.MHT_E_INVALID
        assert b"mht_initiator_set_lift" in lib.mht_last_error()
        init.set_lift(6, tail_x, tail_P)
        for k in range(1, 6):
            z = np.ascontiguousarray(p0 + v * np.float32(2.5 * k))
            _lib.check(lib.mht_forest_step_host(h, z.ctypes.data_as(C.c_void_p), len(z)))
            _lib.check(lib.mht_forest_initiate(h, init.handle, None, len(z), 2.5 * (k + 1)))
            _lib.check(lib.mht_forest_report_begin(h))
            rep = _lib.MhtScanReport()
            _lib.check(lib.mht_forest_report(h, C.byref(rep)))
            if not rep.n_births:
                continue
            b = np.frombuffer(C.string_at(rep.births, rep.n_births * born_dt.itemsize), dtype=born_dt)
            x4, P4, m = np.zeros((256, 4)), np.zeros((256, 16), np.float32), np.zeros(256, np.int32)
            nb = C.c_int32(0)
            _lib.check(lib.mht_initiator_born(init.handle, 256, x4.ctypes.data_as(C.c_void_p), P4.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p),
                                              C.byref(nb), None, None))
            assert nb.value == len(b)
            P = b["P0"].reshape(-1, 6, 6)
            assert np.array_equal(b["x0"][:, :4], x4[:len(b)]) and np.array_equal(P[:, :4, :4], P4[:len(b)].reshape(-1, 4, 4))
            assert np.all(b["x0"][:, 4:] == tail_x.astype(np.float64)) and np.all(P[:, 4:, 4:] == tail_P)
            assert np.all(P[:, :4, 4:] == 0) and np.all(P[:, 4:, :4] == 0)
            assert np.array_equal(b["meas"], m[:len(b)])
            seen += int((b["id"] >= 0).sum())
        assert seen == len(p0)
        x = np.zeros((64, 6))
        n = C.c_int32(0)
        _lib.check(lib.mht_forest_leaves(h, 64, x.ctypes.data_as(C.c_void_p), None, None, None, None, None, None, None, C.byref(n)))
        assert n.value >= len(p0)
    finally:
        init.close()
        trk.close()
    ctx4 = Context(0)
    init4 = m_of_n.Initiator(2, 3, 20, pv.C_RADAR, pv.R_RADAR(), 25.0, ctx=ctx4, maxMeasurements=64)
    try:
        with pytest.raises(_lib.MhtError) as ei:
            init4.set_lift(6, tail_x, tail_P)
        assert ei.value.code == _lib.MHT_E_INVALID
    finally:
        init4.close()
        ctx4.close()


def test_six_state_initiator_without_lift_keeps_refusing():
    from pymht_amd.models import ct
    from pymht_amd.tracker import Tracker
    with pytest.raises(NotImplementedError, match="liftBirths"):
        Tracker(ct, 2.5, 1e-6, 1e-4, useInitiator=True)


def test_birth_tail_override():
    from pymht_amd.models import ct
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, scans = _scene(41, n_scans=6)
    tail = (np.array([0.02, 0.0]), np.diag([5e-4, 2e-6]))
    trk = _tracker(ct, sc, birthTail=tail)
    births, _ = _capture(trk)
    try:
        for z, t in zip(scans, sc["times"]):
            trk.addMeasurementList(MeasurementList(float(t), z))
        trk.getTrackNodes()
        b = np.concatenate(list(births.values()))
        assert len(b) >= 5
        assert np.all(b["x0"][:, 4:] == np.float32(tail[0]).astype(np.float64))
        assert np.all(b["P0"].reshape(-1, 6, 6)[:, 4:, 4:] == np.float32(tail[1]))
    finally:
        trk.close()


def test_more_births_than_the_initiator_holds_is_a_capacity_error(monkeypatch):
    """The six-state counterpart of test_forest_edge_gpu.py's: more confirmed candidates in one scan than max_born -> MHT_E_CAPACITY."""
    from pymht_amd import _lib
    from pymht_amd.initiators import m_of_n
    from pymht_amd.models import ct
    from pymht_amd.utils.classDefinitions import MeasurementList
    monkeypatch.setattr(m_of_n, "MAX_BORN", 3)
    sc, _ = _scene(5, T=2, n_scans=10, radius=300.0, lam=1e-6, n_turn=1)
    trk = _tracker(ct, sc)
    p0 = np.array([[x, y] for y in (-150.0, 150.0) for x in (-180.0, -60.0, 60.0, 180.0)], np.float32)
    v = np.array([4.0, 1.0], np.float32)
    with pytest.raises(_lib.MhtError) as ei:
        for z, t in zip(sc["scans"], sc["times"]):      # eight steady strangers: confirmed in the third scan
            zz = np.concatenate([np.asarray(z, np.float32).reshape(-1, 2), p0 + v * np.float32(t - sc["times"][0])]).astype(np.float32)
            trk.addMeasurementList(MeasurementList(float(t), zz))
        trk.getTrackNodes()
    assert ei.value.code in (_lib.MHT_E_CAPACITY, _lib.MHT_E_STATE)
    trk.close()


def _same(a, b, what):
    assert [r.ID for r in a.__targetList__] == [r.ID for r in b.__targetList__], what
    sa, sb = tracker_selected(a, 6), tracker_selected(b, 6)
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), (what, key)
    la, lb = a.leafBatch(), b.leafBatch()
    for key in la:
        if key != "node":
            assert np.array_equal(la[key], lb[key]), (what, key)


def test_cluster_sharded_lifted_tracker_equals_single_tracker():
    import torch
    from pymht_amd.models import ct
    from pymht_amd.parallel import ClusterShardedTracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, scans = _scene(11)
    solo = _tracker(ct, sc)
    parts = [ClusterShardedTracker(_tracker(ct, sc), 2, i, exchange=lambda t: None) for i in range(2)]
    try:
        for k, (z, t) in enumerate(zip(scans, sc["times"])):
            sl = MeasurementList(float(t), z)
            solo.addMeasurementList(sl)
            for p in parts:
                p.begin(sl)
            merged = torch.stack([p.sel_rel for p in parts]).max(dim=0).values
            for p in parts:
                p.sel_rel.copy_(merged)
                p.end()
            for i, p in enumerate(parts):
                _same(p.trk, solo, "scan %d shard %d" % (k + 1, i))
        assert solo.nTargets >= 10
    finally:
        for p in parts:
            p.trk.close()
        solo.close()


def test_sector_group_with_a_lifted_constant_turn_member_equals_solo_trackers():
    from pymht_amd.models import ct
    from pymht_amd.sectors import SectorGroup
    from pymht_amd.utils.classDefinitions import MeasurementList
    from test_tracker_gpu import make_tracker
    sc, scans = _scene(23)
    sc4, scans4 = _scene(24)
    solo6, solo4 = _tracker(ct, sc), make_tracker(sc4["period"], sc4["lambda_phi"], 1e-4, sc4["P_d"], 3, 5.99, sc4["x0"][:0], sc4["t0"])[0]
    mem6, mem4 = _tracker(ct, sc), make_tracker(sc4["period"], sc4["lambda_phi"], 1e-4, sc4["P_d"], 3, 5.99, sc4["x0"][:0], sc4["t0"])[0]
    g = SectorGroup([mem4, mem6])
    try:
        for k, (z, t, z4, t4) in enumerate(zip(scans, sc["times"], scans4, sc4["times"])):
            solo6.addMeasurementList(MeasurementList(float(t), z))
            solo4.addMeasurementList(MeasurementList(float(t4), z4))
            g.addMeasurementLists([MeasurementList(float(t4), z4), MeasurementList(float(t), z)])
            _same(mem6, solo6, "scan %d six-state member" % (k + 1))
            assert [r.ID for r in mem4.__targetList__] == [r.ID for r in solo4.__targetList__]
        assert solo6.nTargets >= 10
    finally:
        g.close()
        for t_ in (solo6, solo4, mem6, mem4):
            t_.close()
