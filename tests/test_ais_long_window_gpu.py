"""AIS-aided tracking with N-scan windows of 8 to 12 (Tracker(..., aisAided=True, N=n); tracker.py:112-114 takes any N): path / ancestor
records of 32 ints -- two halves of 16 levels, radar rows and AIS-message rows -- and the fgrow_ais_kernel<8> instance that writes them.
Live-oracle traces scan by scan (tests/ais_long_util.py), the streamed path, groups, cluster shards and value-table turnover."""
import numpy as np
import pytest

from ais_long_util import (compare_scan, long_window_scenario, make_pair, msgs_of, oracle_msgs_of, prune_on, record_depth, run_trace)

pytestmark = pytest.mark.gpu


def _tracker(N, aisAided, **kw):
    from pymht_amd.tracker import Tracker
    from pymht_amd.models import pv
    return Tracker(pv, 2.5, 1e-6, 1e-4, P_d=0.9, N=N, eta2=5.99, radarRange=900.0, position=np.zeros(2), aisAided=aisAided,
                   maxTargets=64, maxNodes=1 << 12, maxMeasurements=64, **kw)


@pytest.mark.parametrize("N", [8, 10, 12])
def test_ais_forest_takes_long_windows(N):
    trk = _tracker(N, True)
    try:
        assert trk._cfg.n_scan == N
    finally:
        trk.close()


def test_ais_window_above_12_fails_like_radar():
    """N = 13 needs a ring of 17 layers: refused by mht_forest_create for every forest, with and without AIS."""
    from pymht_amd import _lib
    with pytest.raises(_lib.MhtError) as radar:
        _tracker(13, False)
    with pytest.raises(_lib.MhtError) as ais:
        _tracker(13, True)
    assert str(ais.value) == str(radar.value) and ais.value.code == radar.value.code


# scenes whose equipped ships report while they have tracks: fused children on both sides of the comparison
TRACE_SEEDS = {(8, False): 4180, (8, True): 4188, (10, False): 4200, (10, True): 4205, (12, False): 4221, (12, True): 4225}


@pytest.mark.parametrize("ais_init", [False, True])
@pytest.mark.parametrize("N", [8, 10, 12])
def test_long_window_trace_equals_live_oracle(N, ais_init):
    """N + 6 scans: the window fills and the roots advance six times.  Every scan exact against the oracle; the leaves' records must
    really be the long ones (an entry beyond the 16 a record of the N <= 7 layout holds, or a radar row at level >= 8)."""
    seed = TRACE_SEEDS[N, ais_init]
    n, (most, radar_lvl), n_fused, stop = run_trace(seed, N, ais_init)
    assert n >= N + 6, "trace stopped after %d scans (%s)" % (n, stop)
    assert n_fused > 0
    assert most > 16 or radar_lvl >= 8, (most, radar_lvl)


def test_streamed_long_window_equals_live_oracle():
    """N = 10, nothing looked at between the calls: reports are folded by later calls, a scan with messages waits for the fold of the
    one before (tracker.py: _arm_ais); scans with and without messages.  The end state must be the oracle's."""
    from pymht_amd.utils.classDefinitions import MeasurementList
    N, ais_init = 10, True
    sc, ais = long_window_scenario(4300, N)
    trk, o = make_pair(sc, N, ais_init)
    try:
        assert any(len(a) for a in ais) and any(len(a) == 0 for a in ais)
        infos = [o.add_scan(float(t), z, prune_similar=prune_on(k), ais=oracle_msgs_of(ais[k]), ais_initialization=ais_init)
                 for k, (z, t) in enumerate(zip(sc["scans"], sc["times"]))]
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            trk.addMeasurementList(MeasurementList(float(t), z), msgs_of(ais[k]), aisInitialization=ais_init, pruneSimilar=prune_on(k))
        compare_scan(trk, o, infos[-1], "streamed end state")
        most, radar_lvl = record_depth(trk)
        assert most > 16 or radar_lvl >= 8, (most, radar_lvl)
    finally:
        trk.close()


def _same_state(a, b, what):
    sa, sb = a._sel[0], b._sel[0]
    for name in ("id", "status", "sel_meas", "sel_x", "sel_cnllr", "score", "root_scan", "root_meas", "root_x", "n_leaves", "cluster"):
        assert np.array_equal(sa[name], sb[name]), (what, name)
    assert a.nTargets == b.nTargets, what
    la, lb = a.leafBatch(), b.leafBatch()
    for key in ("ID", "meas", "x", "cnllr", "P") + (("mmsi", "Pf64") if "mmsi" in la else ()):
        assert np.array_equal(la[key], lb[key]), (what, key)


def test_group_with_a_long_window_ais_member():
    """A SectorGroup of two radar-only sectors (N = 5, batched launches) and one AIS-aided sector with N = 10 (launches of its own):
    every member must equal a lone Tracker fed the same scans."""
    from pymht_amd.sectors import SectorGroup
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import pv
    from pymht_amd.utils.classDefinitions import MeasurementList
    from pymht_amd.utils.scenario import make_scenario
    N = 10
    sc_a, ais = long_window_scenario(4400, N)
    radar = [make_scenario(T=30, radius=1500.0, lambda_phi=5e-6, n_scans=N + 6, P_d=0.9, seed=4410 + q, centre=(0.0, 20000.0 * (q + 1)))
             for q in range(2)]

    def radar_trk(sc):
        t = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=5, eta2=5.99, maxTargets=256, maxNodes=1 << 16,
                    maxMeasurements=256, deviceTiming=False)
        t._add_targets([Target(sc["t0"], None, x.copy(), pv.P0, status="preinitialized") for x in sc["x0"]])
        return t
    solo = [radar_trk(sc) for sc in radar] + [make_pair(sc_a, N, False)[0]]
    grouped = [radar_trk(sc) for sc in radar] + [make_pair(sc_a, N, False)[0]]
    grp = SectorGroup([grouped[0], grouped[2], grouped[1]])
    try:
        for k in range(N + 6):
            lists = [MeasurementList(float(sc["times"][k]), sc["scans"][k]) for sc in radar + [sc_a]]
            for q in range(2):
                solo[q].addMeasurementList(lists[q])
            solo[2].addMeasurementList(lists[2], msgs_of(ais[k]), aisInitialization=False, pruneSimilar=prune_on(k))
            grp.addMeasurementLists([lists[0], lists[2], lists[1]], aisLists=[None, msgs_of(ais[k]), None],
                                    pruneSimilar=[False, prune_on(k), False], aisInitialization=False)
            for q in range(3):
                _same_state(grouped[q], solo[q], "scan %d sector %d" % (k, q))
    finally:
        grp.close()
        for t in solo + grouped:
            t.close()


def test_cluster_sharded_long_window_ais_equals_single_forest():
    """Two cluster shards on one GPU, AIS-aided with N = 9: every shard equals the single forest scan by scan, and both shards solve
    some of the ILPs."""
    import torch
    from pymht_amd.parallel import ClusterShardedTracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    N, ais_init = 9, True
    sc, ais = long_window_scenario(4500, N, T=6, radius=300.0)
    single = make_pair(sc, N, ais_init)[0]
    parts = [ClusterShardedTracker(make_pair(sc, N, ais_init)[0], 2, i, exchange=lambda t: None) for i in range(2)]
    solved = [0, 0]
    try:
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            kw = dict(aisInitialization=ais_init, pruneSimilar=prune_on(k))
            single.addMeasurementList(MeasurementList(float(t), z), msgs_of(ais[k]), **kw)
            for q in parts:
                q.begin(MeasurementList(float(t), z), msgs_of(ais[k]), **kw)
            both = torch.stack([(q.sel_rel >= 0).int() for q in parts])
            assert int(both.sum(dim=0).max()) <= 1
            for i in range(2):
                solved[i] += int(both[i].sum())
            merged = torch.stack([q.sel_rel for q in parts]).max(dim=0).values
            for q in parts:
                q.sel_rel.copy_(merged)
                q.end()
            ref_nodes = list(single.getTrackNodes())
            for q in parts:
                trk = q.trk
                assert [r.ID for r in trk.__targetList__] == [r.ID for r in single.__targetList__], k
                nodes = list(trk.getTrackNodes())
                assert [n.ID for n in nodes] == [n.ID for n in ref_nodes], k
                assert [n.mmsi for n in nodes] == [n.mmsi for n in ref_nodes], k
                assert [n.measurementNumber for n in nodes] == [n.measurementNumber for n in ref_nodes], k
                la, lb = single.leafBatch(), trk.leafBatch()
                for key in ("ID", "meas", "mmsi", "x", "Pf64", "P", "cnllr"):
                    assert np.array_equal(la[key], lb[key]), (k, key)
        assert min(solved) > 0, solved
    finally:
        single.close()
        for q in parts:
            q.trk.close()


def test_long_window_trace_across_value_table_generations(monkeypatch):
    """N = 12 with a small covariance-value table (MHT_VTAB_CAP): the host sees it filling and re-keys the live leaves into the other
    generation, which has to last R + 2 = 18 scans.  The trace must stay exact against the oracle across the switches."""
    import ctypes as C
    from pymht_amd import _lib
    from pymht_amd.utils.classDefinitions import MeasurementList
    N, ais_init = 12, False
    sc, ais = long_window_scenario(4600, N, n_scans=40)
    monkeypatch.setenv("MHT_VTAB_CAP", str(VTAB_CAP_N12))
    trk, o = make_pair(sc, N, ais_init)
    monkeypatch.delenv("MHT_VTAB_CAP")
    try:
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            info = o.add_scan(float(t), z, prune_similar=prune_on(k), ais=oracle_msgs_of(ais[k]), ais_initialization=ais_init)
            trk.addMeasurementList(MeasurementList(float(t), z), msgs_of(ais[k]), aisInitialization=ais_init, pruneSimilar=prune_on(k))
            compare_scan(trk, o, info, "scan %d" % k)
        r = np.zeros(1, np.int32)
        _lib.check(trk._lib.mht_forest_debug_read(trk._ctx.handle, b"vt_rebuilds", r.ctypes.data_as(C.c_void_p), 4))
        assert r[0] >= 1, "the table was meant to fill: %d generation switches" % int(r[0])
    finally:
        trk.close()


VTAB_CAP_N12 = 1 << 20      # (the scene hands out 45-95 k ids per scan once the window is full: two switches in 40 scans, 18 apart)
