"""GPU: the OVERLAPPING scan path -- the one the headline figure is measured on -- held to the looked-at path at EVERY scan.

Nobody looks between the scans on that path (the raw `mht_forest_step` replay, the streamed `Tracker.addMeasurementList`): the scan's commit
rides in the next grow launch, and that launch runs any-order next to the previous scan's ILP launch (`FDyn::ovl`, `step_grow` in
pymht_amd/csrc/mht_forest.hip).  Every trace test, fuzz slice and live-oracle test reads the tracker after each scan, which flushes the deferred
commit; test_overlap_golden_gpu.py and the deferred-commit tests compare the LAST scan or per-scan counts.  A wrong scan in the middle of a
stream that the N-scan window prunes away a few scans later left no trace.  Here (tests/overlap_util.py):
  1. the streamed drop-in path against the reference's recorded traces at every scan (the reports the tracker folds two scans late are kept);
  2. 240 streamed scans against the looked-at path at every scan -- headline size, fresh / stale host hints, value-table generation switches
     and pruning toggles in the middle of overlapped chains;
  3. the raw replay `bench.py` times, read at stop points (start of a chain, the ring's wrap, the `s_table - k < 60` bound of `targets_ub`,
     the rings of 64 of `births_after` / `bhint`), a fresh forest per stop;
  4. a group of uneven sectors at stop points.
The host-timing-dependent inputs of the path (the grow grid from `targets_ub`, the ILP grid from `blp_hint_grid`, the scan at which
`vt_switch_generation` fires) must not change any result: the cadences of 2 and 3 move them.  `uf_ovl` proves that launches really overlapped.
Each test prints one `overlap-parity` line with its counters (profiles/overlap_parity.txt)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import overlap_util as ou
from trace_util import sha

pytestmark = pytest.mark.gpu
SCORE_ATOL = 2e-5
N_LONG = 240          # scans of the long streamed runs
N_RAW = 200           # the raw replay's last stop


def _note(case, **kw):
    print("overlap-parity %-44s %s" % (case, " ".join("%s=%s" % (k, ("%.2f" % v) if isinstance(v, float) else v) for k, v in kw.items())))


def _lists(sc, n=None):
    from pymht_amd.utils.classDefinitions import MeasurementList
    return [MeasurementList(float(t), z) for z, t in zip(sc["scans"][:n], sc["times"][:n])]


def _tracker(sc, **kw):
    """A tracker for a scenario of pymht_amd.utils.scenario with its initial targets admitted in one batch, sized like bench.py's for the
    headline config (500 targets) and like the sector tests' for the small ones."""
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import pv
    big = len(sc["x0"]) > 250
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=sc["N"], eta2=5.99, maxTargets=2048 if big else 1024,
                  maxNodes=1 << (19 if big else 18), maxMeasurements=1024, **kw)
    trk._add_targets([Target(sc["t0"], None, x.copy(), pv.P0, status="preinitialized") for x in sc["x0"]])
    return trk


def _small_table(**kw):
    """A tracker made under MHT_VTAB_CAP=2048 (read when the forest is made): the covariance-value table switches generation every few scans."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MHT_VTAB_CAP", "2048")
        return _tracker(**kw)


# ---- 1. the streamed drop-in path against the reference's recorded traces, at every scan ---------------------------------------------------
@pytest.mark.parametrize("name", ["g6b_trace_cfg3_long", "g6_trace_cfg3", "g3b_trace_cfg2", "g2_trace_cfg1", "g3_trace_dense"])
def test_streamed_api_every_scan_equals_reference(name, gold_dir):
    """All scans of a trace recorded from the reference (pymht/tracker.py:162-307) streamed through `Tracker.addMeasurementList` without a look:
    deferred commits, admissions riding in the next grow launch, any-order grow launches next to the previous scan's ILP launch.  The report rows
    and births the tracker folds two scans late are kept as they pass, and only after the last scan compared with the fixture -- for EVERY
    scan: L/G/M, unused measurements, the target list, selections and states (bit for bit), scores, terminations, births, cluster lists."""
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import pv
    from pymht_amd.utils.classDefinitions import MeasurementList
    t0 = time.perf_counter()
    g = np.load(os.path.join(gold_dir, name + ".npz"))
    trk = Tracker(pv, float(g["period"]), float(g["lambda_phi"]), float(g["lambda_nu"]), P_d=float(g["P_d"]), N=int(g["N"]), eta2=float(g["eta2"]), logScanStats=True)
    for x, ok in zip(g["x0"], g["accepted"]):
        n0 = trk.nTargets
        trk.initiateTarget(Target(float(g["t0"]), None, x.copy(), pv.P0, status="preinitialized"))
        assert (trk.nTargets > n0) == bool(ok)
    rec = ou.Recording().attach(trk)
    n = int(g["n_scans"])
    for k in range(n):
        trk.addMeasurementList(MeasurementList(float(g["times"][k]), g["s%02d_z" % k]))
    uf, ovl, _ = ou.debug_counts(trk)      # (host counters: reading them does not touch the device)
    log = trk.scanStatsLog                 # the first look: folds the last two reports
    assert rec.scans() == list(range(1, n + 1)) and len(log) == n
    for s in range(1, n + 1):
        ou.check_scan_against_trace(g, s, rec.rows[s], rec.births_of(s), log[s - 1], SCORE_ATOL)
    leaf = trk.leafBatch()
    p = "s%02d_" % (n - 1)
    if p + "leaf_ID" in g.files:
        assert np.array_equal(leaf["ID"], g[p + "leaf_ID"]) and np.array_equal(leaf["meas"], g[p + "leaf_meas"])
        assert np.array_equal(leaf["x"], g[p + "leaf_x"]) and np.array_equal(leaf["P"], g[p + "leaf_P"]), "leaf states and covariances (bit for bit)"
    else:
        assert len(leaf["meas"]) == int(g[p + "leaf_n"][0])
        assert sha(np.asarray(leaf["meas"], dtype=np.int64)) == bytes(g[p + "leaf_sha_meas"]).hex(), "leaf measurement numbers (sha-256 of all leaves)"
        assert sha(np.asarray(leaf["x"], dtype=np.float64).reshape(-1, 4)) == bytes(g[p + "leaf_sha_x"]).hex(), "leaf states (sha-256 of all leaves)"
    assert uf >= n - 2 and ovl > 0, "the scans were clustered by the union-find (%d) and grow launches overlapped the previous ILP launch (%d)" % (uf, ovl)
    trk.close()
    _note("trace[%s]" % name, scans=n, uf=uf, ovl=ovl, seconds=time.perf_counter() - t0)


# ---- 2. long streamed runs against the looked-at path, at every scan -------------------------------------------------------------------------
def _run_api(sc, lists, make=_tracker, look=False, sync_every=0, prune=None):
    """One tracker over the stream, recording through the fold hooks.  look: `lastScanStats` is read after every scan (the looked-at path);
    sync_every: a device-wide synchronise every that many scans -- the host's hints are then fresh, nothing is folded early
    (`Tracker.synchronize` would drain, which is looking)."""
    import torch
    t0 = time.perf_counter()
    trk = make(sc=sc, logScanStats=True)
    rec = ou.Recording().attach(trk)
    for k, sl in enumerate(lists):
        if prune is None:
            trk.addMeasurementList(sl)
        else:
            trk.addMeasurementList(sl, pruneSimilar=prune(k))
        if look:
            _ = trk.lastScanStats
        elif sync_every and k % sync_every == sync_every - 1:
            torch.cuda.synchronize()
    counts = ou.debug_counts(trk)
    log = list(trk.scanStatsLog)      # (a streaming run's first look)
    leaf = trk.leafBatch()
    trk.close()
    return dict(rec=rec, log=log, leaf=leaf, uf=counts[0], ovl=counts[1], vt=counts[2], seconds=time.perf_counter() - t0)


def _same_run(a, b, n):
    assert a["rec"].scans() == list(range(1, n + 1))
    ou.compare_recordings(a["rec"], b["rec"])
    ou.compare_stats(a["log"], b["log"])
    assert len(a["leaf"]["ID"]) > 0
    ou.compare_leaves(a["leaf"], b["leaf"], n)


@pytest.fixture(scope="module")
def headline():
    """The headline scene (config 3 confined: 500 targets, about 13 k leaves, N = 5) and tracker A on it: looked at after every scan."""
    from pymht_amd.utils.scenario import make_config
    sc = make_config("cfg3", seed=5446, n_scans=N_LONG, confine=True)
    lists = _lists(sc)
    a = _run_api(sc, lists, look=True)
    assert a["log"][-1]["L"] > 10000 and a["log"][-1]["ilp"] > 10, "the headline regime"
    assert a["ovl"] == 0, "a host that looks after every scan flushes every commit: no any-order launch"
    _note("streamed headline A (looked at)", scans=N_LONG, L=a["log"][-1]["L"], ilp=a["log"][-1]["ilp"], uf=a["uf"], ovl=a["ovl"], vt=a["vt"], seconds=a["seconds"])
    return sc, lists, a


@pytest.mark.parametrize("sync_every", [0, 1, 5])
def test_streamed_headline_every_scan_equals_looked_at(sync_every, headline):
    """Headline size -- where the target workgroups fill the machine next to the ILP launch: B streams 240 scans and looks once at the end, the
    host never waiting (stale hints), synchronising the device after every scan, and after every fifth (fresh hints, nothing folded early).
    Every scan's report rows (all fields but the node handles) and births, the scan log and the final leaves equal A's."""
    sc, lists, a = headline
    b = _run_api(sc, lists, sync_every=sync_every)
    _note("streamed headline B sync_every=%d" % sync_every, scans=N_LONG, uf=b["uf"], ovl=b["ovl"], vt=b["vt"], seconds=b["seconds"])
    assert b["uf"] >= N_LONG - 2 and b["ovl"] > 0, (b["uf"], b["ovl"])
    _same_run(a, b, N_LONG)


@pytest.fixture(scope="module")
def cfg2_long():
    from pymht_amd.utils.scenario import make_config
    sc = make_config("cfg2", seed=5446, n_scans=N_LONG, confine=True)
    return sc, _lists(sc)


def test_streamed_generation_switches_every_scan_equals_looked_at(cfg2_long):
    """Config 2 (births and deaths on most scans): B with a value table of 2 048 ids streams without a look -- the generation switch happens in
    the middle of overlapped chains, at a scan the host picks from a hint -- against A with the default table (no switch), looked at after
    every scan."""
    sc, lists = cfg2_long
    a = _run_api(sc, lists, look=True)
    b = _run_api(sc, lists, make=_small_table)
    _note("streamed cfg2 generations A (looked at)", scans=N_LONG, uf=a["uf"], ovl=a["ovl"], vt=a["vt"], seconds=a["seconds"])
    _note("streamed cfg2 generations B (table 2048)", scans=N_LONG, uf=b["uf"], ovl=b["ovl"], vt=b["vt"], seconds=b["seconds"])
    assert a["vt"] == 0 and b["vt"] >= 3, (a["vt"], b["vt"])
    assert b["ovl"] > 0
    assert len(set(len(r) for r in a["rec"].rows.values())) > 3 and len(a["rec"].births) > 10, "births and deaths happened"
    _same_run(a, b, N_LONG)


def test_streamed_pruning_toggles_every_scan_equals_looked_at(cfg2_long):
    """Config 2 with similar-state pruning on all scans but every seventh: scans with pruning take the clustering kernel and publish no
    per-target records, scans without take the union-find -- the stream crosses between the two about 34 times without anybody looking."""
    sc, lists = cfg2_long
    on = lambda k: k % 7 != 5
    a = _run_api(sc, lists, look=True, prune=on)
    b = _run_api(sc, lists, prune=on)
    _note("streamed cfg2 pruning toggles A (looked at)", scans=N_LONG, uf=a["uf"], ovl=a["ovl"], vt=a["vt"], seconds=a["seconds"])
    _note("streamed cfg2 pruning toggles B", scans=N_LONG, uf=b["uf"], ovl=b["ovl"], vt=b["vt"], seconds=b["seconds"])
    # (a scan with pruning cannot take the union-find; how many of the others do is the library's choice)
    assert 0 < b["uf"] <= sum(1 for k in range(N_LONG) if not on(k)), "scans without pruning were clustered by the union-find (%d)" % b["uf"]
    _same_run(a, b, N_LONG)


# ---- 3. the raw replay -- what bench.py times -- at stop points --------------------------------------------------------------------------------
def _prepass(sc, lists, stops, prune=None):
    """One looked-at pass through the drop-in API (device initiator): the births per scan, as bench.py's prepass records them, and the
    reference snapshot at every stop -- header, rows, used words, the full leaf batch.  prune: similar-state pruning of scan k (0-based)."""
    trk = _tracker(sc)
    rec = ou.Recording().attach(trk)
    snaps = {}
    for k, sl in enumerate(lists[:max(stops)]):
        trk.addMeasurementList(sl, pruneSimilar=bool(prune(k)) if prune else False)
        _ = trk.lastScanStats      # looked at after every scan: the commit runs as a launch of its own
        if k + 1 in stops:
            rep = trk._rep         # (the report block of the scan just folded)
            hdr = ou.header_of(rep)
            assert hdr[0] == k + 1
            snaps[k + 1] = (hdr, rec.rows[k + 1], np.frombuffer(C.string_at(rep.used, 8 * rep.used_words), dtype=np.uint64), trk.leafBatch())
    births = [[] for _ in range(max(stops))]
    for s, b in rec.births.items():
        births[s - 1] = [(r["x0"].astype(np.float32), r["P0"].reshape(4, 4).copy(), int(r["meas"])) for r in b]
    assert ou.debug_counts(trk)[1] == 0
    dev = trk._ctx.device
    trk.close()
    return snaps, births, ou.DeviceStream(sc["scans"][:max(stops)], births, sc["P_d"], dev)


def _raw_stop(sc, stream, K, sync_every=0, make=_tracker, prune=None):
    """A fresh forest without initiator, scans 1..K stepped with `mht_forest_step` on scans resident in HBM, the births replayed with
    `mht_forest_add_targets_dev`, no report call in between.  sync_every: `mht_synchronize` every that many scans (waits, flushes nothing).
    Returns the counters read BEFORE the report, the report's return code, the snapshot and the tracker (still open)."""
    from pymht_amd import _lib
    trk = make(sc=sc, useInitiator=False)
    for k in range(K):
        if prune:
            trk._set_prune_similar(bool(prune(k)))      # (`mht_forest_set_prune_similar`: a host-side switch, nothing is flushed)
        stream.step(trk, k)
        if sync_every and k % sync_every == sync_every - 1:
            _lib.check(trk._lib.mht_synchronize(trk._ctx.handle))
    uf, ovl, vt = ou.debug_counts(trk)
    rc, hdr, rows, used = ou.read_report(trk)
    snap = None if rc else (hdr, rows, used, ou.leaf_export(trk, hdr))
    return (uf, ovl, vt), rc, snap, trk


def _raw_case(case, sc, pre, stops, sync_every=0, make=_tracker, ovl_half_at_last=False, vt_at_last=0, prune=None):
    snaps, _, stream = pre
    for K in stops:
        t0 = time.perf_counter()
        (uf, ovl, vt), rc, snap, trk = _raw_stop(sc, stream, K, sync_every, make, prune)
        trk.close()
        _note("%s K=%d" % (case, K), uf=uf, ovl=ovl, vt=vt, seconds=time.perf_counter() - t0)
        assert rc == 0, "stop %d: report returned %d" % (K, rc)
        ou.compare_snapshot(snaps[K], snap, K)
        if K >= 3 and prune is None:
            assert ovl > 0, "stop %d: no grow launch overlapped the previous scan's ILP launch (uf %d)" % (K, uf)
        if K == stops[-1]:
            if ovl_half_at_last:      # (a condition on the scene: a birth scan breaks the chain for a launch or two, config 3 confined gives birth rarely)
                assert ovl >= K / 2, "stop %d: only %d any-order launches" % (K, ovl)
            assert vt >= vt_at_last, "stop %d: %d generation switches" % (K, vt)


@pytest.fixture(scope="module")
def headline_raw():
    from pymht_amd.utils.scenario import make_config
    sc = make_config("cfg3", seed=5446, n_scans=N_RAW, confine=True)
    stops = ou.stop_set(sc["N"], N_RAW)
    t0 = time.perf_counter()
    pre = _prepass(sc, _lists(sc), stops)
    _note("raw headline pre-pass", scans=N_RAW, births=sum(len(b) for b in pre[1]), seconds=time.perf_counter() - t0)
    assert pre[0][N_RAW][0][3] > 10000 and pre[0][N_RAW][0][7] > 10, "the headline regime"
    return sc, stops, pre


@pytest.fixture(scope="module")
def cfg2_raw():
    from pymht_amd.utils.scenario import make_config
    sc = make_config("cfg2", seed=5446, n_scans=N_RAW, confine=True)
    stops = ou.stop_set(sc["N"], N_RAW)
    t0 = time.perf_counter()
    pre = _prepass(sc, _lists(sc), stops)      # (default table: no generation switch)
    _note("raw cfg2 pre-pass", scans=N_RAW, births=sum(len(b) for b in pre[1]), seconds=time.perf_counter() - t0)
    assert sum(1 for b in pre[1] if b) > 20, "births on many scans"
    return sc, stops, pre


def test_raw_replay_headline_stop_points_host_never_waiting(headline_raw):
    """The replay as bench.py drives it, the host never waiting (its hints are as stale as the launch queue is deep): every stop equals the
    looked-at pass -- header, every row field but the node handles, used words, every leaf key but `node`."""
    sc, stops, pre = headline_raw
    assert stops == [1, 2, 3, 5, 6, 8, 9, 10, 19, 59, 60, 61, 63, 64, 65, 128, 200]
    _raw_case("raw headline never waiting", sc, pre, stops, ovl_half_at_last=True)


def test_raw_replay_headline_stop_points_fresh_hints(headline_raw):
    """The same with `mht_synchronize` after every scan: the hint words are fresh at every step; `ovl` shows that the wait flushes no commit."""
    sc, stops, pre = headline_raw
    _raw_case("raw headline sync every scan", sc, pre, stops, sync_every=1, ovl_half_at_last=True)


def test_raw_replay_generation_switches_stop_points(cfg2_raw):
    """Config 2 (N = 3) with a value table of 2 048 ids and a synchronise every 4 scans -- inside the slack the switch is documented for (a hint
    that lags a scan or two: 2 (R + 3) x the largest per-scan consumption): the generation switches in the middle of raw overlapped chains."""
    sc, stops, pre = cfg2_raw
    assert stops == [1, 2, 3, 4, 6, 7, 8, 15, 59, 60, 61, 63, 64, 65, 128, 200]
    _raw_case("raw cfg2 table 2048 sync every 4", sc, pre, stops, sync_every=4, make=_small_table, vt_at_last=3)


def test_raw_replay_small_table_host_never_waiting(cfg2_raw):
    """The same table with the host never waiting, to the last stop: the host may be hundreds of scans ahead of the hint the switch is timed
    by.  Either the result equals the looked-at pass, or the report returns MHT_E_CAPACITY and the forest refuses further steps -- never a
    clean report with other content ("Raw replay": which of the two happens)."""
    from pymht_amd import _lib
    sc, stops, pre = cfg2_raw
    K = stops[-1]
    t0 = time.perf_counter()
    (uf, ovl, vt), rc, snap, trk = _raw_stop(sc, pre[2], K, make=_small_table)
    try:
        _note("raw cfg2 table 2048 never waiting K=%d" % K, uf=uf, ovl=ovl, vt=vt, outcome="equal" if rc == 0 else "error %d" % rc, seconds=time.perf_counter() - t0)
        if rc == 0:
            ou.compare_snapshot(pre[0][K], snap, K)
        else:
            assert rc == _lib.MHT_E_CAPACITY, rc
            with pytest.raises(_lib.MhtError):      # the forest refuses further scans
                pre[2].step(trk, 0)
    finally:
        trk.close()


def test_raw_replay_pruning_toggles_stop_points(cfg2_raw):
    """Config 2 with similar-state pruning on all scans but every seventh (`mht_forest_set_prune_similar` between the steps, nobody looks):
    scan 6 is clustered by the union-find and publishes per-target records, scan 7 -- a stop -- takes the clustering kernel right behind it.
    That scan's grow launch used to overlap scan 6's ILP launch and file its edge list under compacted indices it did not have yet
    (DESIGN.md section 4).  No any-order launch is expected here: a union-find scan never follows one."""
    sc, stops, _ = cfg2_raw
    on = lambda k: k % 7 != 5
    t0 = time.perf_counter()
    pre = _prepass(sc, _lists(sc), stops, prune=on)
    _note("raw cfg2 pruning toggles pre-pass", scans=N_RAW, births=sum(len(b) for b in pre[1]), seconds=time.perf_counter() - t0)
    assert not on(5) and on(6) and 7 in stops and 8 in stops
    _raw_case("raw cfg2 pruning toggles", sc, pre, stops, prune=on)


# ---- 4. a sector group at stop points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", ["0", "1"])
def test_group_raw_replay_uneven_sectors_stop_points(light, monkeypatch):
    """The scene of test_group_raw_replay_uneven_sectors (three sectors of different sizes, one sees nothing for a scan) over 30 scans: a fresh
    group per stop, stepped through `mht_group_step` without a look (every commit rides in the next batched grow launch), against single
    forests that are looked at after every scan; light ILP pass forced off and on."""
    import torch
    from pymht_amd import _lib
    from pymht_amd.sectors import SectorGroup
    from pymht_amd.utils.scenario import make_scenario
    monkeypatch.setenv("MHT_BLP_LIGHT", light)
    t0 = time.perf_counter()
    n_scans, N = 30, 3
    params = [dict(T=60, radius=500.0, lambda_phi=3e-5), dict(T=7, radius=300.0, lambda_phi=1e-5), dict(T=200, radius=2500.0, lambda_phi=2e-6)]
    scs = []
    for q, pr in enumerate(params):
        sc = make_scenario(n_scans=n_scans, P_d=0.85, seed=100 + q, centre=(0.0, 20000.0 * q), **pr)
        sc["N"] = N
        scs.append(sc)
    scs[1]["scans"][4] = np.zeros((0, 2), np.float32)      # a sector that sees nothing for a scan
    stops = ou.group_stop_set(N, n_scans)
    assert stops == [1, 2, 4, 7, 8, 30]
    dev = torch.device("cuda", 0)
    zd = [[torch.from_numpy(np.ascontiguousarray(z, np.float32).reshape(-1, 2) if len(z) else np.zeros((1, 2), np.float32)).to(dev) for z in sc["scans"]] for sc in scs]
    M = [[len(z) for z in sc["scans"]] for sc in scs]

    def snapshot(trk, what):
        rc, hdr, rows, used = ou.read_report(trk)
        assert rc == 0, (what, rc)
        return hdr, rows, used, ou.leaf_export(trk, hdr)

    ref = [{} for _ in scs]
    for q, sc in enumerate(scs):      # single forests, looked at after every scan
        solo = _tracker(sc, useInitiator=False)
        for k in range(n_scans):
            _lib.check(solo._lib.mht_forest_step(solo._ctx.handle, zd[q][k].data_ptr(), M[q][k]))
            snap = snapshot(solo, ("solo", q, k))
            if k + 1 in stops:
                ref[q][k + 1] = snap
        solo.close()
    for K in stops:
        members = [_tracker(sc, useInitiator=False) for sc in scs]
        grp = SectorGroup(members)
        for k in range(K):
            grp.step_dev([zd[q][k].data_ptr() for q in range(3)], [M[q][k] for q in range(3)])
        for q in range(3):
            try:
                ou.compare_snapshot(ref[q][K], snapshot(members[q], ("group", q, K)), K)
            except AssertionError as e:
                raise AssertionError("sector %d, light %s: %s" % (q, light, e))
        grp.close()
        for t in members:
            t.close()
    _note("group uneven sectors light=%s" % light, stops=len(stops), seconds=time.perf_counter() - t0)
