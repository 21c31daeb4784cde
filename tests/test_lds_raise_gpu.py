"""GPU: kernels launched with more than 48 KB of dynamic LDS.  Every kernel instance gets its limit raised by the launch that first
needs it (mht_common.h: launch_kernel), per context -- an instance whose raise is missing fails to launch, but only above 48 KB, which
the small shapes of the other tests never reach in the one-sector grow kernels of a plain forest.

What makes the grow workgroup large is the scan, not the forest's capacity: its hit masks are ceil(M / 64) words per leaf for the M
measurements of the scan.  fgrow_lds_bytes_cap(W = 29, pds = 8, AW, 96 leaves) = 2 * 29 * 256 (measurements) + 96 * 144 (leaf records)
+ 96 * 29 * 8 (hit masks) + ... = 64 KB, 78 KB with 128 leaves per pass.  So the plain scenes carry ~1 800 measurements per scan in a
forest made for 2 048: five ships, and clutter so sparse (2.3e-7 per m^2 over a disc of 50 km) that it neither gates nor starts tracks
worth mentioning -- the oracle stays at a quarter of a second per scan.  The AIS forest with N = 8 is above 48 KB with any scan (its
32-int path records alone are 24 KB per workgroup)."""
import functools

import numpy as np
import pytest

from test_tracker_gpu import SCORE_ATOL, make_tracker, tracker_selected

pytestmark = pytest.mark.gpu

N_SCANS = 12
MAX_MEAS = 2048


@functools.lru_cache(maxsize=None)
def _plain_reference(N):
    """(scene, oracle results after every scan): computed once per window, shared by the runs below and never modified."""
    from pymht_amd.utils.scenario import make_scenario
    from trace_util import make_oracle
    sc = make_scenario(T=5, radius=50000.0, lambda_phi=2.3e-7, n_scans=N_SCANS, P_d=0.9, seed=4700)
    assert all(1700 < len(z) <= MAX_MEAS for z in sc["scans"])      # W = 27..31 words per leaf: 60 KB and more
    o = make_oracle(dict(period=sc["period"], lambda_phi=sc["lambda_phi"], lambda_nu=1e-4, P_d=sc["P_d"], N=N, eta2=5.99,
                         x0=sc["x0"], t0=sc["t0"], accepted=[True] * len(sc["x0"])))
    after = []
    for z, t in zip(sc["scans"], sc["times"]):
        info = o.add_scan(float(t), z)
        after.append(dict(L=info["L"], G=info["G"], unused=np.array(info["unused"]), ids=[r.ID for r in o.targets], sel=o.selected(),
                          leaf=o.leaf_batch(), n_clusters=len(o.clusters), n_ilp=o.n_ilp))
    return sc, after


def _plain_tracker(sc, N, **kw):
    trk, acc = make_tracker(sc["period"], sc["lambda_phi"], 1e-4, sc["P_d"], N, 5.99, sc["x0"], sc["t0"],
                            maxTargets=64, maxNodes=1 << 15, maxMeasurements=MAX_MEAS, **kw)      # (the device initiator is on by default)
    assert all(acc)
    return trk


def _compare_plain(trk, want, what):
    assert [r.ID for r in trk.__targetList__] == want["ids"], what
    ts, tb = tracker_selected(trk), trk.leafBatch()
    assert np.array_equal(want["sel"]["ID"], ts["ID"]) and np.array_equal(want["sel"]["meas"], ts["meas"]), what
    assert np.array_equal(want["sel"]["x"], ts["x"]), what
    assert np.allclose(want["sel"]["cnllr"], ts["cnllr"], rtol=0, atol=SCORE_ATOL), what
    assert np.array_equal(want["leaf"]["ID"], tb["ID"]) and np.array_equal(want["leaf"]["meas"], tb["meas"]), what
    assert np.array_equal(want["leaf"]["x"], tb["x"]), what      # every leaf state, bit for bit
    assert np.allclose(want["leaf"]["cnllr"], tb["cnllr"], rtol=0, atol=SCORE_ATOL), what
    assert want["n_clusters"] == len(trk.__clusterList__), what


@pytest.mark.parametrize("N", [3, 8])      # path records of 8 ints (fgrow_kernel<2>) and of 16 (fgrow_kernel<4>; targets of more than 128 leaves)
@pytest.mark.parametrize("streamed", [False, True])
def test_plain_forest_with_long_scans_equals_live_oracle(N, streamed):
    """A host that looks at the tracker after every scan takes the plain launch (the commit and the admission run behind the scan, in a
    launch of their own); a host that streams the scans in takes the admission launch and the any-order launch (the commit rides in the
    next scan's grow launch, which may start before the ILP launch in front of it has ended).  Scan by scan, and the end state of the
    stream, against the oracle."""
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, after = _plain_reference(N)
    trk = _plain_tracker(sc, N)
    try:
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            trk.addMeasurementList(MeasurementList(float(t), z))
            if streamed:
                continue
            st, want = trk.lastScanStats, after[k]
            assert (st["L"], st["G"]) == (want["L"], want["G"]), k
            assert np.array_equal(st["unused"], want["unused"]), k
            assert want["n_ilp"] == trk.nOptimSolved, k
            _compare_plain(trk, want, "scan %d" % k)
        _compare_plain(trk, after[-1], "end state")
    finally:
        trk.close()


def test_ais_forest_with_a_window_of_eight_equals_live_oracle():
    """fgrow_ais_kernel<8> (records of 32 ints) in a forest made for 2 048 measurements, scan by scan against the oracle: decisions and
    identities exact, every leaf state bit for bit."""
    from ais_long_util import AIS_SCORE_ATOL, long_window_scenario, make_pair, msgs_of, oracle_msgs_of, prune_on
    from trace_util import oracle_rows
    from pymht_amd.utils.classDefinitions import MeasurementList
    N = 8
    sc, ais = long_window_scenario(4188, N, T=5, n_scans=N_SCANS)
    trk, o = make_pair(sc, N, False, max_meas=MAX_MEAS)
    try:
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            info = o.add_scan(float(t), z, prune_similar=prune_on(k), ais=oracle_msgs_of(ais[k]), ais_initialization=False)
            trk.addMeasurementList(MeasurementList(float(t), z), msgs_of(ais[k]), aisInitialization=False, pruneSimilar=prune_on(k))
            st, tb = trk.lastScanStats, trk.leafBatch()
            lb = oracle_rows([l for r in o.targets for l in r.leaves()])
            assert st["L"] == info["L"] and np.array_equal(st["unused"], info["unused"]), k
            assert [r.ID for r in o.targets] == [r.ID for r in trk.__targetList__], k
            for key in ("ID", "meas", "mmsi", "x", "Pf64"):
                assert np.array_equal(lb[key], tb[key]), (k, key)
            assert np.allclose(lb["cnllr"], tb["cnllr"], rtol=0, atol=AIS_SCORE_ATOL), k
            assert o.n_ilp == trk.nOptimSolved, k
        assert any(len(a) for a in ais)
    finally:
        trk.close()


def test_groups_on_two_devices_in_one_process():
    """A group of two sectors on device 0, then one on device 1 in the same process: the second device's kernels need their limits
    raised as well (the attribute belongs to the function on one device).  Both against single forests."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from pymht_amd.sectors import SectorGroup
    from pymht_amd.utils.classDefinitions import MeasurementList
    N = 3
    sc, _ = _plain_reference(N)
    for dev in (0, 1):
        solo = [_plain_tracker(sc, N, device=dev, deviceTiming=False) for _ in range(2)]
        grp_t = [_plain_tracker(sc, N, device=dev, deviceTiming=False) for _ in range(2)]
        grp = SectorGroup(grp_t)
        try:
            for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
                for q in solo:
                    q.addMeasurementList(MeasurementList(float(t), z))
                grp.addMeasurementLists([MeasurementList(float(t), z) for _ in range(2)])
            for q in range(2):
                la, lb = grp_t[q].leafBatch(), solo[q].leafBatch()
                for key in la:
                    if key != "node":      # node indices are handles (block taken with an atomic)
                        assert np.array_equal(la[key], lb[key]), (dev, q, key)
        finally:
            grp.close()
            for q in solo + grp_t:
                q.close()
