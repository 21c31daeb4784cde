"""GPU: the LINEAR six-state forest -- Tracker(pymht_amd.models.ca, ...): the four-state forest's kernels (fgrow_kernel, fgrow_batch_kernel,
blp_uf_kernel, prune_similar_kernel, the covariance value table, commit, chains) compiled at NX = 6, a gains row of 80 bytes, 36 floats per
covariance value -- held to the live oracle and to itself beyond the one recorded trace G17: random scenarios with random acceleration
tails, similar-state pruning, streamed hosts, fused groups whose mean is a new covariance value, windows of 8 and 9 scans, switches of the
value table's generation, sector groups (the batched launch set) and the cluster-sharded step.  What every scene reaches is asserted from
the oracle alone, without a device, in tests/test_six_state_fuzz_cpu.py; the figures in the docstrings below are that census."""
import ctypes as C

import numpy as np
import pytest

import fuzz_util
from fuzz_util import CA_PLAIN_SEEDS as PLAIN_SEEDS, CA_SIMILAR_SEEDS as SIMILAR_SEEDS, CA_MAX_LEAVES as MAX_LEAVES

pytestmark = pytest.mark.gpu

# seeds taken out of a slice, with the reason: at most 2 of 24, and only where the scenario's ILP optimum is shown not to be unique (re-solved
# with the device's selection as a constraint: the same objective).  None so far.
EXCLUDED = {}


def _slice(seeds, **kw):
    bad, total = [], {}
    for seed in seeds:
        if seed in EXCLUDED:
            continue
        ok, desc, msg, census = fuzz_util.run_case_ca(seed, max_leaves=MAX_LEAVES, **kw)
        fuzz_util.add_census(total, census)
        if not ok:
            bad.append(desc + ' ' + msg)
    assert len(EXCLUDED) <= 2
    assert not bad, "\n".join(bad)
    return total


def test_ca_fuzz_slice_against_oracle():
    """24 random scenarios with random acceleration tails, looked at after every scan.  Census (oracle): 240 ILPs, largest cluster 40
    targets, 71 terminations, largest scan 5 068 leaves, no fused group."""
    c = _slice(PLAIN_SEEDS)
    assert c["ilp"] >= 100 and c["cluster"] >= 16 and c["dead"] >= 30 and c["L"] >= 1000


def test_ca_fuzz_slice_with_similar_state_pruning():
    """24 scenarios with similar-state pruning on three scans of four and a random merge radius.  Census (oracle): 357 ILPs, largest cluster
    56 targets, 125 terminations, largest scan 2 515 leaves, 1 902 fused groups (1 876 of one hit, 24 of two, 2 of three)."""
    c = _slice(SIMILAR_SEEDS, similar=True)
    assert len(c["groups"]) >= 500


def test_ca_fuzz_slice_streamed():
    """16 of the plain seeds with a host that streams the scans in and looks once at the end (the commits ride in the next scan's grow
    launch): per-scan statistics from the tracker's log, the final state in full.  Census (oracle): 186 ILPs, largest cluster 40 targets,
    45 terminations, largest scan 5 068 leaves."""
    c = _slice(PLAIN_SEEDS[:16], streamed=True)
    assert c["ilp"] >= 80


def _large_groups(name, model):
    scene = fuzz_util.crafted_scene(name, model)
    rec = fuzz_util.oracle_run(scene)
    assert rec["census"]["merged_leaves"] > 0 and max(rec["census"]["groups"]) >= 6
    ok, msg = fuzz_util.device_run(scene, rec)
    assert ok, scene["desc"] + ' ' + msg


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_ca_similar_state_pruning_large_groups(name):
    """Dense scenes whose fused groups are large, pruning on at every scan, against the live oracle: a mean over n hits that is not one of
    the hits' covariances (n other than 1, 2, 4) is a NEW value -- mht_similar.hip::fuse_group inserts it, takes a pseudo-parent key and
    writes a gains row (vt_gains).  The covariance of every merged leaf is held to the oracle's np.mean at FUZZ_REL; no leaf carries flag 8.
    Census (oracle), group size: count -- A {1: 67, 2: 31, 3: 12, 4: 3, 5: 1, 6: 1}, 16 ILPs, largest cluster 10 targets, 100 merged leaves;
    B {1: 47, 2: 17, 3: 20, 4: 16, 5: 14, 6: 4, 7: 5}, 5 ILPs, largest cluster 2, 34 merged leaves;
    C {1: 2, 2: 3, 3: 2, 4: 4, 5: 4, 6: 1, 7: 3, 8: 1, 9: 1, 11: 1, 23: 1}, 1 ILP, largest cluster 2, 11 merged leaves."""
    _large_groups(name, "ca")


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_pv_similar_state_pruning_large_groups(name):
    """The same three scenes under models.pv: the four-state build's first groups beyond six hits.  Census (oracle), group size: count --
    A {1: 102, 2: 42, 3: 12, 4: 2, 5: 1, 6: 1}, 20 ILPs, largest cluster 9 targets; B {1: 42, 2: 13, 3: 10, 4: 14, 5: 6, 6: 4, 7: 1}, 5 ILPs;
    C {3: 10, 4: 7, 5: 14, 6: 15, 7: 10, 8: 8, 9: 4, 10: 6, 11: 6, 12: 2, 14: 1, 17: 1, 18: 2, 20: 2} and 3 smaller, 2 ILPs."""
    _large_groups(name, "pv")


@pytest.mark.parametrize("N", [8, 9])
def test_ca_long_window(N):
    """Windows of 8 and 9 scans (path records of 16 ints, targets of more than 128 leaves) over 12 scans: one tracker looked at after
    every scan, one streamed, both against one oracle run.  Census (oracle): N = 8: 17 ILPs, largest cluster 14 targets, largest scan
    3 887 leaves; N = 9: 16 ILPs, largest cluster 10 targets, largest scan 6 806 leaves."""
    scene = fuzz_util.long_window_scene(N)
    rec = fuzz_util.oracle_run(scene)
    assert rec["census"]["scans"] == 12 and rec["census"]["L"] > 2000
    for streamed in (False, True):
        ok, msg = fuzz_util.device_run(scene, rec, streamed=streamed)
        assert ok, scene["desc"] + ' ' + msg


def _tracker(scene, **kw):
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    model = fuzz_util._model_of(scene)
    sc = scene["sc"]
    kw.setdefault("useInitiator", False)
    trk = Tracker(model, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=scene["N"], eta2=scene["eta2"], maxTargets=256, maxNodes=1 << 18,
                  maxMeasurements=512, pruneThreshold=scene["thr"], **kw)
    trk._add_targets([Target(sc["t0"], None, x.copy(), model.P0, status="preinitialized") for x in scene["x0"]])
    return trk


def _scan(scene, k):
    from pymht_amd.utils.classDefinitions import MeasurementList
    return MeasurementList(float(scene["sc"]["times"][k]), scene["sc"]["scans"][k])


def _same_state(a, b, what):
    """Device against device: the scan's report and the whole leaf batch bit for bit (node indices are handles: a block taken with an atomic)."""
    sa, sb = a._sel[0], b._sel[0]
    for name in ("id", "status", "sel_meas", "sel_x", "sel_cnllr", "score", "root_scan", "root_meas", "root_x", "n_leaves", "cluster"):
        assert np.array_equal(sa[name], sb[name]), (what, name)
    for k in ("L", "G", "M", "leaves_out", "clusters", "ilp"):
        assert a.lastScanStats[k] == b.lastScanStats[k], (what, k)
    la, lb = a.leafBatch(), b.leafBatch()
    for key in la:
        if key != "node":
            assert np.array_equal(la[key], lb[key]), (what, key)


def _rebuilds(trk):
    from pymht_amd import _lib
    r = np.zeros(1, np.int32)
    _lib.check(trk._lib.mht_forest_debug_read(trk._ctx.handle, b"vt_rebuilds", r.ctypes.data_as(C.c_void_p), 4))
    return int(r[0])


def test_ca_value_table_generations(monkeypatch):
    """The covariance-value table at 36 floats per value and 80-byte gains rows: a table of 2 048 ids (MHT_VTAB_CAP) switches its generation
    while the default table never does; ids, measurement numbers, states, scores and covariances of all leaves must be the same bits after
    every scan.  Similar-state pruning is on for six scans of seven (merged nodes carry keys of their own through the switch).
    The stream: 12 targets at cfg2's clutter density, 22 scans -- the device switches in front of scans 11 and 20 (20 scans is the shortest
    stream that reaches two switches; the last two scans run with both generations in the ring): vt_rebuilds = 2.  cfg2's own 50 targets
    overflow a 2 048-id table at six states in scan 16 (MHT_E_CAPACITY, as documented: ~350 new values per scan, and a generation has to
    last R + 2 scans).  Census (oracle): 39 ILPs, largest cluster 10 targets, largest scan 140 leaves, 79 fused groups of one hit."""
    scene = fuzz_util.vtab_scene()
    ref = _tracker(scene)
    monkeypatch.setenv("MHT_VTAB_CAP", "2048")
    small = _tracker(scene)
    monkeypatch.delenv("MHT_VTAB_CAP")
    try:
        for k in range(len(scene["on"])):
            for t in (ref, small):
                t.addMeasurementList(_scan(scene, k), pruneSimilar=scene["on"][k])
            _same_state(small, ref, "scan %d" % k)
        print("vt_rebuilds", _rebuilds(small), "leaves", ref.lastScanStats["L"])
        assert _rebuilds(ref) == 0 and _rebuilds(small) >= 2, (_rebuilds(ref), _rebuilds(small))
    finally:
        ref.close()
        small.close()


@pytest.mark.parametrize("light", ["0", "1"])
def test_ca_sector_group_equals_solo_trackers(light, monkeypatch):
    """Linear six-state members share a group's BATCHED launch set (fgrow_batch_kernel at NX = 6; only AIS-aided and constant-turn members
    have launches of their own): two ca trackers on different scenes, member 0 pruning on three scans of four, member 1 never, with the
    group's light ILP pass forced off and on -- after every scan each member must be, bit for bit, the same tracker stepped alone.
    Census (oracle): sector 0: 20 ILPs, largest cluster 35 targets, 2 terminations, largest scan 411 leaves, 77 fused groups (75 of one
    hit, 2 of two); sector 1: 18 ILPs, largest cluster 28 targets, largest scan 336 leaves."""
    from pymht_amd.sectors import SectorGroup
    monkeypatch.setenv("MHT_BLP_LIGHT", light)
    scenes = fuzz_util.sector_scenes()
    solo = [_tracker(s) for s in scenes]
    grouped = [_tracker(s) for s in scenes]
    grp = SectorGroup(grouped)
    try:
        assert grp._batched == [0, 1]
        n_ilp = 0
        for k in range(len(scenes[0]["on"])):
            flags = [s["on"][k] for s in scenes]
            for q in range(2):
                solo[q].addMeasurementList(_scan(scenes[q], k), pruneSimilar=flags[q])
            grp.addMeasurementLists([_scan(s, k) for s in scenes], pruneSimilar=flags)
            for q in range(2):
                _same_state(grouped[q], solo[q], "scan %d sector %d" % (k, q))
                n_ilp += solo[q].lastScanStats["ilp"]
        assert n_ilp >= 10
    finally:
        grp.close()
        for t in solo + grouped:
            t.close()


def test_sector_group_refuses_batched_members_of_two_state_dimensions():
    """A ca member and a pv member would both go into the batched launch set, but they live in different libraries (libmht_amd6.so and
    libmht_amd.so: one mht_group_create cannot take both forests): the group is refused when it is made, and the trackers go on alone."""
    from pymht_amd.sectors import SectorGroup
    scenes = [fuzz_util.crafted_scene("A", "ca"), fuzz_util.crafted_scene("A", "pv")]
    members = [_tracker(s) for s in scenes]
    try:
        with pytest.raises(ValueError, match="state dimension"):
            SectorGroup(members)
        for t, s in zip(members, scenes):
            t.addMeasurementList(_scan(s, 0))
            assert t.lastScanStats["L"] > 0
    finally:
        for t in members:
            t.close()


def test_ca_cluster_sharded_equals_single_tracker():
    """ClusterShardedTracker with two shards in one process (two contexts, the all-reduce(MAX) replaced by an element-wise maximum) against
    a solo ca tracker, scan by scan, on the plain slice's seed 320017.  Census (oracle): 12 ILPs over 8 scans, largest cluster 34 targets,
    11 terminations, largest scan 752 leaves."""
    import torch
    from pymht_amd.parallel import ClusterShardedTracker
    scene = fuzz_util.ca_scene(fuzz_util.SHARDED_SEED)
    rec = fuzz_util.oracle_run(scene, MAX_LEAVES)
    assert rec["census"]["cluster"] >= 16
    solo = _tracker(scene)
    parts = [ClusterShardedTracker(_tracker(scene), 2, i, exchange=lambda t: None) for i in range(2)]
    solved = [0, 0]
    try:
        for k, r in enumerate(rec["scans"]):
            sl = _scan(scene, k)
            solo.addMeasurementList(sl)
            for p in parts:
                p.begin(sl)
            both = torch.stack([(p.sel_rel >= 0).int() for p in parts])
            assert int(both.sum(dim=0).max()) <= 1, "a target was solved by two shards"
            for i in range(2):
                solved[i] += int(both[i].sum())
            merged = torch.stack([p.sel_rel for p in parts]).max(dim=0).values
            for p in parts:
                p.sel_rel.copy_(merged)
                p.end()
            assert solo.lastScanStats["ilp"] == r["n_ilp"] and [t.ID for t in solo.__targetList__] == r["ids"], k
            for i, p in enumerate(parts):
                sa, sb = p.trk._sel[0], solo._sel[0]
                for name in ("id", "status", "sel_meas", "sel_x", "sel_cnllr", "n_leaves", "cluster"):
                    assert np.array_equal(sa[name], sb[name]), (k, i, name)
                la, lb = p.trk.leafBatch(), solo.leafBatch()
                for key in la:
                    if key != "node":
                        assert np.array_equal(la[key], lb[key]), (k, i, key)
        assert min(solved) > 0, solved
    finally:
        solo.close()
        for p in parts:
            p.trk.close()
