"""GPU: the target workgroup of the grow launch (pymht_amd/csrc/mht_fgrow_dev.h: target_part, target_tail, fg_emit_child) on the OVERLAPPING
path, at the sizes where its code changes path -- held to the looked-at path at every scan and to the live oracle.

Scenes from grow_workgroup_util (checked on the CPU by test_grow_workgroup_scenes_cpu.py), at most 8 targets:
  * planted: four targets whose children counts per scan sit on the wavefront edges of the emission (63 / 64 / 65, 127 / 128 / 129, 192 / 193 in
    one chunk), whose leaf counts sit on the edges of the count phase (1, 63, 64, 65, 127, 128 leaves in one pass; 129, 192, 193 in two) and
    which have scans without any hit (one leaf, four leaves, 192 leaves);
  * tail: a target dies (leaves the radar's range) in the middle of a cluster; the overlapping scan right behind the death learns from the
    commit's word (FCounts::ni_flag, bit 32) that compacted indices and slots differ and redoes its place in the union-find under the
    alternative epoch -- a cluster with members behind the dead slot comes out wrong if it does not.  Four-state build and a constant-turn
    forest (six-state build; its candidate list is live during the emission).  A constant-turn forest's grow launch is never any-order
    (Forest::ovl_ok), its workgroups take the overlapping code path all the same (FDyn::ovl: deferred commit, records, tail), so the `ovl`
    counter is asserted on the four-state build only.
Every scan K of a raw replay that never looks (a fresh forest per K, `mht_forest_step` K times, one report at the end) is compared with the same
stream looked at after every scan (tests/overlap_util.py: header, report rows -- clusters, selections, leaves kept --, used words, leaf export)."""
import numpy as np
import pytest

import grow_workgroup_util as gw
import overlap_util as ou

pytestmark = pytest.mark.gpu


def _tracker(sc, model=None, **kw):
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import pv
    m = pv if model is None else model
    trk = Tracker(m, sc["period"], sc["lambda_phi"], gw.LAMBDA_NU, P_d=sc["P_d"], N=sc["N"], eta2=gw.ETA2, maxTargets=1024, maxNodes=1 << 18, maxMeasurements=1024,
                  useInitiator=False, **kw)
    trk._add_targets([Target(sc["t0"], None, x.copy(), m.P0, status="preinitialized") for x in sc["x0"]])
    return trk


def _snapshot(trk, what):
    rc, hdr, rows, used = ou.read_report(trk)
    assert rc == 0, (what, rc)
    return hdr, rows, used, ou.leaf_export(trk, hdr)


def _looked_at(sc, model=None, **kw):
    """The stream stepped through the raw ABI and looked at after EVERY scan (every report flushes the commit: no launch overlaps)."""
    trk = _tracker(sc, model, **kw)
    stream = ou.DeviceStream(sc["scans"], [[] for _ in sc["scans"]], sc["P_d"], trk._ctx.device)
    snaps = {}
    for k in range(len(sc["scans"])):
        stream.step(trk, k)
        snaps[k + 1] = _snapshot(trk, ("looked at", k + 1))
    assert ou.debug_counts(trk)[1] == 0
    trk.close()
    return snaps, stream


def _never_looking(sc, stream, K, model=None, **kw):
    trk = _tracker(sc, model, **kw)
    for k in range(K):
        stream.step(trk, k)
    uf, ovl, _ = ou.debug_counts(trk)
    snap = _snapshot(trk, ("never looking", K))
    trk.close()
    return uf, ovl, snap


# ---- planted children and leaf counts ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    sc = gw.planted_scene()
    snaps, stream = _looked_at(sc)
    return sc, snaps, stream


def test_planted_counts_are_reached_on_the_device(planted):
    """Read from the report: while the window fills nothing is pruned, so a row's `n_leaves` (leaves kept) is the target's children count of
    that scan, and the header carries the sums."""
    sc, snaps, _ = planted
    seen = set()
    for K in range(1, len(sc["scans"]) + 1):
        hdr, rows = snaps[K][0], snaps[K][1]
        assert rows["n_leaves"].tolist() == [p[K - 1] for p in gw.PLANS], K
        assert hdr[3] == sum(sc["leaves_in"][K - 1]) and hdr[4] == sum(sc["children"][K - 1]), (K, hdr)
        seen |= set(rows["n_leaves"].tolist())
    assert {63, 64, 65, 127, 128, 129, 192, 193} <= seen
    assert {1, 63, 64, 65} <= {n for row in sc["leaves_in"] for n in row} and max(max(row) for row in sc["leaves_in"]) > 128


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_planted_overlapping_scan_equals_looked_at(K, planted):
    """Scan K of the replay that never waits: header, report rows (clusters, selections, leaves kept), used words and every leaf equal the
    looked-at stream's.  K = 2: 63 / 64 / 65 children from 7 / 8 / 5 leaves; K = 3: 127 / 128 / 129 children from 63 / 64 / 65 leaves, four
    leaves without a hit; K = 4: 192 / 193 children from 127 / 128 leaves, 129 leaves in two passes; K = 5: 192 leaves in two passes without
    a hit, 193 leaves in two passes."""
    sc, snaps, stream = planted
    uf, ovl, snap = _never_looking(sc, stream, K)
    ou.compare_snapshot(snaps[K], snap, K)
    assert snap[1]["n_leaves"].tolist() == [p[K - 1] for p in gw.PLANS]
    assert uf == K
    if K >= 3:
        assert ovl > 0, "scan %d: no grow launch overlapped the previous scan's ILP launch" % K


# ---- the tail behind a death --------------------------------------------------------------------------------------------------------------------
def _tail_case(model, monkeypatch=None):
    sc = gw.tail_scene(model=model)
    s_dead = gw.tail_conditions(sc)
    kw = dict(position=np.array([0.0, 0.0]), radarRange=sc["range"])
    snaps, stream = _looked_at(sc, model, **kw)
    n = len(sc["scans"])
    # the looked-at stream against the live oracle: the death, the clusters, the selections of every scan
    for K in range(1, n + 1):
        rows = snaps[K][1]
        dead_ids = sorted(rows["id"][rows["status"] != 0].tolist())
        assert dead_ids == sorted(sc["dead"][K - 1]), (K, dead_ids)
        cl = ou.clusters_of(rows)
        assert len(cl) == len(sc["clusters"][K - 1]) and all(np.array_equal(a, b) for a, b in zip(cl, sc["clusters"][K - 1])), (K, [c.tolist() for c in cl])
        alive = rows[rows["status"] == 0]
        assert alive["id"].tolist() == sc["ids"][K - 1] and np.array_equal(alive["sel_meas"].astype(np.int64), sc["sel_meas"][K - 1]), K
    assert sorted(snaps[s_dead][1]["id"][snaps[s_dead][1]["status"] != 0].tolist()) == [2], "the death happened on the scan before an overlapping one"
    moved = snaps[s_dead + 1][1]
    assert any(len(c) >= 2 and c.max() >= 2 for c in ou.clusters_of(moved)), "a cluster behind the dead slot"
    ovl_seen = 0
    for K in range(1, n + 1):
        uf, ovl, snap = _never_looking(sc, stream, K, model, **kw)
        ou.compare_snapshot(snaps[K], snap, K)
        assert uf == K, "every scan was clustered by the union-find (%d of %d)" % (uf, K)
        ovl_seen = max(ovl_seen, ovl)
        if K == s_dead + 1 and model is None:
            assert ovl >= K - 2, "scan %d, right behind the death, ran as an overlapping launch (%d any-order launches)" % (K, ovl)
    return ovl_seen


def test_tail_behind_a_death_four_state():
    assert _tail_case(None) > 0


def test_tail_behind_a_death_constant_turn():
    from pymht_amd.models import ct
    _tail_case(ct)
