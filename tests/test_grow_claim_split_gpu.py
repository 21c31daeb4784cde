"""GPU: the target workgroup of the grow launch (pymht_amd/csrc/mht_fgrow_dev.h: target_part) with the union-find's claim walking all 64-word
chunks of the association bitset in one round (csrc/mht_uf.h: uf_claim), on the OVERLAPPING path, in a four-state forest and in a
constant-turn forest.  (The file's name is from the first form of the change, which collected the claim's answers behind the counts barrier;
that form was measured and dropped, profiles/claim_split.txt.  The scenes stay: they are where a claim that loses or misfiles an answer shows.)

Scenes, all checked on the CPU by the oracle alone:
  * grow_workgroup_util, unchanged: `planted_scene` (children counts on the wavefront edges of the emission, targets of two passes, every
    target alone in its cluster) and `tail_scene` (a death inside a cluster, the redo of the claim under the alternative epoch);
  * grow_claim_split_util.shared_scene (test_grow_claim_split_scenes_cpu.py): a cluster of three whose middle target (a) has more than 128
    leaves -- two passes, the conflict list is written in the first emitting chunk and `cand` is re-used by the next -- and shares nodes with
    both neighbours, (b) grows more than 192 children from one chunk, so that the last wavefront emits behind its links, (c) shares nodes in
    ring slots of all three 64-word chunks of the 144-word bitset (N = 5, 1 024 measurements per slot: the headline's AW) -- the cluster holds
    only if the one walk finds the nodes of every chunk.
  * A conflict list longer than the constant-turn kernel's 256 entries is NOT planted here: a target would have to meet more than 256
    owner words of other targets, a scene far beyond a few seconds of oracle time.  The overflow path (entries beyond `cap` linked at once)
    runs in tests/test_uf_claim_split_gpu.py at cap 0, 1 and 3.
Every scan of the stream looked at after every scan is held to the LIVE oracle (deaths, clusters, target list, selections); every scan K of a
replay that never looks (a fresh forest per K) is held to the looked-at one (tests/overlap_util.py: header, report rows -- clusters,
selections, leaves kept --, used words, leaf export), every scan clustered by the union-find and the `ovl` counter positive (four-state
build; a constant-turn forest's grow launch is never any-order, its workgroups take the overlapping code path all the same)."""
import numpy as np
import pytest

import grow_claim_split_util as cs
import grow_workgroup_util as gw
import mht_oracle as orc
import overlap_util as ou
from test_grow_workgroup_gpu import _looked_at, _never_looking

pytestmark = pytest.mark.gpu


def _live_oracle(sc, model=None, **kw):
    """the scene's scans through a fresh oracle: per scan the dead ids, the clusters, the target list and the selections"""
    nx = 4 if model is None else 6
    x0 = np.zeros((len(sc["x0"]), nx))
    x0[:, 0:sc["x0"].shape[1]] = sc["x0"]
    o = orc.OracleTracker(sc["period"], sc["lambda_phi"], gw.LAMBDA_NU, P_d=sc["P_d"], N=sc["N"], eta2=gw.ETA2, model=model, **kw)
    P0 = orc.model_P0() if model is None else model.P0
    for x in x0:
        assert o.initiate_target(sc["t0"], x.copy(), P0.copy(), status="preinitialized")
    out = dict(sc, x0=x0, dead=[], clusters=[], sel_meas=[], ids=[])
    for z, t in zip(sc["scans"], sc["times"]):
        info = o.add_scan(t, z)
        out["dead"].append(list(info["dead"]))
        out["clusters"].append([np.asarray(c, dtype=np.int64) for c in o.clusters])
        out["sel_meas"].append(o.selected()["meas"]); out["ids"].append([r.ID for r in o.targets])
    return out


def _case(sc, model=None, **kw):
    """sc carries the live oracle's dead / clusters / ids / sel_meas per scan.  Returns the largest `ovl` counter seen."""
    snaps, stream = _looked_at(sc, model, **kw)
    n = len(sc["scans"])
    for K in range(1, n + 1):
        rows = snaps[K][1]
        assert sorted(rows["id"][rows["status"] != 0].tolist()) == sorted(sc["dead"][K - 1]), K
        cl = ou.clusters_of(rows)
        assert len(cl) == len(sc["clusters"][K - 1]) and all(np.array_equal(a, b) for a, b in zip(cl, sc["clusters"][K - 1])), (K, [c.tolist() for c in cl])
        alive = rows[rows["status"] == 0]
        assert alive["id"].tolist() == sc["ids"][K - 1] and np.array_equal(alive["sel_meas"].astype(np.int64), sc["sel_meas"][K - 1]), K
    ovl_seen = 0
    for K in range(1, n + 1):
        uf, ovl, snap = _never_looking(sc, stream, K, model, **kw)
        ou.compare_snapshot(snaps[K], snap, K)
        assert uf == K, "every scan was clustered by the union-find (%d of %d)" % (uf, K)
        ovl_seen = max(ovl_seen, ovl)
    return ovl_seen, snaps


def test_shared_cluster_four_state():
    sc = cs.shared_scene()
    cond = cs.shared_conditions(sc)
    ovl, snaps = _case(sc)
    assert ovl > 0, "no grow launch overlapped the previous scan's ILP launch"
    for K in cond["two_pass"] + cond["last_wave"]:      # the device grew what the oracle grew: leaves in, children out
        assert snaps[K][0][3] == sum(sc["leaves_in"][K - 1]) and snaps[K][0][4] == sum(sc["children"][K - 1]), (K, snaps[K][0])


def test_shared_cluster_constant_turn():
    from pymht_amd.models import ct
    sc = cs.shared_scene(model=ct)
    cs.shared_conditions(sc)
    _case(sc, ct)


def test_planted_scene_four_state():
    sc = _live_oracle(gw.planted_scene())
    assert all(len(c) == 1 for cl in sc["clusters"] for c in cl) and not any(sc["dead"])
    ovl, snaps = _case(sc)
    assert ovl > 0
    for K in range(1, len(sc["scans"]) + 1):
        assert snaps[K][1]["n_leaves"].tolist() == [p[K - 1] for p in gw.PLANS], K


def test_planted_scene_constant_turn():
    from pymht_amd.models import ct
    _case(_live_oracle(gw.planted_scene(), ct), ct)


def test_tail_scene_four_state():
    sc = gw.tail_scene()
    gw.tail_conditions(sc)
    ovl, _ = _case(sc, position=np.array([0.0, 0.0]), radarRange=sc["range"])
    assert ovl > 0


def test_tail_scene_constant_turn():
    from pymht_amd.models import ct
    sc = gw.tail_scene(model=ct)
    gw.tail_conditions(sc)
    _case(sc, ct, position=np.array([0.0, 0.0]), radarRange=sc["range"])
