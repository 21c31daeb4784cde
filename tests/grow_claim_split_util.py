"""Scene of tests/test_grow_claim_split_gpu.py, built with the CPU oracle alone (self-test: test_grow_claim_split_scenes_cpu.py).

`shared_scene`: three targets in a row, 26 m apart, and one far away.  Every scan brings one measurement near each target and one between two
neighbours -- between the first two in odd scans, between the last two in even ones -- so the middle target gates two or three measurements per
leaf and scan, its tree fills the N-scan window, and the three stay one cluster through nodes of EVERY scan of the window.  What the grow
launch's target workgroup meets there (csrc/mht_fgrow_dev.h: target_part; csrc/mht_uf.h: uf_claim, one walk over all chunks of the bitset):
  (a) a target with more than 128 leaves -- the chunk loop runs twice -- that shares nodes with two neighbours;
  (b) a chunk of at most 128 leaves with more than 192 children: the last wavefront has a share of the emission behind its links;
  (c) shared nodes in three ring slots that lie in three different 64-word chunks of the association bitset (N = 5, 1 024 measurements per
      slot: 9 slots of 16 words, AW = 144 -- chunks are slots 0-3, 4-7 and 8).

Nothing here imports the GPU side."""
import numpy as np

import mht_oracle as orc

PERIOD, LAMBDA_PHI, LAMBDA_NU, ETA2 = 2.5, 1e-6, 1e-4, 5.99
X0 = np.array([
    [0.0, 0.0, 0.0, 0.0],
    [26.0, 0.0, 0.0, 0.0],        # the middle one
    [52.0, 0.0, 0.0, 0.0],
    [5000.0, 3000.0, 3.0, -2.0],  # alone
])
GROUP = [0, 1, 2]
CAP, LAST_WAVE_FROM = 128, 192      # leaves per chunk; the last wavefront emits children 192 .. 255 of a chunk
SLOT_WORDS, RING_EXTRA = 16, 4      # 1 024 measurements per ring slot; the ring holds N + 4 scans


def shared_scene(n_scans=10, N=5, P_d=0.9, seed=4, model=None):
    """Returns the scene and what the oracle saw: per scan the leaves every target went in with and came out with, the association sets the
    clustering ran on, the clusters, the dead ids, the selections."""
    rng = np.random.default_rng(seed)
    nx = 4 if model is None else 6
    x0 = np.zeros((len(X0), nx))
    x0[:, 0:4] = X0
    o = orc.OracleTracker(PERIOD, LAMBDA_PHI, LAMBDA_NU, P_d=P_d, N=N, eta2=ETA2, model=model)
    P0 = orc.model_P0() if model is None else model.P0
    for x in x0:
        assert o.initiate_target(0.0, x.copy(), P0.copy(), status="preinitialized")
    seen = []
    plain = orc.find_clusters

    def spy(sets):      # (the sets of the scan: the window's nodes and this scan's hits, before anything is pruned)
        seen.append([set(s) for s in sets])
        return plain(sets)
    scans, times, leaves_in, children, assoc, clusters, dead, sel_meas, ids = [], [], [], [], [], [], [], [], []
    grown = {}
    grow = o._grow

    def counted(ti, *args, **kw):      # (children a target grows in the scan: 1 missed detection per leaf + its gated pairs)
        l, g = grow(ti, *args, **kw)
        grown[ti] = l + g
        return l, g
    o._grow = counted
    orc.find_clusters = spy
    try:
        for k in range(n_scans):
            t = (k + 1) * PERIOD
            pos = X0[:, 0:2] + X0[:, 2:4] * t
            z = [pos[i] + rng.normal(0.0, 0.7, size=2) for i in range(len(pos))]
            a, b = (0, 1) if k % 2 == 0 else (1, 2)
            z.append(0.5 * (pos[a] + pos[b]) + rng.normal(0.0, 0.7, size=2))
            z = np.array(z, dtype=np.float32)[rng.permutation(len(z))]
            leaves_in.append([len(r.leaves()) for r in o.targets])
            n_seen = len(seen)
            info = o.add_scan(t, z)
            assert len(seen) == n_seen + 1
            children.append([grown[i] for i in range(len(leaves_in[-1]))])
            scans.append(z); times.append(t); dead.append(list(info["dead"])); assoc.append(seen[-1])
            clusters.append([np.asarray(c, dtype=np.int64) for c in o.clusters])
            sel_meas.append(o.selected()["meas"]); ids.append([r.ID for r in o.targets])
    finally:
        orc.find_clusters = plain
    return dict(x0=x0, scans=scans, times=times, N=N, P_d=P_d, period=PERIOD, lambda_phi=LAMBDA_PHI, t0=0.0,
                leaves_in=leaves_in, children=children, assoc=assoc, clusters=clusters, dead=dead, sel_meas=sel_meas, ids=ids)


def chunks_of_shared_nodes(sets, members, N, offset):
    """64-word chunks of the association bitset in which two members of a cluster share a node; the scan numbered s sits in ring slot
    (s - offset) mod (N + 4)"""
    R, out = N + RING_EXTRA, set()
    for i, a in enumerate(members):
        for b in members[i + 1:]:
            for (s, _m) in sets[a] & sets[b]:
                out.add((((s - offset) % R) * SLOT_WORDS) // 64)
    return out


def shared_conditions(sc):
    """{"two_pass": scans (1-based) of (a), "last_wave": scans of (b), "three_chunks": scans of (c)}, each checked to be there"""
    assert not any(sc["dead"]), "nobody dies: slots are indices throughout"
    a, b, c = [], [], []
    for k in range(len(sc["scans"])):
        together = any(set(GROUP) <= set(cl.tolist()) for cl in sc["clusters"][k])
        sets = sc["assoc"][k]
        if together and sc["leaves_in"][k][1] > CAP and sets[0] & sets[1] and sets[1] & sets[2]:
            a.append(k + 1)
        if together and any(sc["leaves_in"][k][t] <= CAP and sc["children"][k][t] > LAST_WAVE_FROM for t in GROUP):
            b.append(k + 1)
        if together and all(chunks_of_shared_nodes(sets, GROUP, sc["N"], off) == {0, 1, 2} for off in (0, 1)):
            c.append(k + 1)      # (whichever of the two the forest's scan counter starts at)
    assert a, "a target of two passes that shares nodes with two neighbours"
    assert b, "a single chunk with more than 192 children in a cluster"
    assert c, "shared nodes in all three 64-word chunks of the bitset"
    return dict(two_pass=a, last_wave=b, three_chunks=c)
