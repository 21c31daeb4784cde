"""Scenes of tests/test_grow_workgroup_gpu.py, built with the CPU oracle alone (self-test: test_grow_workgroup_scenes_cpu.py).

`planted_scene`: targets far from each other, each with a PLAN -- the number of children (1 missed detection + hits per leaf, summed over its
leaves) it shall have at every scan.  The measurements of a scan are picked from random candidates around the target's predicted leaves by
a subset sum over the candidates' gate counts (the oracle's own gating), so the plan is met exactly; while the N-scan window has not filled
(scan <= N) nothing is pruned and a target's children of scan k are its leaves of scan k + 1 and the `n_leaves` of its report row.

`tail_scene`: a target leaves the radar's range -- and dies -- in the middle of a group of targets that share measurements, so that from the
next scan on compacted indices and slots differ and the clustering is decided by indices behind the dead slot.

Nothing here imports the GPU side."""
import numpy as np

import mht_oracle as orc

PERIOD, LAMBDA_PHI, LAMBDA_NU, ETA2 = 2.5, 1e-6, 1e-4, 5.99

# plans per target (N = 5, five scans): children counts on the edges of the emission's wavefronts (63 / 64 / 65, 127 / 128 / 129, 192 / 193),
# leaf counts on the edges of the count phase (1, 63 / 64 / 65 leaves, 127 / 128 in one pass, 129 / 192 / 193 in two), scans without any hit
PLANS = (
    (7, 63, 127, 192, 192),      # leaves 1, 7, 63, 127, 192 (two passes, no hit at all)
    (8, 64, 128, 193, 200),      # leaves 1, 8, 64, 128, 193 (two passes)
    (5, 65, 129, 140, 150),      # leaves 1, 5, 65, 129 (two passes), 140
    (1, 4, 4, 9, 30),            # a single leaf without a hit, a single leaf with hits, four leaves without a hit
)


def _subset(g, need, first):
    """Indices of candidates whose gate counts g sum to `need`, `first` among them (None: no such subset)."""
    if need == 0:
        return []
    head = [int(first)]
    if g[first] > need:      # (fewer pairs wanted than leaves gate the middle: without it)
        g = g.copy(); g[first] = 0; head = []
    rest = need - int(g[first])
    reach = {0: []}
    for j in np.argsort(-g):      # (large counts first: few measurements)
        if j == first or g[j] == 0:
            continue
        for s in sorted(reach, reverse=True):
            t = s + int(g[j])
            if t <= rest and t not in reach:
                reach[t] = reach[s] + [int(j)]
        if rest in reach:
            break
    return None if rest not in reach else head + reach[rest]


def planted_scene(plans=PLANS, N=5, P_d=0.9, seed=11, spacing=20000.0):
    """Returns dict(x0, scans, times, N, P_d, period, lambda_phi, plans, oracle rows per scan): len(plans) targets `spacing` metres apart."""
    rng = np.random.default_rng(seed)
    n_scans = len(plans[0])
    x0 = np.array([[spacing * i, 100.0 * i, 2.0, -1.0] for i in range(len(plans))], dtype=np.float64)
    o = orc.OracleTracker(PERIOD, LAMBDA_PHI, LAMBDA_NU, P_d=P_d, N=N, eta2=ETA2)
    for x in x0:
        assert o.initiate_target(0.0, x.copy(), orc.model_P0(), status="preinitialized")
    scans, times, leaves_in, children = [], [], [], []
    for k in range(n_scans):
        zs, lin = [], []
        for ti, plan in enumerate(plans):
            leaves = o.targets[ti].leaves()
            L, need = len(leaves), plan[k] - len(leaves)
            assert need >= 0, "target %d scan %d: %d leaves, %d children wanted" % (ti, k + 1, L, plan[k])
            lin.append(L)
            x = np.array([l.x for l in leaves], ndmin=2)
            P = np.array([l.P for l in leaves], ndmin=3)
            zh = o.A.astype(np.float64).dot(x.astype(np.float64).T).T[:, 0:2]
            for attempt in range(20):
                spread = rng.choice([1.0, 3.0, 8.0, 20.0], size=300)[:, None]
                cand = (zh[rng.integers(0, L, size=300)] + rng.normal(0.0, 1.0, size=(300, 2)) * spread).astype(np.float32)
                cand[0] = zh.mean(axis=0).astype(np.float32)      # (a measurement in the middle: the best leaf keeps a good score)
                r = orc.process_leaves(o.A, o.Q, o.C, o.R, ETA2, o.lambda_ex, x, P, [l.P_d for l in leaves], cand)
                g = np.zeros(len(cand), dtype=np.int64)
                for idx in r["idx"]:
                    g[idx] += 1
                pick = _subset(g, need, 0)
                if pick is not None:
                    break
            assert pick is not None, "target %d scan %d: no measurement set gives %d gated pairs" % (ti, k + 1, need)
            zs.append(cand[sorted(pick)].reshape(-1, 2))
        z = np.concatenate(zs, axis=0).astype(np.float32) if sum(len(a) for a in zs) else np.zeros((0, 2), np.float32)
        info = o.add_scan((k + 1) * PERIOD, z)
        assert len(o.targets) == len(plans) and not info["dead"], "scan %d: a planted target died" % (k + 1)
        got = [len(r.leaves()) for r in o.targets]
        assert got == [p[k] for p in plans], "scan %d: children %s against the plan" % (k + 1, got)
        assert info["L"] == sum(lin) and info["L"] + info["G"] == sum(got)
        scans.append(z); times.append((k + 1) * PERIOD); leaves_in.append(lin); children.append(got)
    return dict(x0=x0, scans=scans, times=times, N=N, P_d=P_d, period=PERIOD, lambda_phi=LAMBDA_PHI, plans=plans, t0=0.0,
                leaves_in=leaves_in, children=children)


# ---- the tail: a death in the middle of a group ---------------------------------------------------------------------------------------------
RANGE = 1000.0
TAIL_X0 = np.array([
    [-500.0, -300.0, 0.0, 0.0],      # 0: alone
    [900.0, 0.0, 0.0, 0.0],          # 1: the group (26 m apart: closer roots are merged at their admission) ...
    [926.0, 0.0, 12.0, 0.0],         # 2: ... the one that leaves the range (30 m per scan)
    [952.0, 0.0, 0.0, 0.0],          # 3
    [978.0, 0.0, 0.0, 0.0],          # 4
    [400.0, 700.0, 0.0, 0.0],        # 5: alone
    [965.0, -26.0, 0.0, 0.0],        # 6: the group again, behind a slot that is not in it
    [-200.0, 600.0, 0.0, 0.0],       # 7: alone
])


def tail_scene(n_scans=7, N=3, P_d=0.9, seed=3, model=None):
    """Eight targets, five of them 14 m apart near the edge of the radar's range, one of those moving out of it.  Every scan: one measurement per
    target near its true position and one between every two neighbours of the group.  model: None (pv, four states) or pymht_amd.models.ct
    (six states: turn rate and its derivative 0).  Returns the scene and what the oracle saw: per scan the dead ids, the cluster lists,
    the selections."""
    rng = np.random.default_rng(seed)
    nx = 4 if model is None else 6
    x0 = np.zeros((len(TAIL_X0), nx))
    x0[:, 0:4] = TAIL_X0
    o = orc.OracleTracker(PERIOD, LAMBDA_PHI, LAMBDA_NU, P_d=P_d, N=N, eta2=ETA2, position=(0.0, 0.0), radarRange=RANGE, model=model)
    P0 = orc.model_P0() if model is None else model.P0
    for x in x0:
        assert o.initiate_target(0.0, x.copy(), P0.copy(), status="preinitialized")
    group = [1, 2, 3, 4, 6]
    scans, times, dead, clusters, sel_meas, ids = [], [], [], [], [], []
    for k in range(n_scans):
        t = (k + 1) * PERIOD
        pos = TAIL_X0[:, 0:2] + TAIL_X0[:, 2:4] * t
        z = [pos[i] + rng.normal(0.0, 0.7, size=2) for i in range(len(pos))]
        gp = pos[group][np.argsort(pos[group][:, 0])]
        z += [0.5 * (gp[i] + gp[i + 1]) + rng.normal(0.0, 0.7, size=2) for i in range(len(gp) - 1)]
        z = np.array(z, dtype=np.float32)[rng.permutation(len(z))]
        info = o.add_scan(t, z)
        scans.append(z); times.append(t); dead.append(list(info["dead"]))
        clusters.append([np.asarray(c, dtype=np.int64) for c in o.clusters])
        sel_meas.append(o.selected()["meas"]); ids.append([r.ID for r in o.targets])
    return dict(x0=x0, scans=scans, times=times, N=N, P_d=P_d, period=PERIOD, lambda_phi=LAMBDA_PHI, t0=0.0, range=RANGE,
                dead=dead, clusters=clusters, sel_meas=sel_meas, ids=ids)


def tail_conditions(sc):
    """The scan (1-based) in which target 2 dies, checked for what the tail test needs: it dies alone, not in the first two scans (the scan
    behind it must be an overlapping one), as a member of a cluster with members on both sides of its slot, and the scan BEHIND its death has a
    cluster of at least two targets whose slots lie behind the dead one (their compacted indices differ from their slots)."""
    died = [k + 1 for k, d in enumerate(sc["dead"]) if d]
    assert died and sc["dead"][died[0] - 1] == [2], "target 2 dies first and alone: %s" % sc["dead"]
    s = died[0]
    assert 3 <= s < len(sc["scans"]), "the death (scan %d) has overlapping scans on both sides" % s
    mine = [c for c in sc["clusters"][s - 1] if 2 in c.tolist()][0]      # (clusters of scan s: indices into the list the scan ran on = slots)
    assert mine.min() < 2 < mine.max(), "target 2 sits inside its cluster: %s" % mine
    after = [c for c in sc["clusters"][s] if len(c) >= 2 and c.max() >= 2]      # (scan s + 1: compacted indices; index >= 2 = slot + 1)
    assert after, "a cluster behind the dead slot in scan %d: %s" % (s + 1, sc["clusters"][s])
    return s
