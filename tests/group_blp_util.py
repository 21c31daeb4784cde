"""Shared by tests/test_blp_prologue_gpu.py, tests/test_group_blp_cpu.py and tests/test_group_blp_gpu.py.

Two things live here.  The recipe for clusters of a chosen size: `_scene` places stationary targets in runs on a line, `_tracker` plants
them through mht_forest_add_targets without its neighbour test, `_rd` reads a named table through mht_forest_debug_read.  And the host
side of a multi-target cluster's 0-1 ILP: `Cluster` is the instance in the form oracle/mht_oracle.py: solve_blp_exact takes -- rebuilt
from the tables read back after a step (`read_tables`, `clusters_of`) or from an instance the oracle recorded (`from_instance`) -- with
`feasible`, `objective` and `light_verdict`, the light pass of a sector group (csrc/mht_blp.hip: blp_light) restated in NumPy.

NumPy only at import; the library is imported inside the functions that talk to the device."""
import ctypes as C
import os

import numpy as np

PERIOD, P_D, LAMBDA_PHI, N_SCANS = 2.5, 0.9, 1.0e-5, 3
SPACING, GAP, ROW, WIDTH = 12.0, 60.0, 80.0, 1500.0
LIGHT_MAXK = 8                 # csrc/mht_blp.hip
CERTIFIED = 1                  # include/mht_amd.h: MHT_BLP_CERTIFIED
# a clash pair's own detections lie CLASH_OFFSET off their targets, across the line: further than the 6 m to the link plot between the two,
# which is thereby the cheapest hit of both (the cost of a hit grows with its distance, mht_oracle.kf_nllr) -- and still inside the gate:
# 7.5^2 / S < 5.99 for every innovation variance S above 9.4 m^2, and S is never below R + Q = 6.25 + 9.77
CLASH_OFFSET = 7.5


def _runs_mixed(nT):
    """mostly lone targets, pairs and triples between them, cut off at nT targets"""
    pattern, out, k = (1, 1, 2, 1, 3, 1, 1, 2, 1, 1, 1, 4), [], 0
    while sum(out) < nT:
        out.append(min(pattern[k % len(pattern)], nT - sum(out)))
        k += 1
    return out


def _scene(runs, seed=5446, n_scans=N_SCANS, clash=(), gap=GAP, width=WIDTH):
    """clash: indices into `runs`; the first two neighbours of those runs are a clash pair (see CLASH_OFFSET) on every scan.
    gap, width: GAP keeps the runs apart for three scans -- a hypothesis of four misses in a row has a gate of some 70 m, which a scene
    of four scans and more has to allow for between its runs and between its rows."""
    rng = np.random.default_rng(seed)
    pos, links, off, x, y = [], [], [], 0.0, 0.0
    for i, K in enumerate(runs):
        if x + K * SPACING > width:
            x, y = 0.0, y + ROW
        for m in range(K):
            pos.append((x, y))
            off.append((0.0, (CLASH_OFFSET if m == 0 else -CLASH_OFFSET) if (i in clash and K >= 2 and m < 2) else 0.0))
            if m:
                links.append((x - 0.5 * SPACING, y))
            x += SPACING
        x += gap - SPACING
    pos, links = np.array(pos, dtype=np.float64).reshape(-1, 2), np.array(links, dtype=np.float64).reshape(-1, 2)
    own = pos + np.array(off, dtype=np.float64).reshape(-1, 2)
    x0 = np.concatenate([pos, np.zeros_like(pos)], axis=1)
    scans = []
    for _ in range(n_scans):
        z = np.concatenate([own + rng.normal(0.0, 0.3, size=pos.shape), links + rng.normal(0.0, 0.3, size=links.shape)], axis=0)
        rng.shuffle(z, axis=0)
        scans.append(np.ascontiguousarray(z, dtype=np.float32).reshape(-1, 2))
    return x0, scans


def _tracker(x0, env, mirror=False, **kw):
    """mirror: the host tables of the drop-in Tracker are told about the planted targets as Tracker._add_targets tells them, so that the
    tracker can be stepped through addMeasurementList / SectorGroup.addMeasurementLists and not only through the C ABI"""
    from pymht_amd import _lib
    from pymht_amd.tracker import Tracker
    from pymht_amd.models import pv
    names = ("MHT_BLP_GENERIC", "MHT_NO_UF", "MHT_BLP_GRID")
    old = {n: os.environ.pop(n, None) for n in names}
    os.environ.update(env)      # (read when the forest is created)
    try:
        args = dict(P_d=P_D, N=3, eta2=5.99, useInitiator=False, maxTargets=2048, maxNodes=1 << 18, maxMeasurements=2048)
        args.update(kw)
        trk = Tracker(pv, PERIOD, LAMBDA_PHI, 1e-4, **args)
        n = len(x0)
        xs = np.ascontiguousarray(x0, dtype=np.float64)
        P0 = np.ascontiguousarray(np.tile(np.asarray(pv.P0, dtype=np.float32).reshape(1, 16), (n, 1)))
        flags, pd, meas = np.zeros(n, dtype=np.uint8), np.full(n, P_D, dtype=np.float64), np.zeros(n, dtype=np.int32)
        acc, ids = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(trk._lib.mht_forest_add_targets(trk._ctx.handle, n, p(xs), p(P0), p(flags), p(pd), p(meas), 0, p(acc), p(ids)))
        assert acc.all()
        if mirror:
            rows = np.zeros(n, dtype=trk._REPORT_DTYPE)
            rows["id"], rows["root_scan"], rows["root_node"], rows["root_meas"], rows["root_x"] = ids, 0, -1, meas, xs
            trk._tbl_ = rows
            for i in range(n):
                trk._birth[int(ids[i])] = (0.0, 0, xs[i].copy(), pv.P0, None, None, "preinitialized")
            trk._leaf_time, trk.trackIdCounter = 0.0, int(ids.max()) + 1
    finally:
        for n in names:
            os.environ.pop(n, None)
            if old[n] is not None:
                os.environ[n] = old[n]
    return trk


def _rd(trk, name, n, dtype=np.int32, first=0):
    """n elements of the named table from element `first` on"""
    from pymht_amd import _lib
    a = np.zeros(max(int(n), 1), dtype=dtype)
    if first:
        name = "%s@%d" % (name, int(first) * a.itemsize)
    _lib.check(trk._lib.mht_forest_debug_read(trk._ctx.handle, name.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes))
    return a[:int(n)]


# ---- the host side of a cluster's ILP ------------------------------------------------------------------------------------------------
class Cluster:
    """cols[h]: the rows of column h (ints, 0 .. nR-1); sizes[k]: columns of member k, in member order; cost[h]: float64.  Columns are
    numbered inside the cluster; `first[k]` is member k's first column, `node0[k]` the node index of it in the tables it was read from
    (-1: none), `c` the cluster's index there and `members` its targets."""

    def __init__(self, cols, sizes, cost, c=-1, members=None, node0=None):
        self.cols = [np.asarray(r, dtype=np.int64).reshape(-1) for r in cols]
        self.sizes = [int(s) for s in sizes]
        self.cost = np.asarray(cost, dtype=np.float64).reshape(-1)
        assert len(self.cols) == len(self.cost) == sum(self.sizes)
        self.first = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.K, self.nH = len(self.sizes), len(self.cols)
        self.c, self.members = c, (list(range(self.K)) if members is None else [int(t) for t in members])
        self.node0 = [-1] * self.K if node0 is None else [int(v) for v in node0]

    def key(self):
        flat = np.concatenate([np.append(r, -1) for r in self.cols]) if self.nH else np.zeros(0, np.int64)
        return (tuple(self.sizes), flat.tobytes(), self.cost.tobytes())

    def instance(self):
        """(cols, sizes, cost) as solve_blp_exact takes them"""
        return [r.tolist() for r in self.cols], list(self.sizes), self.cost.copy()


def from_instance(inst):
    """an instance OracleTracker.ilp_recorder kept"""
    return Cluster(inst["cols"], inst["sizes"], inst["cost"])


def feasible(cl, sel):
    """one column per member, inside that member's range, and no row used twice"""
    sel = [int(h) for h in sel]
    if len(sel) != cl.K:
        return False
    used = set()
    for k, h in enumerate(sel):
        if not cl.first[k] <= h < cl.first[k + 1]:
            return False
        for r in cl.cols[h].tolist():
            if r in used:
                return False
            used.add(r)
    return True


def objective(cl, sel):
    return float(np.sum(cl.cost[np.asarray(sel, dtype=np.int64)], dtype=np.float64))


def light_verdict(cl):
    """What blp_light must do with the cluster: ("deferred", None) for more than LIGHT_MAXK members, a member without a column, or two
    members whose cheapest columns (lowest index among equals) share a row; ("finished", those minimisers) otherwise."""
    if cl.K > LIGHT_MAXK or min(cl.sizes) == 0:
        return "deferred", None
    mins = [int(cl.first[k] + np.argmin(cl.cost[cl.first[k]:cl.first[k + 1]])) for k in range(cl.K)]
    seen = set()
    for h in mins:
        rows = set(cl.cols[h].tolist())
        if rows & seen:
            return "deferred", None
        seen |= rows
    return "finished", mins


def read_tables(trk):
    """The cluster tables, the selections and the columns of the scan just stepped, from the tracker's own context."""
    cnt = _rd(trk, "cl_counts", 8).copy()
    nC = int(cnt[0])
    t = dict(cl_counts=cnt, cl_ptr=_rd(trk, "cl_ptr", nC + 1).copy())
    nT = int(t["cl_ptr"][-1]) if nC else 0
    for name, n in (("cl_members", nT), ("tchild", nT), ("tcend", nT), ("sel", nT), ("cl_status", nC), ("cl_iters", nC)):
        t[name] = _rd(trk, name, n).copy()
    lo, hi = (int(t["tchild"].min()), int(t["tcend"].max())) if nT else (0, 0)
    t["node_lo"] = lo
    t["cost"] = _rd(trk, "cost", hi - lo, np.float64, lo).copy()
    t["path"] = _rd(trk, "path", (hi - lo) * 8, np.int32, lo * 8).copy().reshape(-1, 8)
    return t


def clusters_of(t):
    """every multi-target cluster of the tables: columns = the members' child ranges tchild[t] .. tcend[t], rows = the non-negative entries
    of each column's 8-int path record (renumbered 0 .. nR-1 in ascending order)"""
    out = []
    ptr, lo = t["cl_ptr"], t["node_lo"]
    for c in range(len(ptr) - 1):
        members = t["cl_members"][ptr[c]:ptr[c + 1]]
        if len(members) < 2:
            continue
        nodes = np.concatenate([np.arange(t["tchild"][m], t["tcend"][m], dtype=np.int64) for m in members])
        rec = t["path"][nodes - lo]
        ids = np.unique(rec[rec >= 0])
        cols = [np.searchsorted(ids, r[r >= 0]) for r in rec]
        out.append(Cluster(cols, [int(t["tcend"][m] - t["tchild"][m]) for m in members], t["cost"][nodes - lo], c=c, members=members,
                           node0=[int(t["tchild"][m]) for m in members]))
    return out


def selection(t, cl):
    """the read-back selection of the cluster's members, as columns of the cluster"""
    return [int(t["sel"][m]) - n0 + int(f) for m, n0, f in zip(cl.members, cl.node0, cl.first[:-1])]
