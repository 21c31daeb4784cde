"""Helpers of the every-scan tests of the OVERLAPPING scan path (tests/test_overlap_every_scan_gpu.py; self-test: test_overlap_util_cpu.py).

The overlapping path -- the raw `mht_forest_step` replay and the streamed `Tracker.addMeasurementList`, where nobody looks between the scans,
the scan's commit rides in the next grow launch and that launch runs any-order next to the previous scan's ILP launch (FDyn::ovl) -- cannot
be looked at scan by scan: every look flushes the deferred commit.  What CAN be kept without looking:
  * the drop-in API folds every scan's report (rows, births) into its host mirror two scans late: `Recording.attach` wraps the two fold
    functions and keeps a copy of what they are handed;
  * the raw ABI has no such report, so it is observed at stop points (`stop_set`): a fresh forest per stop, stepped without a look, read at the stop.
The comparers raise AssertionError naming the scan, the field and the first differing target; node indices (`sel_node`, `root_node`, a
leaf's `node`) are handles -- a target's children take their block of the node index space with an atomic -- and are never compared.

Nothing here imports the GPU side at module level (the CPU self-test imports this file)."""
import ctypes as C

import numpy as np

HANDLES = ("sel_node", "root_node")      # report fields that are handles
LEAF_HANDLES = ("node",)
HEADER = ("scan", "n_targets", "n_alive", "n_leaves_in", "n_children", "n_leaves_out", "n_clusters", "n_ilp")
STOPS_TOP = (59, 60, 61, 63, 64, 65, 128, 200)      # the `s_table - k < 60` bound of targets_ub, the rings of 64 (births_after / bhint), two long chains


def stop_set(N, n_scans, top=STOPS_TOP):
    """Stop points of a raw replay with window N (ring R = N + 4): the start of a chain, the window filling, the ring's wrap (once and twice), then `top`."""
    R = N + 4
    s = {1, 2, 3, N, N + 1, R - 1, R, R + 1, 2 * R + 1} | set(top)
    return sorted(k for k in s if 1 <= k <= n_scans)


def group_stop_set(N, n_scans):
    R = N + 4
    return sorted(k for k in {1, 2, N + 1, R, R + 1, n_scans} if 1 <= k <= n_scans)


# ---- recordings of the drop-in API ----------------------------------------------------------------------------------------------------------
class Recording:
    """rows[s] / births[s]: the report rows and the ADMITTED births of scan s (1-based) as the tracker folded them."""

    def __init__(self):
        self.rows, self.births = {}, {}

    def attach(self, trk):
        """Wraps `Tracker._apply_report` and `Tracker._apply_births` of this tracker object: copies, nothing is looked at."""
        rep0, born0 = trk._apply_report, trk._apply_births

        def apply_report(recs, scanTime, scanNumber, z, all_alive=None):
            self.rows[int(scanNumber)] = np.array(recs)
            return rep0(recs, scanTime, scanNumber, z, all_alive)

        def apply_births(births, scanTime, scanNumber, z_unused):
            self.births[int(scanNumber)] = np.array(births[births["id"] >= 0])
            return born0(births, scanTime, scanNumber, z_unused)

        trk._apply_report, trk._apply_births = apply_report, apply_births
        return self

    def scans(self):
        return sorted(self.rows)

    def births_of(self, s):
        return self.births.get(s)      # (None: the scan gave birth to nothing)


def ids_behind(rows, births):
    """The target list behind a scan: surviving rows, then the admitted births, in table order."""
    alive = rows["id"][rows["status"] == 0]
    return np.concatenate([alive, births["id"]]).astype(np.int64) if births is not None and len(births) else alive.astype(np.int64)


def clusters_of(rows):
    """The cluster lists of a scan from the rows' `cluster` labels (indices into the target list the scan ran on), as `Tracker.__clusterList__` builds them."""
    labels = rows["cluster"]
    return [np.where(labels == lab)[0] for lab in np.unique(labels)]


# ---- comparers ------------------------------------------------------------------------------------------------------------------------------
def _first_bad(a, b):
    a, b = np.asarray(a), np.asarray(b)
    bad = a != b
    if bad.ndim > 1:
        bad = bad.reshape(len(bad), -1).any(axis=1)
    return int(np.flatnonzero(bad)[0])


def compare_rows(a, b, scan, what="report rows", skip=HANDLES):
    if len(a) != len(b):
        raise AssertionError("scan %d: %s: %d rows against %d" % (scan, what, len(a), len(b)))
    for name in a.dtype.names:
        if name in skip or np.array_equal(a[name], b[name]):
            continue
        i = _first_bad(a[name], b[name])
        raise AssertionError("scan %d: %s: field %r differs in %d rows, first at row %d (target id %d): %r against %r" % (
            scan, what, name, int(np.count_nonzero(np.asarray(a[name] != b[name]).reshape(len(a), -1).any(axis=1))), i, int(a["id"][i]),
            a[name][i].tolist(), b[name][i].tolist()))


def compare_births(a, b, scan):
    if a is None or b is None:
        if (a is None or len(a) == 0) and (b is None or len(b) == 0):
            return
        raise AssertionError("scan %d: births: %d against %d" % (scan, 0 if a is None else len(a), 0 if b is None else len(b)))
    compare_rows(a, b, scan, what="admitted births", skip=())


def compare_used(a, b, scan):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    if a.shape != b.shape:
        raise AssertionError("scan %d: used-measurement words: %d against %d" % (scan, len(a), len(b)))
    if not np.array_equal(a, b):
        w = _first_bad(a, b)
        raise AssertionError("scan %d: used-measurement words differ, first in word %d: %#x against %#x" % (scan, w, int(a[w]), int(b[w])))


def compare_leaves(a, b, scan, skip=LEAF_HANDLES, keys=None):
    for key in (keys if keys is not None else sorted(a)):
        if key in skip:
            continue
        if key not in b:
            raise AssertionError("scan %d: leaves: key %r is missing" % (scan, key))
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.shape != y.shape:
            raise AssertionError("scan %d: leaves: %r has %d entries against %d" % (scan, key, len(x), len(y)))
        if not np.array_equal(x, y):
            i = _first_bad(x, y)
            raise AssertionError("scan %d: leaves: %r differs first at leaf %d (target id %d): %r against %r" % (
                scan, key, i, int(np.asarray(a["ID"])[i]), x[i].tolist(), y[i].tolist()))


def compare_header(a, b, scan):
    if tuple(a) != tuple(b):
        diff = ["%s %d against %d" % (n, x, y) for n, x, y in zip(HEADER, a, b) if x != y]
        raise AssertionError("scan %d: report header: %s" % (scan, ", ".join(diff)))


def compare_stats(la, lb):
    """Two `Tracker.scanStatsLog` lists, scan by scan, every key."""
    if len(la) != len(lb):
        raise AssertionError("scan logs of %d and %d scans" % (len(la), len(lb)))
    for s, (a, b) in enumerate(zip(la, lb), start=1):
        if sorted(a) != sorted(b):
            raise AssertionError("scan %d: scan log keys %s against %s" % (s, sorted(a), sorted(b)))
        for k in a:
            if not np.array_equal(np.asarray(a[k]), np.asarray(b[k])):
                raise AssertionError("scan %d: scan log %r: %r against %r" % (s, k, np.asarray(a[k]).tolist(), np.asarray(b[k]).tolist()))


def compare_recordings(A, B):
    """Two recordings of one stream, scan by scan in order: every report field but the handles, and the admitted births."""
    if A.scans() != B.scans():
        raise AssertionError("recorded scans %d..%d (%d) against %d..%d (%d)" % (
            min(A.scans() or [0]), max(A.scans() or [0]), len(A.scans()), min(B.scans() or [0]), max(B.scans() or [0]), len(B.scans())))
    for s in A.scans():
        compare_rows(A.rows[s], B.rows[s], s)
        compare_births(A.births_of(s), B.births_of(s), s)


def compare_snapshot(ref, got, scan, leaf_keys=None):
    """A stop point of a raw replay: (header tuple, rows, used words, leaf batch) as in test_deferred_commit_equals_immediate_commit."""
    compare_header(ref[0], got[0], scan)
    compare_rows(ref[1], got[1], scan)
    compare_used(ref[2], got[2], scan)
    compare_leaves(ref[3], got[3], scan, keys=leaf_keys)


def check_scan_against_trace(g, s, rows, births, stats, score_atol):
    """Scan s (1-based) of a recording against what a fixture recorded from the reference holds for it (fixture index s - 1): gating counts,
    unused measurements, the target list behind the scan, the selections (survivors, then the newborn roots as the reference lists them),
    terminations, births and the cluster lists."""
    p = "s%02d_" % (s - 1)

    def need(ok, what):
        if not ok:
            raise AssertionError("scan %d (fixture index %d): %s" % (s, s - 1, what))

    need([stats["L"], stats["G"], stats["M"]] == g[p + "LGM"].tolist(), "L/G/M %s against %s" % ([stats["L"], stats["G"], stats["M"]], g[p + "LGM"].tolist()))
    need(np.array_equal(stats["unused"], g[p + "unused"]), "unused measurements")
    alive = rows[rows["status"] == 0]
    nb = 0 if births is None else len(births)
    ids = ids_behind(rows, births)
    need(np.array_equal(ids, g[p + "ids"]), "target list behind the scan")
    need(stats["nTargets"] == len(ids), "nTargets of the scan log")
    need(sorted(rows["id"][rows["status"] != 0].tolist()) == g[p + "dead"].tolist(), "terminated targets")
    need((births["id"].tolist() if nb else []) == g[p + "new_ids"].tolist(), "ids of the births")
    sel_meas = alive["sel_meas"].astype(np.int64)
    sel_x = np.array(alive["sel_x"], dtype=np.float64).reshape(-1, 4)
    sel_cn = alive["sel_cnllr"].astype(np.float64)
    if nb:      # a newborn target's selected node is its root: float32 state, measurement it was confirmed with, score 0
        bx = births["x0"].astype(np.float32).astype(np.float64)
        need(np.array_equal(bx, g[p + "born_x"]), "states of the births (bit for bit)")
        need(np.array_equal(births["P0"].reshape(nb, 4, 4).astype(np.float64), g[p + "born_P"]), "covariances of the births (bit for bit)")
        sel_meas = np.concatenate([sel_meas, np.where(births["meas"] > 0, births["meas"], 0).astype(np.int64)])
        sel_x = np.concatenate([sel_x, bx])
        sel_cn = np.concatenate([sel_cn, np.zeros(nb)])
    need(np.array_equal(ids, g[p + "sel_ID"]) and sel_meas.shape == g[p + "sel_meas"].shape, "targets of the selections")
    if not np.array_equal(sel_meas, g[p + "sel_meas"]):
        i = _first_bad(sel_meas, g[p + "sel_meas"])
        need(False, "selections differ for %d targets, first target id %d: measurement %d against %d" % (
            int(np.count_nonzero(sel_meas != g[p + "sel_meas"])), int(ids[i]), int(sel_meas[i]), int(g[p + "sel_meas"][i])))
    need(np.array_equal(sel_x, g[p + "sel_x"]), "selected states (bit for bit)")
    need(np.allclose(sel_cn, g[p + "sel_cnllr"], rtol=0, atol=score_atol), "selected scores")
    ptr, mem = g[p + "cl_ptr"], g[p + "cl_members"]
    cl = clusters_of(rows)
    need(len(cl) == len(ptr) - 1, "%d clusters against %d" % (len(cl), len(ptr) - 1))
    for c, members in enumerate(cl):
        need(np.array_equal(members, mem[ptr[c]:ptr[c + 1]]), "cluster %d" % c)


# ---- device side (imports inside the functions) ----------------------------------------------------------------------------------------------
def debug_counts(trk):
    """(uf, ovl, vt_rebuilds): host-side counters of the library -- scans clustered by the union-find, grow launches made any-order, switches
    of the value table's generation.  Reading them does not touch the device."""
    v, r = np.zeros(2, dtype=np.int32), np.zeros(1, dtype=np.int32)
    from pymht_amd import _lib
    _lib.check(trk._lib.mht_forest_debug_read(trk._ctx.handle, b"uf_ovl", v.ctypes.data_as(C.c_void_p), 8))
    _lib.check(trk._lib.mht_forest_debug_read(trk._ctx.handle, b"vt_rebuilds", r.ctypes.data_as(C.c_void_p), 4))
    return int(v[0]), int(v[1]), int(r[0])


def header_of(rep):
    return tuple(int(getattr(rep, n)) for n in HEADER)


def read_report(trk):
    """`mht_forest_report` (flushes the pending commit): return code, header tuple, rows, used words."""
    from pymht_amd import _lib
    rep = _lib.MhtScanReport()
    rc = trk._lib.mht_forest_report(trk._ctx.handle, C.byref(rep))
    if rc:
        return rc, None, None, None
    dt = trk._REPORT_DTYPE
    recs = np.frombuffer(C.string_at(rep.targets, rep.n_targets * dt.itemsize), dtype=dt) if rep.n_targets else np.zeros(0, dtype=dt)
    used = np.frombuffer(C.string_at(rep.used, 8 * rep.used_words), dtype=np.uint64)
    return 0, header_of(rep), recs, used


def leaf_export(trk, hdr):
    cap = int(min(trk._cfg.max_nodes, max(4096, 2 * hdr[5] + 4 * hdr[1] + 1024)))
    leaf = trk._leaf_export(cap)
    return leaf if leaf is not None else trk._leaf_export(trk._cfg.max_nodes)


class DeviceStream:
    """The scans of a scenario and the births of a pre-pass resident in HBM, as bench.py's Replay keeps them."""

    def __init__(self, scans, births, P_d, device):
        import torch
        self.M = [int(len(z)) for z in scans]
        zall = np.concatenate([np.asarray(z, np.float32).reshape(-1, 2) for z in scans] + [np.zeros((1, 2), np.float32)], axis=0)
        self.z = torch.from_numpy(np.ascontiguousarray(zall)).to(device)
        self.zoff = np.concatenate([[0], np.cumsum(self.M)]).astype(np.int64)
        flat = [b for per in births for b in per]
        self.nb = [len(per) for per in births]
        self.boff = np.concatenate([[0], np.cumsum(self.nb)]).astype(np.int64)
        n = max(len(flat), 1)
        x0, P0, me = np.zeros((n, 4)), np.zeros((n, 16), np.float32), np.zeros(n, np.int32)
        for i, (x, P, m) in enumerate(flat):
            x0[i], P0[i], me[i] = np.asarray(x, np.float64), np.asarray(P, np.float32).reshape(16), m
        self.bx, self.bP, self.bm = torch.from_numpy(x0).to(device), torch.from_numpy(P0).to(device), torch.from_numpy(me).to(device)
        self.bf = torch.full((n,), 3, dtype=torch.uint8, device=device)      # (float32 state and score chains: initiator-born)
        self.bpd = torch.full((n,), float(P_d), dtype=torch.float64, device=device)
        torch.cuda.synchronize()

    def step(self, trk, k):
        """Scan k (0-based) and the births recorded behind it: `mht_forest_step` + `mht_forest_add_targets_dev`, nothing is read."""
        from pymht_amd import _lib
        lib, h = trk._lib, trk._ctx.handle
        _lib.check(lib.mht_forest_step(h, self.z.data_ptr() + int(self.zoff[k]) * 8, self.M[k]))
        nb = self.nb[k]
        if nb:
            o = int(self.boff[k])
            _lib.check(lib.mht_forest_add_targets_dev(h, nb, self.bx.data_ptr() + o * 32, self.bP.data_ptr() + o * 64, self.bf.data_ptr() + o,
                                                      self.bpd.data_ptr() + o * 8, self.bm.data_ptr() + o * 4, 1, None, None))
