"""GPU: the two instances of the union-find ILP launch (mht_blp.hip) -- blp_uf_kernel_plain, a plain forest's switches compiled in, and the
generic blp_uf_kernel that reads them at run time -- must be the same solver: one small seeded scene is stepped through two trackers in one
process, the second created under MHT_BLP_GENERIC=1, and every scan's results are compared bit for bit.  launch_blp's pick of the instance
is read back through mht_forest_debug_read("blp_instance")."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INST_TABLES, INST_UF, INST_UF_PLAIN = 1, 2, 3      # mht_kernels.h: BlpInstance (1 and 2 read every switch at run time: the generic kernels)
BRANCHED = 2                                       # include/mht_amd.h: MHT_BLP_BRANCHED
PERIOD, P_D, LAMBDA_PHI, RADIUS, N_SCANS, SEED = 2.5, 0.9, 1.0e-5, 400.0, 12, 5446
SPACING = 35.0      # metres between the members of a group at the start (30-40 m)


def _scene():
    """12 targets in four groups of three.  The members of a group start SPACING apart on the corners of a triangle and run through its
    centre on crossing courses (they meet half way through the run), the group as a whole drifts: around the crossing the three gates hold the
    same measurements.  Detections with P_d 0.9, sigma 2.5 m, a few clutter points per scan."""
    rng = np.random.default_rng(SEED)
    r = SPACING / np.sqrt(3.0)
    t_cross = 0.5 * N_SCANS * PERIOD
    x = []
    for g in range(4):
        centre = 220.0 * np.array([np.cos(0.5 * np.pi * g + 0.3), np.sin(0.5 * np.pi * g + 0.3)])
        drift = rng.normal(0.0, 3.0, size=2)
        for m in range(3):
            a = 2.0 * np.pi * m / 3.0 + 0.4 * g
            off = r * np.array([np.cos(a), np.sin(a)])
            x.append(np.concatenate([centre + off, drift - off / t_cross]))
    x = np.array(x, dtype=np.float64)
    x0 = x.copy()
    scans, times = [], []
    for k in range(N_SCANS):
        x[:, 0:2] += PERIOD * x[:, 2:4]
        seen = rng.uniform(size=len(x)) <= P_D
        det = x[seen, 0:2] + rng.normal(0.0, 2.5, size=(int(seen.sum()), 2))
        n_cl = rng.poisson(LAMBDA_PHI * np.pi * RADIUS * RADIUS)
        rc, tc = RADIUS * np.sqrt(rng.uniform(size=n_cl)), rng.uniform(0.0, 2.0 * np.pi, size=n_cl)
        z = np.concatenate([det, np.stack([rc * np.cos(tc), rc * np.sin(tc)], axis=1)], axis=0)
        rng.shuffle(z, axis=0)
        scans.append(np.ascontiguousarray(z, dtype=np.float32).reshape(-1, 2))
        times.append(1000.0 + (k + 1) * PERIOD)
    return x0, scans, times


def _tracker(x0, N, generic=False, **kw):
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import pv
    old = os.environ.pop("MHT_BLP_GENERIC", None)
    if generic:
        os.environ["MHT_BLP_GENERIC"] = "1"      # (read when the forest is created)
    try:
        trk = Tracker(pv, PERIOD, LAMBDA_PHI, 1e-4, P_d=P_D, N=N, eta2=5.99, useInitiator=False, maxTargets=64, maxNodes=1 << 18,
                      maxMeasurements=128, **kw)
        trk._add_targets([Target(1000.0, None, x.copy(), pv.P0, status="preinitialized") for x in x0])
    finally:
        os.environ.pop("MHT_BLP_GENERIC", None)
        if old is not None:
            os.environ["MHT_BLP_GENERIC"] = old
    return trk


def _rd(trk, name, n):
    from pymht_amd import _lib
    a = np.zeros(max(int(n), 1), dtype=np.int32)
    _lib.check(trk._lib.mht_forest_debug_read(trk._ctx.handle, name.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes))
    return a[:int(n)]


def _instance(trk):
    return int(_rd(trk, "blp_instance", 1)[0])


# the report's columns that do not name a node.  (Node indices are not compared as such: a target that outgrows its static block of the
# node pool continues in the overflow area, whose regions are handed out by atomic counters -- two runs of the SAME build place such
# children at different indices.  The selection is compared as the child's position in its target's block, the roots by scan / measurement /
# state / score.)
ROW_FIELDS = ("id", "status", "sel_meas", "sel_x", "sel_cnllr", "score", "root_scan", "root_meas", "root_x", "root_cnllr", "n_leaves", "cluster")


def _scan_results(trk, k):
    """everything the ILP launch of the last scan left: the report's rows and the solver's tables, all targets and all clusters"""
    from pymht_amd import _lib
    rep = _lib.MhtScanReport()
    _lib.check(trk._lib.mht_forest_report(trk._ctx.handle, C.byref(rep)))
    assert rep.error == 0 and rep.scan == k + 1
    nT = int(rep.n_targets)
    dt = trk._REPORT_DTYPE
    rows = np.ctypeslib.as_array(C.cast(rep.targets, C.POINTER(C.c_uint8)), shape=(nT * dt.itemsize,)).view(dt).copy()
    cnt = _rd(trk, "cl_counts", 8)
    nC = int(cnt[0])
    out = {"row_" + f: rows[f] for f in ROW_FIELDS if f in dt.names}
    assert len(out) >= 10, dt.names
    out.update({"counts": cnt[:3].copy(), "cl_ptr": _rd(trk, "cl_ptr", nC + 1), "multi_list": _rd(trk, "multi_list", int(cnt[1]))})
    out["sel"] = _rd(trk, "sel", nT) - _rd(trk, "tchild", nT)      # selected child, counted from the first child of its target
    for name, n in (("t_label", nT), ("cl_members", nT), ("cl_status", nC), ("cl_iters", nC), ("cl_nodes", nC)):
        out[name] = _rd(trk, name, n)
    return out


@pytest.mark.parametrize("N", [5, 3])
def test_plain_and_generic_instance_agree_scan_by_scan(N):
    import torch
    from pymht_amd import _lib
    x0, scans, _ = _scene()
    plain, generic = _tracker(x0, N), _tracker(x0, N, generic=True)
    dev = plain._ctx.device
    zall = torch.from_numpy(np.concatenate(scans, axis=0)).to(dev)
    zoff = np.concatenate([[0], np.cumsum([len(z) for z in scans])]).astype(np.int64)
    torch.cuda.synchronize()
    iterated = branched = triples = 0
    try:
        for k in range(N_SCANS):
            res = []
            for trk, want in ((plain, INST_UF_PLAIN), (generic, INST_UF)):
                _lib.check(trk._lib.mht_forest_step(trk._ctx.handle, zall.data_ptr() + int(zoff[k]) * 8, len(scans[k])))
                assert _instance(trk) == want, "scan %d: ILP launch ran as instance %d, expected %d" % (k, _instance(trk), want)
                res.append(_scan_results(trk, k))
            a, b = res
            for name in a:
                if name == "cl_nodes":
                    # (the exact search of a small cluster deals its subtrees out to the wavefronts, which prune against ONE incumbent word
                    # they all lower as they go: how many nodes a wavefront visits before a sibling's better selection cuts it short is a
                    # matter of timing -- two runs of the same kernel differ.  Its result is not.  Counts of clusters settled that way are
                    # compared as "searched at all", every other cluster's count exactly.)
                    br = a["cl_status"] == BRANCHED
                    assert np.array_equal(a[name][~br], b[name][~br]) and np.array_equal(a[name][br] > 0, b[name][br] > 0), "scan %d: cl_nodes" % k
                    continue
                assert np.array_equal(a[name], b[name]), "scan %d: %s differs between the plain and the generic instance" % (k, name)
            ml, ptr = a["multi_list"], a["cl_ptr"]
            iterated += int((a["cl_iters"][ml] >= 1).sum())
            branched += int((a["cl_status"][ml] == BRANCHED).sum())
            triples += int(((ptr[ml + 1] - ptr[ml]) == 3).sum())
        print("N=%d: clusters with >= 1 dual round %d, settled by the exact paths %d, with three members %d" % (N, iterated, branched, triples))
        assert iterated >= 1, "no cluster of the scene needed a dual round"
        assert branched >= 1, "no cluster of the scene was settled by the exact paths (status BRANCHED)"
        assert triples >= 1, "no cluster of the scene had three members"
    finally:
        plain.close()
        generic.close()


def test_similar_state_pruning_takes_a_generic_instance():
    """similar-state pruning marks children dead between clustering and the ILPs (BlpArgs::skip_dead): not a plain forest's scan"""
    from pymht_amd.utils.classDefinitions import MeasurementList
    x0, scans, times = _scene()
    trk = _tracker(x0, 5)
    try:
        trk.addMeasurementList(MeasurementList(float(times[0]), scans[0]))
        trk._ctx.synchronize()
        assert _instance(trk) == INST_UF_PLAIN
        trk.addMeasurementList(MeasurementList(float(times[1]), scans[1]), pruneSimilar=True)
        trk._ctx.synchronize()
        assert _instance(trk) in (INST_TABLES, INST_UF)
    finally:
        trk.close()


def test_cluster_sharded_step_takes_a_generic_instance():
    """two shards in one process (tests/test_sharded_gpu.py): shard_n = 2, selections relative to the targets' blocks"""
    import torch
    from pymht_amd.parallel import ClusterShardedTracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    x0, scans, times = _scene()
    parts = [ClusterShardedTracker(_tracker(x0, 5), 2, i, exchange=lambda t: None) for i in range(2)]
    try:
        for k in range(2):
            sl = MeasurementList(float(times[k]), scans[k])
            for p in parts:
                p.begin(sl)
            for p in parts:
                assert _instance(p.trk) in (INST_TABLES, INST_UF)
            merged = torch.stack([p.sel_rel for p in parts]).max(dim=0).values
            for p in parts:
                p.sel_rel.copy_(merged)
                p.end()
    finally:
        for p in parts:
            p.trk.close()
