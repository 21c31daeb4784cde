"""GPU: the cluster tables every workgroup of the union-find ILP launch derives for itself (uf_prologue, mht_blp.hip) against the
clustering kernel's, table for table.

Three trackers in one process step through the same crafted scene: the default one (blp_uf_kernel_plain), one created under
MHT_BLP_GENERIC=1 (blp_uf_kernel) and one created under MHT_NO_UF=1, whose clusters come from cluster_kernel.  After every scan
cl_counts, cl_ptr, cl_members, multi_list, single_list and t_label must be equal under np.array_equal (the clustering kernel's two lists
after sorting, see ATOMIC_ORDER), and every report row's (id, status, sel_meas).  Which kernel ran is read back through mht_forest_debug_read("blp_instance").

The scenes: stationary targets in runs on a line, SPACING apart within a run, every scan a detection on each target and one half way
between the neighbours of a run -- 6 m off, well inside both gates (NIS < 4 for any innovation variance above 10 m^2), so a run of K
neighbours is one cluster (the test asserts it).  Runs are GAP apart, far outside any gate.  The targets go in through
mht_forest_add_targets without its neighbour test, which turns away a target within 25 m of another.  The sizes are the boundaries of the prologue's code: the wavefront
(64), the workgroup (256: one target per thread, then two), the speculative fetch of UF_SPEC x 256 parents and the four targets a thread
keeps in registers across the scan (1 024 against 1 025), a cluster beyond the 64 members wavefront 0 ranks in registers, a team-sized
cluster (the writer's path in every workgroup), more multi-target clusters than workgroups."""
import ctypes as C

import numpy as np
import pytest

from group_blp_util import N_SCANS, _rd, _runs_mixed, _scene, _tracker

pytestmark = pytest.mark.gpu

INST_TABLES, INST_UF, INST_UF_PLAIN = 1, 2, 3      # mht_kernels.h: BlpInstance
TEAM_MIN_K = 24                                    # mht_kernels.h
TABLES = ("cl_ptr", "cl_members", "multi_list", "single_list", "t_label")
# cluster_kernel hands out the slots of these two lists by atomic counter (mht_cluster.hip: "the (atomic) order of multi_list"): beyond one
# wavefront its order changes from run to run.  The prologue's lists are ascending; the clustering kernel's must hold the same entries, so
# they are compared sorted -- against the prologue's own order, which is thereby asserted ascending.  The two prologue instances are
# compared entry for entry.
ATOMIC_ORDER = ("multi_list", "single_list")

# name -> (runs, environment of every tracker of the scene)
SCENES = {("nT%d" % n): (_runs_mixed(n), {}) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)}
SCENES.update({
    "alone": ([1] * 70, {}),
    "one_chain": ([40], {}),
    "cluster65": ([1, 65, 2, 1], {}),
    "team_min_k": ([2, TEAM_MIN_K, 1, 3], {}),
    "clusters_beyond_grid": ([3] * 80, {"MHT_BLP_GRID": "1"}),      # 80 multi-target clusters, 240 / 8 + 1 = 31 workgroups
})


def _scan_results(trk, k):
    from pymht_amd import _lib
    rep = _lib.MhtScanReport()
    _lib.check(trk._lib.mht_forest_report(trk._ctx.handle, C.byref(rep)))
    assert rep.error == 0 and rep.scan == k + 1
    nT = int(rep.n_targets)
    dt = trk._REPORT_DTYPE
    rows = np.ctypeslib.as_array(C.cast(rep.targets, C.POINTER(C.c_uint8)), shape=(nT * dt.itemsize,)).view(dt).copy()
    cnt = _rd(trk, "cl_counts", 8)
    out = {"row_" + f: rows[f] for f in ("id", "status", "sel_meas")}
    out["cl_counts"] = cnt[:3].copy()
    for name, n in zip(TABLES, (int(cnt[0]) + 1, nT, int(cnt[1]), int(cnt[2]), nT)):
        out[name] = _rd(trk, name, n)
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_prologue_tables_equal_the_cluster_kernels(name):
    import torch
    from pymht_amd import _lib
    runs, env = SCENES[name]
    x0, scans = _scene(runs)
    nT = len(x0)
    assert nT == sum(runs)
    trackers = [(_tracker(x0, dict(env)), INST_UF_PLAIN, "the plain instance"),
                (_tracker(x0, dict(env, MHT_NO_UF="1")), INST_TABLES, "the clustering kernel"),
                (_tracker(x0, dict(env, MHT_BLP_GENERIC="1")), INST_UF, "the generic instance")]
    dev = trackers[0][0]._ctx.device
    zall = torch.from_numpy(np.concatenate(scans, axis=0)).to(dev)
    zoff = np.concatenate([[0], np.cumsum([len(z) for z in scans])]).astype(np.int64)
    torch.cuda.synchronize()
    try:
        for k in range(N_SCANS):
            res = []
            for trk, want, _ in trackers:
                _lib.check(trk._lib.mht_forest_step(trk._ctx.handle, zall.data_ptr() + int(zoff[k]) * 8, len(scans[k])))
                got = int(_rd(trk, "blp_instance", 1)[0])
                assert got == want, "scan %d: ILP launch ran as instance %d, expected %d" % (k, got, want)
                res.append(_scan_results(trk, k))
            ref = res[0]
            for other, (_, want, who) in zip(res[1:], trackers[1:]):
                for key in ref:
                    theirs = np.sort(other[key]) if (want == INST_TABLES and key in ATOMIC_ORDER) else other[key]
                    assert np.array_equal(ref[key], theirs), "scan %d: %s differs between the plain instance and %s" % (k, key, who)
            # the scene is the one meant: every run one cluster, in index order
            sizes = np.diff(ref["cl_ptr"])
            assert sizes.tolist() == list(runs), "scan %d: cluster sizes %s" % (k, sizes.tolist()[:20])
            assert ref["cl_counts"].tolist() == [len(runs), sum(1 for r in runs if r >= 2), sum(1 for r in runs if r == 1)]
            assert np.array_equal(ref["cl_members"], np.arange(nT))
            assert len(ref["row_id"]) == nT
    finally:
        for trk, _, _ in trackers:
            trk.close()
