"""GPU: the member lists of the union-find ILP launch (uf_prologue, mht_blp.hip) for clusters whose members are SCATTERED over the target
table.

tests/test_blp_prologue_gpu.py plants runs of consecutive target indices, so cl_members is arange(nT) there.  A workgroup's own member
list is collected by its four wavefronts in stripes of 64 targets (stripe i: wavefront i % 4, pass i / 4), the slots of a stripe handed
out by an LDS atomic -- in any order -- and the at most 64 entries ranked in wavefront 0's registers; neither the order of the slots nor
the ranking shows with consecutive members.  Here the scenes of group_blp_util._scene (runs of neighbours on a line, every run one
cluster) are planted through a permutation of the targets: target i stands at the scene's position place[i], so chosen INDEX SETS form
the clusters.  The scans are positions only and stay as they are.

Three trackers step through each scene, as in that test: the plain instance, the generic one (MHT_BLP_GENERIC=1) and the clustering
kernel (MHT_NO_UF=1).  After every scan cl_counts, cl_ptr, cl_members, multi_list, single_list, t_label and the report rows' (id, status,
sel_meas) must be equal under np.array_equal across the three (the clustering kernel's two atomic-order lists sorted) AND equal to the
tables computed on the host from the index sets alone: label = smallest member, clusters in order of their smallest member, members
ascending.

600 targets are ten stripes, the last one partial: three passes for wavefronts 0 and 1, two for the others.  Every scene is padded with
lone targets and a few pairs of consecutive indices, so that there are several multi-target clusters and every workgroup has another
root."""
import ctypes as C

import numpy as np
import pytest

from group_blp_util import N_SCANS, _rd, _scene, _tracker

pytestmark = pytest.mark.gpu

INST_TABLES, INST_UF, INST_UF_PLAIN = 1, 2, 3      # mht_kernels.h: BlpInstance
TABLES = ("cl_ptr", "cl_members", "multi_list", "single_list", "t_label")
ATOMIC_ORDER = ("multi_list", "single_list")       # cluster_kernel: slots by atomic counter (tests/test_blp_prologue_gpu.py)


def _every(step, n, first=3):
    return [first + step * i for i in range(n)]


# name -> (targets, index sets in the order their members stand on the line, environment of every tracker of the scene)
SCENES = {
    "first_and_last": (600, [[0, 599]], {}),                            # the last stripe is partial
    "stripe_edge": (600, [[63, 64]], {}),
    "four_wavefronts_one_pass": (600, [[5, 70, 135, 200]], {}),
    "one_wavefront_three_passes": (600, [[10, 266, 522]], {}),          # stripes 0, 4, 8
    "cluster64_every_9th": (600, [_every(9, 64)], {}),                  # the largest cluster a wavefront ranks in registers
    "cluster65_every_9th": (600, [_every(9, 65)], {}),                  # ... and one more: the full path
    "one_stripe_descending": (600, [[190, 181, 177, 170, 150, 131, 129]], {}),      # stripe 2, the line's order against the indices'
    "nT65": (65, [[0, 64]], {}),
    "nT257": (257, [[1, 256]], {}),
    # 80 scattered triples, 240 / 8 + 1 = 31 workgroups: several clusters per workgroup, the full path with scattered members
    "triples_beyond_grid": (240, [[i, i + 160, i + 80] for i in range(80)], {"MHT_BLP_GRID": "1"}),
}
N_PAIRS = 4      # pairs of consecutive indices among the padding


def _layout(nT, sets):
    """runs of the scene and place[i] = the scene's position of target i: the index sets first, then N_PAIRS pairs of free consecutive
    indices, then every other target alone; returns (runs, place, all index sets of the scene, the lone targets included)"""
    taken = set(t for s in sets for t in s)
    assert len(taken) == sum(len(s) for s in sets) and max(taken) < nT
    groups, t = [list(s) for s in sets], 20
    while len(groups) < len(sets) + N_PAIRS and t + 1 < nT:
        if t not in taken and t + 1 not in taken:
            groups.append([t, t + 1])
            taken.update((t, t + 1))
            t += 37
        else:
            t += 1
    groups += [[t] for t in range(nT) if t not in taken]
    place, pos = np.zeros(nT, dtype=np.int64), 0
    for g in groups:
        for t in g:
            place[t] = pos
            pos += 1
    assert pos == nT
    return [len(g) for g in groups], place, groups


def _host_tables(nT, groups):
    """what the launch must derive, from the index sets alone"""
    order = sorted((sorted(g) for g in groups), key=lambda g: g[0])
    label = np.zeros(nT, dtype=np.int32)
    for g in order:
        label[g] = g[0]
    return {
        "cl_counts": np.array([len(order), sum(1 for g in order if len(g) >= 2), sum(1 for g in order if len(g) == 1)], dtype=np.int32),
        "cl_ptr": np.concatenate([[0], np.cumsum([len(g) for g in order])]).astype(np.int32),
        "cl_members": np.array([t for g in order for t in g], dtype=np.int32),
        "multi_list": np.array([c for c, g in enumerate(order) if len(g) >= 2], dtype=np.int32),
        "single_list": np.array([g[0] for g in order if len(g) == 1], dtype=np.int32),
        "t_label": label,
    }


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


def test_host_tables_of_a_small_layout():
    """the reference itself, by hand: five targets, {4, 1} one cluster"""
    runs, place, groups = _layout(5, [[4, 1]])
    assert runs == [2, 1, 1, 1] and place.tolist() == [2, 1, 3, 4, 0]
    want = _host_tables(5, groups)
    assert want["cl_counts"].tolist() == [4, 1, 3] and want["cl_ptr"].tolist() == [0, 1, 3, 4, 5]
    assert want["cl_members"].tolist() == [0, 1, 4, 2, 3] and want["t_label"].tolist() == [0, 1, 2, 3, 1]
    assert want["multi_list"].tolist() == [1] and want["single_list"].tolist() == [0, 2, 3]


@pytest.mark.parametrize("name", list(SCENES))
def test_member_lists_of_scattered_clusters(name):
    import torch
    from pymht_amd import _lib
    nT, sets, env = SCENES[name]
    runs, place, groups = _layout(nT, sets)
    pos0, scans = _scene(runs)
    assert len(pos0) == nT
    x0 = pos0[place]      # target i stands where the scene has its position place[i]
    want = _host_tables(nT, groups)
    assert int(want["cl_counts"][1]) >= 2
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
            for trk, inst, _ in trackers:
                _lib.check(trk._lib.mht_forest_step(trk._ctx.handle, zall.data_ptr() + int(zoff[k]) * 8, len(scans[k])))
                got = int(_rd(trk, "blp_instance", 1)[0])
                assert got == inst, "scan %d: ILP launch ran as instance %d, expected %d" % (k, got, inst)
                res.append(_scan_results(trk, k))
            ref = res[0]
            for key in want:
                assert np.array_equal(ref[key], want[key]), "scan %d: %s of the plain instance differs from the host's" % (k, key)
            for other, (_, inst, who) in zip(res[1:], trackers[1:]):
                for key in ref:
                    theirs = np.sort(other[key]) if (inst == INST_TABLES and key in ATOMIC_ORDER) else other[key]
                    assert np.array_equal(ref[key], theirs), "scan %d: %s differs between the plain instance and %s" % (k, key, who)
            assert len(ref["row_id"]) == nT
    finally:
        for trk, _, _ in trackers:
            trk.close()
