"""GPU: mht_kbest_hypotheses (csrc/mht_kbest.hip) through the raw seam of both builds, pymht_amd.evaluation.k_best_hypotheses,
mht_forest_leaf_rows and Tracker.getGlobalHypotheses.

Raw seam: the cases of tests/kbest_ref.py, every output preset to a sentinel and none left behind; costs, tuples, count, status and
nodes bit for bit the host twin's (tests/hostmath/kbest_host.cpp, which tests/test_kbest_cpu.py holds to the reference); prob and the
marginals within (2 K + 64) eps of the np.longdouble fold of the device's own costs (the ratio is printed).
Tracker level: fuzz_util.scenario_of seeds 11, 16 and 36 and one six-state scene next to the live oracle: the exported window rows are
the oracle's ILP columns as key sets, the lists are the reference's on the device's own cnllr and rows bit for bit, and the tracker's
own selection is where it must be."""
import ctypes as C

import numpy as np
import pytest
import torch

import kbest_ref as ref

pytestmark = pytest.mark.gpu
GUARD = 16


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return ref.build_twin(tmp_path_factory.mktemp("kbest_host"))


@pytest.fixture(scope="module", params=[4, 6])
def ctx_nx(request):
    from pymht_amd.device import Context
    ctx = Context(0, nx=request.param)
    yield ctx
    ctx.close()


def call_seam(ctx, p, K, node_limit=1 << 20, expect_rc=0, short_work=False, override=None):
    """The raw seam on a packed call: device copies of the inputs, outputs preset to the sentinel with a guard band behind each.
    Returns the outputs as kbest_ref.outputs' dict (guards checked and cut off)."""
    dev, lib = ctx.device, ctx.lib
    ins = {k: torch.from_numpy(np.ascontiguousarray(p[k])).to(dev) for k in ("group_ptr", "rows", "cost", "cluster_ptr", "cluster_targets")}
    host = ref.outputs(p, K)
    outs = {k: torch.from_numpy(np.concatenate([v.reshape(-1), np.full(GUARD, ref.SENTINEL, dtype=v.dtype)])).to(dev) for k, v in host.items()}
    need = int(lib.mht_kbest_work_bytes(p["nHyp"], p["nT"], p["nC"], p["depth"], K)) if 1 <= K <= ref.MAX_K else 256
    work = torch.zeros(max(need, 256), dtype=torch.uint8, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    a = dict(nHyp=p["nHyp"], nT=p["nT"], nC=p["nC"], depth=p["depth"], K=K, node_limit=node_limit, work=work.data_ptr(),
             work_bytes=need - 1 if short_work else need)
    a.update({k: v.data_ptr() for k, v in ins.items()})
    a.update({k: v.data_ptr() for k, v in outs.items()})
    a.update(override or {})      # (a bad argument in place of a good one)
    rc = lib.mht_kbest_hypotheses(ctx.handle, a["nHyp"], a["nT"], a["nC"], a["depth"], a["K"], a["node_limit"], a["group_ptr"], a["rows"], a["cost"],
                                  a["cluster_ptr"], a["cluster_targets"], a["count"], a["status"], a["nodes"], a["hyp_cost"], a["hyp_prob"], a["hyp_sel"],
                                  a["marginal"], a["work"], a["work_bytes"])
    assert rc == expect_rc, (rc, lib.mht_last_error())
    assert lib.mht_synchronize(ctx.handle) == 0
    got = {}
    for k, v in host.items():
        flat = outs[k].cpu().numpy()
        assert (flat[v.size:] == ref.SENTINEL).all(), "the guard behind %s was written" % k
        got[k] = flat[:v.size].reshape(v.shape)
    return got


def hold_twin(label, got, want):
    for k in ("count", "status", "nodes", "hyp_cost", "hyp_sel"):
        assert ref.same_bits(got[k], want[k]), (label, k, got[k], want[k])


def test_cases_through_the_raw_seam(ctx_nx, twin):
    worst = 0.0
    for case in ref.cases():
        p, K = case["packed"], case["K"]
        got = call_seam(ctx_nx, p, K)
        ref.hold_case(case, got)
        hold_twin(case["label"], got, ref.call_twin(twin, p, K))
        r = ref.hold_probabilities(case["label"], p, got, K)
        worst = max(worst, r)
        print("%d-state build, %s: nodes %s, ratio to the bound %.3g" % (ctx_nx.lib.nx, case["label"], got["nodes"].tolist()[:8], r))
    print("%d-state build: worst ratio of prob and the marginals to the bound (2 K + 64) eps: %.3g" % (ctx_nx.lib.nx, worst))
    assert worst <= 1.0


def test_a_node_limit_that_fires(ctx_nx, twin):
    case = ref._case("chain", [ref.chain_instance(32), ref.random_instance(np.random.default_rng(3), 2)], 8)
    p = case["packed"]
    for limit in (1, 64, 200, 5000):
        got = call_seam(ctx_nx, p, 8, limit)
        assert got["status"][0] == ref.NODE_LIMIT and got["nodes"][0] <= limit
        hold_twin("limit %d" % limit, got, ref.call_twin(twin, p, 8, limit))
        ref.hold_probabilities("limit %d" % limit, p, got, 8)


def test_300_clusters_in_one_launch_and_a_permutation(ctx_nx, twin):
    rng = np.random.default_rng(8)
    insts = [ref.random_instance(rng, int(rng.integers(1, 6)), cost_levels=None if i % 4 else 3, n_rows=int(rng.integers(3, 9))) for i in range(300)]
    case = ref._case("300 clusters", insts, 8)
    p = case["packed"]
    got = call_seam(ctx_nx, p, 8)
    ref.hold_case(case, got)
    hold_twin("300 clusters", got, ref.call_twin(twin, p, 8))
    ref.hold_probabilities("300 clusters", p, got, 8)
    assert (got["count"] > 0).sum() > 200 and (got["count"] == 8).sum() > 50      # (the reference lists 245 feasible clusters, 77 full lists)
    # the clusters in another order (the targets and columns stay where they are): every cluster's outputs move with it, bit for bit
    perm = rng.permutation(300)
    q = dict(p)
    sizes = np.diff(p["cluster_ptr"])
    q["cluster_ptr"] = np.concatenate([[0], np.cumsum(sizes[perm])]).astype(np.int32)
    q["cluster_targets"] = np.concatenate([p["cluster_targets"][p["cluster_ptr"][c]:p["cluster_ptr"][c + 1]] for c in perm]).astype(np.int32)
    moved = call_seam(ctx_nx, q, 8)
    for k in ("count", "status", "nodes"):
        assert np.array_equal(moved[k], got[k][perm]), k
    for k in ("hyp_cost", "hyp_prob"):
        assert ref.same_bits(moved[k], np.ascontiguousarray(got[k][:, perm])), k
    assert ref.same_bits(moved["hyp_sel"], got["hyp_sel"]) and ref.same_bits(moved["marginal"], got["marginal"])


def test_a_too_large_cluster_leaves_its_neighbours_alone(ctx_nx, twin):
    rng = np.random.default_rng(9)
    good = [ref.random_instance(rng, 3) for _ in range(4)]
    big = ref.random_instance(rng, 2, sizes=[1000, 25], n_rows=50)
    alone = call_seam(ctx_nx, ref.pack(good), 8)
    case = ref._case("too large in the middle", good[:2] + [big] + good[2:], 8)
    got = call_seam(ctx_nx, case["packed"], 8)
    ref.hold_case(case, got)
    assert got["status"].tolist() == [0, 0, ref.TOO_LARGE, 0, 0] and got["count"][2] == 0 and got["nodes"][2] == 0
    keep = [0, 1, 3, 4]
    assert ref.same_bits(np.ascontiguousarray(got["hyp_cost"][:, keep]), alone["hyp_cost"]) and ref.same_bits(np.ascontiguousarray(got["hyp_prob"][:, keep]), alone["hyp_prob"])
    assert np.array_equal(got["count"][keep], alone["count"]) and np.array_equal(got["nodes"][keep], alone["nodes"])
    lo, hi = case["packed"]["group_ptr"][[6, 8]]      # (the big cluster's columns)
    assert np.isnan(got["marginal"][lo:hi]).all() and ref.same_bits(np.concatenate([got["marginal"][:lo], got["marginal"][hi:]]), alone["marginal"])


def test_every_bad_argument_is_refused_and_nothing_is_written(ctx_nx):
    from pymht_amd import _lib
    p = ref.cases()[3]["packed"]
    bads = [dict(nHyp=0), dict(nT=0), dict(nC=0), dict(nHyp=-1), dict(depth=-1), dict(K=0), dict(K=ref.MAX_K + 1), dict(node_limit=0), dict(node_limit=-5)]
    bads += [{k: None} for k in ("group_ptr", "rows", "cost", "cluster_ptr", "cluster_targets", "count", "status", "nodes", "hyp_cost", "hyp_prob", "hyp_sel",
                                 "marginal", "work")]
    for bad in bads:
        got = call_seam(ctx_nx, p, 8, expect_rc=_lib.MHT_E_INVALID, override=bad)
        assert all((got[k] == ref.SENTINEL).all() for k in ref.OUT_NAMES), bad
    got = call_seam(ctx_nx, p, 8, expect_rc=_lib.MHT_E_INVALID, short_work=True)
    assert all((got[k] == ref.SENTINEL).all() for k in ref.OUT_NAMES)
    assert ctx_nx.lib.mht_kbest_hypotheses(None, *([1] * 6), *([None] * 13), 0) == _lib.MHT_E_INVALID


def test_evaluation_front_end(gpu_ctx):
    """Arbitrary keys, a leaf set whose targets fall into several clusters, against the reference per cluster."""
    from pymht_amd.evaluation import k_best_hypotheses
    rng = np.random.default_rng(12)
    T = 40
    target = np.sort(np.concatenate([np.arange(T), rng.integers(0, T, 160)])).astype(np.int32)
    # (blocks of four targets draw their keys from a pool of their own: clusters of at most four targets)
    rows = np.where(rng.random((len(target), 3)) < 0.5, -1, ((target // 4)[:, None] * 8 + rng.integers(0, 8, (len(target), 3))) * 1000003 + 17)
    cost = rng.uniform(-3.0, 9.0, len(target))
    out = k_best_hypotheses(cost, target, rows, 8, ctx=gpu_ctx)
    hold_front_end(out, cost, target, rows, 8)
    assert sum(len(c) > 1 for c in out["clusters"]) >= 3 and (out["count"] == 8).any()


def hold_front_end(out, cost, target, rows, k, label=""):
    """k_best_hypotheses' dict against the reference run per cluster on the same costs and keys: bit for bit."""
    T = int(target[-1]) + 1
    seg = np.searchsorted(target, np.arange(T + 1))
    assert sorted(int(t) for c in out["clusters"] for t in c) == list(range(T))
    for c, tg in enumerate(out["clusters"]):
        idx = np.concatenate([np.arange(seg[t], seg[t + 1]) for t in tg])
        sizes = [int(seg[t + 1] - seg[t]) for t in tg]
        keys = [[int(r) for r in rows[i] if r >= 0] for i in idx]
        assert out["status"][c] == ref.OK, (label, c, out["status"][c])
        want, _ = ref.branch_and_bound(sizes, cost[idx], keys, k)
        assert out["count"][c] == len(want), (label, c, out["count"][c], len(want))
        for r, (cst, tup) in enumerate(want):
            assert ref.same_bits(np.float64(out["cost"][c, r]), np.float64(cst)), (label, c, r)
            assert [int(v) for v in out["selection"][r, tg]] == [int(seg[t] + o) for t, o in zip(tg, tup)], (label, c, r)
        assert np.isnan(out["cost"][c, len(want):]).all() and (out["selection"][len(want):, tg] == -1).all()
        # other clusters' keys do not matter: no key of this cluster appears in another
        mine = set(kk for col in keys for kk in col)
        others = np.setdiff1d(np.arange(len(target)), idx)
        assert not mine & set(int(r) for r in rows[others].reshape(-1) if r >= 0), (label, c)
    lp = np.zeros(len(target), dtype=np.longdouble)
    for c, tg in enumerate(out["clusters"]):
        n = int(out["count"][c])
        if n:
            pr = ref.fold_probabilities(out["cost"][c, :n])
            assert np.all(np.abs(out["prob"][c, :n] - pr) <= (2 * k + 64) * ref.EPS * pr)
            for r in range(n):
                lp[out["selection"][r, tg]] += pr[r]
    assert np.all(np.abs(out["leafProbability"] - lp) <= (2 * k + 64) * ref.EPS * lp), label


def oracle_keys(o, N):
    """build_blp over all targets of the oracle: per leaf (the oracle's leaf order) the set of device keys (level << 24) | meas"""
    import mht_oracle as orc
    cols, sizes, cost, meas_list, leaves = orc.build_blp(o.targets, N)
    now = max(l.scan for l in leaves)
    return [set(((now - meas_list[r][0]) << 24) | int(meas_list[r][1]) for r in col) for col in cols], sizes, now


def hold_tracker(trk, o, N, label, shape, dead_nodes):
    """After the last scan: the exported rows against the oracle's columns, the lists against the reference, the tracker's selection."""
    keys, sizes, now = oracle_keys(o, N)
    snap = trk.leafBatch()
    rows = trk.leafRows()
    assert len(rows) == len(keys) == len(snap["cnllr"]) and np.array_equal(np.bincount(snap["target"]), sizes), label
    for i, want in enumerate(keys):
        got = [int(r) for r in rows[i] if r >= 0]
        assert len(got) == len(set(got)) and set(got) == want, (label, i, got, sorted(want))
    # the exported rows as they are (the oracle's columns): the shapes, and the lists of every cluster against the reference
    from pymht_amd.evaluation import k_best_hypotheses
    k = 8
    plain = k_best_hypotheses(snap["cnllr"], snap["target"], rows, k, ctx=trk._ctx)
    multi = sorted((len(tg), int(sum(sizes[t] for t in tg))) for tg in plain["clusters"] if len(tg) > 1)
    print("%s: %d leaves, multi-target clusters (targets, columns) %s, nodes at most %d" % (label, len(keys), multi, int(plain["nodes"].max())))
    shape(multi, len(keys))
    hold_front_end(plain, snap["cnllr"], snap["target"], rows, k, label)
    assert int((plain["count"][[len(tg) > 1 for tg in plain["clusters"]]] == k).sum()) == len(multi), "a multi-target cluster with fewer than %d feasible hypotheses" % k
    # the Tracker's call: the same rows but for the targets born since the last scan (the number of such a target's plot counts the
    # scan's UNUSED plots, the initiator's numbering: it is no key, and the call leaves it out)
    out = trk.getGlobalHypotheses(k=k)
    born = np.array([nd._node < 0 for nd in trk.__trackNodes__])
    used = np.where(born[snap["target"]][:, None], -1, rows)
    assert np.array_equal(out["rows"], used), label
    rows = out["rows"]
    hold_front_end(out, snap["cnllr"], snap["target"], rows, k, label)
    assert out["ids"] == [int(t.ID) for t in trk.__targetList__] and np.array_equal(out["leafIds"], snap["ID"])
    # the tracker's own selection: one leaf per target, feasible; listed where it is cheap enough; first where nothing was terminated
    sel = out["selected"]
    assert (sel >= 0).all() and np.array_equal(snap["target"][sel], np.arange(len(sel))), label
    freed = set()
    for node in dead_nodes:
        n = node
        while n is not None:
            if n.meas not in (0, None) and 0 <= now - n.scan < 128:
                freed.add(((now - n.scan) << 24) | int(n.meas))
            n = n.parent
    n_first = 0
    for c, tg in enumerate(out["clusters"]):
        mine = [int(r) for i in sel[tg] for r in rows[i] if r >= 0]
        assert len(mine) == len(set(mine)), (label, c)
        cst = ref.total(snap["cnllr"], sel[tg])
        n = int(out["count"][c])
        assert n >= 1
        if n < k or cst < out["cost"][c, n - 1]:
            r = int(out["selectedRank"][c])
            assert r >= 0 and ref.same_bits(np.float64(out["cost"][c, r]), np.float64(cst)), (label, c, r)
        cluster_keys = set(int(r) for t in tg for i in np.flatnonzero(snap["target"] == t) for r in rows[i] if r >= 0)
        if not (cluster_keys & freed) and (n == 1 or out["cost"][c, 1] - out["cost"][c, 0] > 1e-9):
            assert out["selectedRank"][c] == 0, (label, c, out["selectedRank"][c], out["cost"][c, :3], cst)
            n_first += 1
    assert n_first >= 1


SHAPES = {11: lambda multi, L: (4, 52) in multi,
          16: lambda multi, L: len(multi) == 7 and L == 685,
          36: lambda multi, L: (14, 353) in multi}


@pytest.mark.parametrize("seed", [11, 16, 36])
def test_tracker_against_the_live_oracle(seed):
    import fuzz_util
    from test_tracker_gpu import make_tracker
    from trace_util import make_oracle
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, N, eta2, desc = fuzz_util.scenario_of(seed)
    g = dict(period=sc["period"], lambda_phi=sc["lambda_phi"], lambda_nu=1e-4, P_d=sc["P_d"], N=N, eta2=eta2, x0=sc["x0"], t0=sc["t0"], accepted=None)
    trk, acc = make_tracker(sc["period"], sc["lambda_phi"], 1e-4, sc["P_d"], N, eta2, sc["x0"], sc["t0"])
    try:
        g["accepted"] = acc
        o = make_oracle(g)
        info = None
        for z, t in zip(sc["scans"], sc["times"]):
            info = o.add_scan(float(t), z)
            trk.addMeasurementList(MeasurementList(float(t), z))
        dead = o.terminated[len(o.terminated) - len(info["dead"]):] if info["dead"] else []

        def shape(multi, L):
            assert SHAPES[seed](multi, L), (desc, multi, L)
        hold_tracker(trk, o, N, desc, shape, dead)
    finally:
        trk.close()


def test_six_state_tracker_against_the_live_oracle():
    """fuzz_util.ca_scene(16): the linear six-state forest.  The oracle is built as fuzz_util.oracle_run builds it, kept here so that
    its trees can be read."""
    import fuzz_util
    import mht_oracle as orc
    from pymht_amd.models import ca
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    scene = fuzz_util.ca_scene(16)
    sc = scene["sc"]
    o = orc.OracleTracker(sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=scene["N"], eta2=scene["eta2"], initiator=None, model=ca)
    trk = Tracker(ca, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=scene["N"], eta2=scene["eta2"], useInitiator=False, maxTargets=256,
                  maxNodes=1 << 18, maxMeasurements=scene["max_meas"], pruneThreshold=scene["thr"])
    try:
        for x in scene["x0"]:
            n0 = trk.nTargets
            trk.initiateTarget(Target(sc["t0"], None, x.copy(), ca.P0, status="preinitialized"))
            assert o.initiate_target(sc["t0"], x.copy(), np.array(ca.P0, copy=True), status="preinitialized") == (trk.nTargets > n0)
        info = None
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            info = o.add_scan(float(t), z, prune_similar=scene["on"][k], prune_threshold=scene["thr"])
            trk.addMeasurementList(MeasurementList(float(t), z), pruneSimilar=scene["on"][k])
        assert trk.nx == 6
        dead = o.terminated[len(o.terminated) - len(info["dead"]):] if info["dead"] else []

        def shape(multi, L):
            assert len(multi) == 4 and (4, 106) in multi and L == 685, (scene["desc"], multi, L)
        hold_tracker(trk, o, scene["N"], scene["desc"], shape, dead)
    finally:
        trk.close()
