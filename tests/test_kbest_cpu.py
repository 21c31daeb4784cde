"""CPU: the search for the K best global hypotheses of a cluster (csrc/mht_kbest.h: kbest_cluster, what the wavefront of kbest_kernel
runs for its cluster) compiled for the host (tests/hostmath/kbest_host.cpp, the 64 lanes as a loop) and held to tests/kbest_ref.py.

  1  the reference checks itself: exhaustive enumeration == branch and bound, on random small clusters and on the recorded ILP
     instances with at most 3e4 combinations; rank 0 is the recorded optimum of every g4 / g6 / g7 instance within the limits
  2  the twin against the reference on kbest_ref.cases(): status, count, costs and tuples bit for bit
  3  prob and the marginals: with the np.longdouble fold of the list's OWN costs as the truth, |got - truth| <= (2 K + 64) eps truth
     (the bound and style of property 8 of tests/test_trial_hyp_cpu.py: K terms summed in ascending rank, one exp and one division
     each, and the difference cost - cost[0] rounded once)
  4  a node limit that fires: the twin defines the partial list; it is sorted, feasible, costed correctly and nodes <= the limit
  5  what the seam refuses, the twin refuses
and what is host-only in pymht_amd: evaluation.k_best_prep against a pure-Python union-find, the docstrings, the AIS refusal.
Measured, host build (g++ -O2, glibc's exp), the worst ratio to the bound of 3 over all cases here: 0.111."""
import inspect
import os

import numpy as np
import pytest

import kbest_ref as ref


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return ref.build_twin(tmp_path_factory.mktemp("kbest_host"))


def test_reference_exhaustive_equals_branch_and_bound_on_random_clusters():
    rng = np.random.default_rng(1)
    seen_ties = 0
    for it in range(300):
        inst = ref.random_instance(rng, int(rng.integers(1, 6)), cost_levels=None if it % 3 else 3, n_rows=int(rng.integers(2, 9)))
        for K in (1, 3, 64):
            want = ref.exhaustive(*inst, K)
            got, _ = ref.branch_and_bound(*inst, K)
            assert got == want, (it, K)
            seen_ties += len(want) > 1 and want[0][0] == want[1][0]
    assert seen_ties > 20      # (the tuple order was exercised)


@pytest.mark.parametrize("name,least", [("g4_ilp", 90), ("g6_ilp_cfg3", 100), ("g7_ilp_hard", 25)])
def test_reference_on_the_recorded_instances(name, least, twin):
    """Rank 0 is the recorded optimum (all of these have unique optima); where exhaustive enumeration is affordable the whole list of
    8 equals it; and the twin gives the branch and bound's list bit for bit."""
    insts = ref.load_recorded(name)
    assert len(insts) >= least
    n_exh = 0
    for g in insts:
        inst = (g["sizes"], g["cost"], g["rows"])
        got, _ = ref.branch_and_bound(*inst, 8)
        assert g["unique"] and len(got) >= 1
        st = ref._starts(g["sizes"])
        assert [st[t] + o for t, o in enumerate(got[0][1])] == g["sel"], (name, g["index"])
        assert abs(got[0][0] - g["obj"]) <= 1e-9 * max(1.0, abs(g["obj"])), (name, g["index"])
        if ref.combinations(g["sizes"]) <= 30000:
            assert got == ref.exhaustive(*inst, 8), (name, g["index"])
            n_exh += 1
        case = ref._case("%s %d" % (name, g["index"]), [inst], 8)
        ref.hold_case(case, ref.call_twin(twin, case["packed"], 8))
    assert n_exh >= 10


def test_twin_against_the_reference_on_the_cases(twin):
    worst, seen = 0.0, set()
    for case in ref.cases():
        o = ref.call_twin(twin, case["packed"], case["K"])
        ref.hold_case(case, o)
        r = ref.hold_probabilities(case["label"], case["packed"], o, case["K"])
        print("%s: status %s, count %s, nodes %s, ratio to the bound %.3g" % (case["label"], o["status"].tolist()[:8], o["count"].tolist()[:8],
                                                                                o["nodes"].tolist()[:8], r))
        worst = max(worst, r)
        seen.update(int(s) for s in o["status"])
        assert (o["nodes"][o["status"] == ref.OK] >= 0).all()
    print("worst ratio to the bound (2 K + 64) eps: %.3g" % worst)
    assert worst <= 1.0
    assert seen == {ref.OK, ref.TOO_LARGE, ref.BAD_ROWS}


def test_cases_cover_what_they_are_meant_to():
    by = {c["label"]: c for c in ref.cases()}
    wave = by["groups of 1, 63, 64, 65 and 130 columns, K 8"]["instances"][0]
    assert wave[0] == [1, 63, 64, 65, 130]
    assert any(len(w) == 0 and s == ref.OK for s, w in by["infeasible next to feasible"]["want"])
    assert any(0 < len(w) < 64 for _, w in by["small clusters, K 64 (above the feasible count)"]["want"])
    assert any(len(w) > 1 and w[0][0] == w[1][0] for _, w in by["equal costs: ties go by tuple"]["want"])
    assert all(w[0][0] < 0 for _, w in by["negative costs"]["want"] if w)
    chain = by["32-target chain, K 64"]
    assert len(chain["instances"][0][0]) == 32 and len(set(chain["instances"][0][1].tolist())) == 64 and len(chain["want"][0][1]) == 64
    assert [s for s, _ in by["33 targets next to a good cluster"]["want"]] == [ref.OK, ref.TOO_LARGE, ref.OK]
    assert [s for s, _ in by["1025 columns next to a good cluster"]["want"]] == [ref.TOO_LARGE, ref.OK]
    assert [s for s, _ in by["1024 columns"]["want"]] == [ref.OK]
    assert [s for s, _ in by["depth 17"]["want"]] == [ref.TOO_LARGE] * 2
    assert [s for s, _ in by["a row id of 2048"]["want"]] == [ref.OK, ref.BAD_ROWS, ref.OK]
    assert [s for s, _ in by["a row id of -2"]["want"]] == [ref.BAD_ROWS, ref.OK]
    assert by["depth 16"]["packed"]["depth"] == 16 and by["depth 16"]["packed"]["rows"].max() < ref.MAX_ROWS


def test_a_node_limit_that_fires(twin):
    """The partial list is the twin's to define; it must be a sorted list of feasible hypotheses with their true costs, and the exact
    list comes back as soon as the limit is the full search's node count."""
    inst = ref.chain_instance(32)
    case = ref._case("chain", [inst, ref.random_instance(np.random.default_rng(3), 2)], 8)
    p = case["packed"]
    full = ref.call_twin(twin, p, 8)
    assert full["status"].tolist() == [ref.OK, ref.OK]
    need, small = int(full["nodes"][0]), int(full["nodes"][1])
    assert need > 1000 and 2 < small < 64
    for limit in (1, 2, 64, 200, need - 1):
        o = ref.call_twin(twin, p, 8, limit)
        assert o["status"].tolist() == [ref.NODE_LIMIT, ref.OK if limit >= small else ref.NODE_LIMIT], (limit, o["status"], o["nodes"])
        assert (0 <= o["nodes"]).all() and (o["nodes"] <= limit).all(), (limit, o["nodes"])
        ref.hold_probabilities("limit %d" % limit, p, o, 8)
        got = ref.listed(p, o, 0)
        assert got == sorted(got) and len(set(got)) == len(got)
        st = ref._starts(inst[0])
        for cst, tup in got:
            cols = [st[t] + off for t, off in enumerate(tup)]
            rows = [r for c in cols for r in inst[2][c]]
            assert len(rows) == len(set(rows)) and ref.same_bits(np.float64(cst), np.float64(ref.total(inst[1], cols)))
        if limit >= small:      # (the limit is per cluster: a neighbour that stays below it is unaffected)
            assert ref.listed(p, o, 1) == ref.listed(p, full, 1) and o["nodes"][1] == small
        if limit < 32:
            assert o["count"][0] == 0
    o = ref.call_twin(twin, p, 8, need)
    assert o["status"].tolist() == [ref.OK, ref.OK] and all(ref.same_bits(o[k], full[k]) for k in ref.OUT_NAMES)


def test_twin_refuses_what_the_seam_refuses(twin):
    case = ref.cases()[3]
    p = case["packed"]
    args = lambda **kw: [kw.get(k, v) for k, v in (("nHyp", p["nHyp"]), ("nT", p["nT"]), ("nC", p["nC"]), ("depth", p["depth"]), ("K", 8), ("limit", 100))]
    for bad in (dict(nHyp=0), dict(nT=0), dict(nC=0), dict(depth=-1), dict(K=0), dict(K=ref.MAX_K + 1), dict(limit=0)):
        o = ref.outputs(p, 8)
        rc = twin.kbest_host(*args(**bad), *[p[k].ctypes.data for k in ("group_ptr", "rows", "cost", "cluster_ptr", "cluster_targets")],
                             *[o[k].ctypes.data for k in ref.OUT_NAMES])
        assert rc == -1 and all((o[k] == ref.SENTINEL).all() for k in ref.OUT_NAMES), bad


def test_garbage_index_arrays_index_nothing(twin):
    """Cluster ranges, target indices and column ranges outside the arrays: the cluster is not searched (the sanitizer build of the
    stand-alone program covers the memory side; here: the status and that the neighbours are unaffected)."""
    case = ref.cases()[3]
    base = case["packed"]
    clean = ref.call_twin(twin, base, 4)
    for name, idx, val in (("cluster_ptr", 1, -5), ("cluster_ptr", 2, 10 ** 6), ("cluster_targets", 0, -1), ("cluster_targets", 0, base["nT"]),
                           ("group_ptr", 1, -3), ("group_ptr", 1, 10 ** 6)):
        p = dict(base)
        p[name] = base[name].copy()
        p[name][idx] = val
        o = ref.call_twin(twin, p, 4)
        assert ref.TOO_LARGE in o["status"].tolist(), (name, idx, val)
        assert o["status"][-1] == ref.OK and ref.listed(p, o, base["nC"] - 1) == ref.listed(base, clean, base["nC"] - 1)


def _union_find_clusters(target, rows):
    parent = {}

    def find(a):
        while parent.setdefault(a, a) != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    T = int(max(target)) + 1
    for t in range(T):
        find(("t", t))
    for t, rr in zip(target, rows):
        for r in rr:
            if r >= 0:
                parent[find(("t", int(t)))] = find(("k", int(r)))
    groups = {}
    for t in range(T):
        groups.setdefault(find(("t", t)), []).append(t)
    return sorted(groups.values(), key=lambda g: g[0])


def test_evaluation_prep_against_a_union_find():
    from pymht_amd import evaluation
    rng = np.random.default_rng(5)
    for it in range(60):
        T = int(rng.integers(1, 12))
        target = np.sort(np.concatenate([np.arange(T) if it % 2 else np.zeros(0, dtype=np.int64), rng.integers(0, T, int(rng.integers(1, 30)))])).astype(np.int32)
        D = int(rng.integers(1, 4))
        rows = np.where(rng.random((len(target), D)) < 0.4, -1, rng.integers(0, 10 ** 9 if it % 3 == 0 else 2 * T, (len(target), D)) * (1 if it % 3 else 7))
        gp, cp, ct, local = evaluation.k_best_prep(target, rows)
        nT = int(target[-1]) + 1
        assert gp.dtype == cp.dtype == ct.dtype == local.dtype == np.int32 and local.shape == (D, len(target))
        assert gp.tolist() == [int(np.sum(target < t)) for t in range(nT + 1)]
        got = [ct[cp[c]:cp[c + 1]].tolist() for c in range(len(cp) - 1)]
        assert got == _union_find_clusters(target.tolist(), rows.tolist()), it
        # the relabelling: -1 kept; inside a cluster a bijection between its keys and 0 .. n - 1 that keeps their order
        assert ((local.T == -1) == (rows == -1)).all()
        cluster_of = np.empty(nT, dtype=np.int64)
        for c, tg in enumerate(got):
            cluster_of[tg] = c
        for c in range(len(got)):
            m = (cluster_of[target] == c)[:, None] & (rows >= 0)
            keys, ids = rows[m], local.T[m]
            uniq = np.unique(keys)
            assert np.array_equal(ids, np.searchsorted(uniq, keys)), (it, c)


def test_empty_input_needs_no_device():
    from pymht_amd import evaluation
    out = evaluation.k_best_hypotheses(np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros((0, 3), dtype=np.int32), 5)
    assert out["clusters"] == [] and out["cost"].shape == (0, 5) and out["prob"].shape == (0, 5) and out["selection"].shape == (5, 0)
    assert all(len(out[k]) == 0 for k in ("count", "status", "nodes", "leafProbability"))
    for bad in (dict(k=0), dict(k=65), dict(k=True), dict(nodeLimit=0), dict(nodeLimit=2 ** 31)):
        kw = dict(k=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            evaluation.k_best_hypotheses(np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros((0, 3), dtype=np.int32), **kw)
    with pytest.raises(ValueError):
        evaluation.k_best_hypotheses(np.zeros(2), np.array([1, 0]), np.zeros((2, 1), dtype=np.int32), 5)
    with pytest.raises(ValueError):
        evaluation.k_best_hypotheses(np.zeros(2), np.array([0, 1]), np.full((2, 1), -2, dtype=np.int32), 5)


def test_docstrings_state_the_three_caveats():
    from pymht_amd import evaluation
    from pymht_amd.tracker import Tracker
    doc = " ".join(inspect.getdoc(Tracker.getGlobalHypotheses).split())
    assert "CURRENT LEAVES, AFTER PRUNING" in doc and "rank 0 may be CHEAPER than the tracker's own selection" in doc
    assert "TRUNCATED to the k listed hypotheses" in doc and "flagged, not guessed" in doc
    assert "finer than the scan's gating clusters" in doc and "NotImplementedError" in doc
    ev = " ".join(inspect.getdoc(evaluation.k_best_hypotheses).split())
    assert "FINER than the scan's gating clusters" in ev and "truncated" in ev and "flagged, not guessed" in ev
    assert "no device call" in ev
    readme = open(os.path.join(os.path.dirname(os.path.dirname(ref.GOLD)), "README.md")).read()
    assert "getGlobalHypotheses" in readme and "truncated to the k listed" in " ".join(readme.split())


def test_ais_aided_tracker_refuses():
    from pymht_amd.tracker import Tracker

    class Stub:
        _ais = True
    with pytest.raises(NotImplementedError):
        Tracker.getGlobalHypotheses(Stub())
    with pytest.raises(NotImplementedError):
        Tracker.leafRows(Stub())
