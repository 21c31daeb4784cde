"""Reference for the K best global hypotheses of a cluster (csrc/mht_kbest.h, mht_kbest_hypotheses): exhaustive enumeration, and an
independent plain recursive branch and bound with the same cost and order rules.  Pure Python on float64; shared by
tests/test_kbest_cpu.py and tests/test_kbest_gpu.py.

An instance is (sizes, cost, rows): sizes[t] columns per target, cost[c] per column, rows[c] an iterable of row ids (any hashable).
A hypothesis is a tuple of column offsets INSIDE their targets, one per target; its cost is the float sum of the picked costs from
0.0, left to right.  A column whose cost is not finite is never picked.  The list is sorted by (cost, tuple)."""
import itertools
import math
import os

import numpy as np

EPS = float(np.finfo(np.float64).eps)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, NODE_LIMIT, TOO_LARGE, BAD_ROWS = 0, 1, 2, 3
MAX_K, MAX_TARGETS, MAX_COLUMNS, MAX_DEPTH, MAX_ROWS = 64, 32, 1024, 16, 2048


def _starts(sizes):
    s = [0]
    for n in sizes:
        s.append(s[-1] + int(n))
    return s


def total(cost, cols):
    s = 0.0
    for c in cols:
        s = s + float(cost[c])
    return s


def combinations(sizes):
    n = 1
    for s in sizes:
        n *= int(s)
    return n


def exhaustive(sizes, cost, rows, K):
    """Every product of the groups, filtered and sorted: [(cost, tuple)] of at most K."""
    st = _starts(sizes)
    out = []
    for tup in itertools.product(*[range(int(s)) for s in sizes]):
        cols = [st[t] + o for t, o in enumerate(tup)]
        if not all(math.isfinite(float(cost[c])) for c in cols):
            continue
        seen, ok = set(), True
        for c in cols:
            for r in rows[c]:
                if r in seen:
                    ok = False
                seen.add(r)
        if ok:
            out.append((total(cost, cols), tup))
    out.sort()
    return out[:K]


def branch_and_bound(sizes, cost, rows, K):
    """Recursive depth-first search, the targets in order, a target's columns by ascending (cost, index); cut where the cheapest
    completion cannot come before the K-th entry (with an allowance of 1e-9 (1 + sum |cost|) for the two ways of summing).
    Returns ([(cost, tuple)], nodes)."""
    st = _starts(sizes)
    n = len(sizes)
    fin = [[c for c in range(st[t], st[t + 1]) if math.isfinite(float(cost[c]))] for t in range(n)]
    if any(len(f) == 0 for f in fin):
        return [], 0
    ranked = [sorted(f, key=lambda c: (float(cost[c]), c)) for f in fin]
    tail = [0.0] * (n + 1)
    for t in range(n - 1, -1, -1):
        tail[t] = tail[t + 1] + float(cost[ranked[t][0]])
    allow = 1e-9 * (1.0 + sum(abs(float(cost[c])) for f in fin for c in f))
    best, used, pick, nodes = [], set(), [], [0]

    def rec(t, s):
        if t == n:
            entry = (s, tuple(c - st[k] for k, c in enumerate(pick)))
            if len(best) < K or entry < best[-1]:
                best.append(entry)
                best.sort()
                del best[K:]
            return
        for c in ranked[t]:
            nodes[0] += 1
            if len(best) == K and (s + float(cost[c])) + tail[t + 1] > best[-1][0] + allow:
                break
            rs = set(rows[c])
            if rs & used:
                continue
            used.update(rs)
            pick.append(c)
            rec(t + 1, s + float(cost[c]))
            pick.pop()
            used.difference_update(rs)

    rec(0, 0.0)
    return best, nodes[0]


def load_recorded(name, max_targets=MAX_TARGETS, max_columns=MAX_COLUMNS, max_depth=MAX_DEPTH):
    """The recorded ILP instances of tests/golden/<name>.npz that fit the limits: dicts of sizes, cost, rows (lists per column), sel
    (the recorded optimum as global columns, ascending), obj, unique."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    out = []
    for i in range(int(g["n_inst"])):
        p = "i%03d_" % i
        ptr, rr = g[p + "col_ptr"], g[p + "col_rows"]
        rows = [[int(r) for r in rr[ptr[c]:ptr[c + 1]]] for c in range(len(ptr) - 1)]
        sizes = [int(s) for s in g[p + "sizes"]]
        if len(sizes) > max_targets or len(rows) > max_columns or max((len(r) for r in rows), default=0) > max_depth:
            continue
        out.append(dict(index=i, sizes=sizes, cost=np.asarray(g[p + "cost"], dtype=np.float64), rows=rows, sel=[int(s) for s in g[p + "sel"]],
                        obj=float(g[p + "obj"]), unique=bool(g[p + "unique"])))
    return out


def pack(instances, depth=None):
    """Several instances (sizes, cost, rows) as the clusters of ONE call of the seam: row ids relabelled per cluster in order of first
    appearance.  Returns dict(nHyp, nT, nC, depth, group_ptr, rows [depth][nHyp], cost, cluster_ptr, cluster_targets) of NumPy arrays."""
    gp, cp, ct, cost, cols = [0], [0], [], [], []
    for sizes, c, rows in instances:
        label = {}
        for s in sizes:
            ct.append(len(gp) - 1)
            gp.append(gp[-1] + int(s))
        cp.append(len(ct))
        assert len(c) == len(rows) == sum(int(s) for s in sizes)
        for col in rows:
            cols.append([label.setdefault(r, len(label)) for r in col])
        cost.extend(float(v) for v in c)
    d = max([len(c) for c in cols] + [0]) if depth is None else depth
    nHyp = len(cols)
    R = np.full((max(d, 1), max(nHyp, 1)), -1, dtype=np.int32)
    for i, col in enumerate(cols):
        R[:len(col), i] = col
    return dict(nHyp=nHyp, nT=len(ct), nC=len(cp) - 1, depth=d, group_ptr=np.asarray(gp, dtype=np.int32), rows=R,
                cost=np.asarray(cost, dtype=np.float64).reshape(-1), cluster_ptr=np.asarray(cp, dtype=np.int32),
                cluster_targets=np.asarray(ct, dtype=np.int32))


def random_instance(rng, n_targets, sizes=None, n_rows=6, depth=2, cost_levels=None, p_empty=0.2):
    """Small random cluster: cost_levels = None: continuous costs in [-5, 15); an int: that many distinct values (ties)."""
    sizes = [int(rng.integers(1, 5)) for _ in range(n_targets)] if sizes is None else list(sizes)
    n = sum(sizes)
    cost = rng.uniform(-5.0, 15.0, n) if cost_levels is None else rng.integers(0, cost_levels, n).astype(np.float64)
    rows = []
    for _ in range(n):
        k = 0 if rng.random() < p_empty else int(rng.integers(1, depth + 1))
        rows.append(sorted(set(int(r) for r in rng.integers(0, n_rows, k))))
    return sizes, cost, rows


def fold_probabilities(costs):
    """prob of a list's own costs in np.longdouble: exp(-(c - c0)) / sum."""
    c = np.asarray(costs, dtype=np.longdouble)
    w = np.exp(-(c - c[0]))
    return w / w.sum()


# ---- the cases tests/test_kbest_cpu.py runs through the host twin and tests/test_kbest_gpu.py through the seam --------------------
def expect(sizes, cost, rows, K, depth, raw_rows_bad=False):
    """(status, list) a cluster must give: the limits restated, then the branch and bound."""
    if len(sizes) > MAX_TARGETS or sum(sizes) > MAX_COLUMNS or depth > MAX_DEPTH:
        return TOO_LARGE, []
    if raw_rows_bad:
        return BAD_ROWS, []
    return OK, branch_and_bound(sizes, cost, rows, K)[0]


def _case(label, instances, K, depth=None, bad=None):
    """One call: its packed arrays and per cluster the expected (status, list).  bad = (cluster, column, value): that column's first
    row cell is overwritten with a value outside the range after packing."""
    p = pack(instances, depth)
    if bad is not None:
        first = int(p["group_ptr"][p["cluster_targets"][p["cluster_ptr"][bad[0]]]])
        p["rows"][0, first + bad[1]] = bad[2]
    want = [expect(s, c, r, K, p["depth"], bad is not None and bad[0] == i) for i, (s, c, r) in enumerate(instances)]
    return dict(label=label, packed=p, K=K, want=want, instances=instances)


def chain_instance(n=32):
    """n targets of 2 columns with distinct costs, the cheap one first or second; the cheap columns of targets t and t + 1 share a row
    where t is a multiple of 8, so the cheapest choice of every target on its own is infeasible four times over at n = 32"""
    sizes, cost, rows = [2] * n, [], []
    for t in range(n):
        pair = [-1.0 - 0.01 * t - 0.001 * (t * t % 7), -0.7 + 0.013 * t + 0.1 * (t % 5)]
        link = [[t - 1] if t % 8 == 1 else ([t] if t % 8 == 0 else []), [1000 + t]]
        if t % 2:
            pair, link = pair[::-1], link[::-1]
        cost += pair
        rows += link
    return sizes, np.asarray(cost), rows


def cases():
    """The calls, built once per process (nobody writes to them)."""
    if cases.cache is not None:
        return cases.cache
    rng = np.random.default_rng(20)
    out = []
    wave = random_instance(rng, 5, sizes=[1, 63, 64, 65, 130], n_rows=40, depth=3)
    out.append(_case("groups of 1, 63, 64, 65 and 130 columns, K 8", [wave], 8))
    out.append(_case("the same, K 64", [wave], 64))
    out.append(_case("one-target clusters", [random_instance(rng, 1, sizes=[s]) for s in (5, 1, 130, 64)], 8))
    small = [random_instance(rng, int(rng.integers(1, 5))) for _ in range(12)]
    out.append(_case("small clusters, K 1", small, 1))
    out.append(_case("small clusters, K 64 (above the feasible count)", small, 64))
    out.append(_case("infeasible next to feasible", [([1, 1], np.array([1.0, 2.0]), [[3], [3]]), small[0], ([2, 1], np.array([1.0, 2.0, 0.5]), [[0, 1], [1], [1]])], 8))
    ties = [random_instance(rng, 4, cost_levels=2, n_rows=5) for _ in range(6)] + [random_instance(rng, 3, sizes=[70, 3, 2], cost_levels=3, n_rows=30)]
    out.append(_case("equal costs: ties go by tuple", ties, 16))
    out.append(_case("equal costs, K 64", ties, 64))
    neg = [(s, -np.abs(c) - 1.0, r) for s, c, r in small[:4]]
    out.append(_case("negative costs", neg, 8))
    nf = []
    for s, c, r in [random_instance(rng, 3, sizes=[4, 5, 3]) for _ in range(4)]:
        c = c.copy()
        c[[0, 5, 10]] = [np.nan, np.inf, -np.inf]
        nf.append((s, c, r))
    nf.append(([2, 2], np.array([1.0, 2.0, np.nan, np.inf]), [[], [], [], []]))      # (a target without a finite column)
    out.append(_case("NaN and inf costs", nf, 8))
    out.append(_case("empty columns", [random_instance(rng, 4, p_empty=1.0) for _ in range(3)], 16, depth=2))
    out.append(_case("no rows at all (depth 0)", [random_instance(rng, 3, p_empty=1.0)], 8, depth=0))
    out.append(_case("32-target chain, K 8", [chain_instance(32)], 8))
    out.append(_case("32-target chain, K 64", [chain_instance(32)], 64))
    good = small[1]
    out.append(_case("33 targets next to a good cluster", [good, chain_instance(33), small[2]], 8))
    out.append(_case("1025 columns next to a good cluster", [random_instance(rng, 2, sizes=[1000, 25], n_rows=50), good], 4))
    out.append(_case("1024 columns", [random_instance(rng, 2, sizes=[1000, 24], n_rows=50)], 4))
    out.append(_case("depth 17", [good, small[3]], 8, depth=17))
    out.append(_case("a row id of 2048", [good, small[3], small[4]], 8, bad=(1, 0, MAX_ROWS)))
    out.append(_case("a row id of -2", [small[3], good], 8, bad=(0, 1, -2)))
    many_rows = ([2, 2], np.array([1.0, 2.0, 3.0, 4.5]), [list(range(0, 16)), list(range(16, 32)), list(range(8, 24)), [2047 - 0]])
    out.append(_case("depth 16", [many_rows], 8))
    cases.cache = out
    return out


cases.cache = None
SENTINEL = -7


def build_twin(directory):
    """tests/hostmath/kbest_host.cpp compiled into `directory`; the ctypes library."""
    import ctypes as C
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(str(directory), "libkbest_host.so")
    subprocess.check_call([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(root, "tests", "hostmath", "kbest_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.kbest_host.restype = C.c_int
    lib.kbest_host.argtypes = [C.c_int32] * 6 + [C.c_void_p] * 12
    lib.kbest_table_bytes_host.restype = C.c_uint64
    lib.kbest_table_bytes_host.argtypes = [C.c_int32] * 3
    lib.kbest_work_bytes_host.restype = C.c_uint64
    lib.kbest_work_bytes_host.argtypes = [C.c_int32] * 2
    return lib


def outputs(p, K):
    """The seam's host-side output arrays preset to a sentinel: count, status, nodes, hyp_cost, hyp_prob, hyp_sel, marginal."""
    nC, nT, nHyp = p["nC"], p["nT"], p["nHyp"]
    return dict(count=np.full(nC, SENTINEL, dtype=np.int32), status=np.full(nC, SENTINEL, dtype=np.int32), nodes=np.full(nC, SENTINEL, dtype=np.int32),
                hyp_cost=np.full((K, nC), float(SENTINEL)), hyp_prob=np.full((K, nC), float(SENTINEL)),
                hyp_sel=np.full((K, nT), SENTINEL, dtype=np.int32), marginal=np.full(nHyp, float(SENTINEL)))


OUT_NAMES = ("count", "status", "nodes", "hyp_cost", "hyp_prob", "hyp_sel", "marginal")


def call_twin(lib, p, K, node_limit=1 << 20):
    o = outputs(p, K)
    rc = lib.kbest_host(p["nHyp"], p["nT"], p["nC"], p["depth"], K, node_limit, *[p[k].ctypes.data for k in ("group_ptr", "rows", "cost", "cluster_ptr", "cluster_targets")],
                        *[o[k].ctypes.data for k in OUT_NAMES])
    assert rc == 0
    return o


def listed(p, o, c):
    """Cluster c's list of an output: [(cost, tuple of offsets)]"""
    tg = p["cluster_targets"][p["cluster_ptr"][c]:p["cluster_ptr"][c + 1]]
    return [(float(o["hyp_cost"][r, c]), tuple(int(o["hyp_sel"][r, t] - p["group_ptr"][t]) for t in tg)) for r in range(int(o["count"][c]))]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def hold_probabilities(label, p, o, K):
    """prob and the marginals of an output against the np.longdouble fold of ITS OWN costs: |got - truth| <= (2 K + 64) eps truth.
    Also: cells beyond count, the marginals of clusters that were not searched, no sentinel left.  Returns the worst ratio to the
    bound."""
    worst = 0.0
    bound = (2 * K + 64) * EPS
    truth_marginal = np.zeros(p["nHyp"], dtype=np.longdouble)
    unknown = np.zeros(p["nHyp"], dtype=bool)
    for c in range(p["nC"]):
        n, tg = int(o["count"][c]), p["cluster_targets"][p["cluster_ptr"][c]:p["cluster_ptr"][c + 1]]
        assert 0 <= n <= K and np.isnan(o["hyp_cost"][n:, c]).all() and np.isnan(o["hyp_prob"][n:, c]).all(), (label, c)
        assert (o["hyp_sel"][n:, tg] == -1).all(), (label, c)
        if o["status"][c] in (TOO_LARGE, BAD_ROWS):
            assert n == 0 and o["nodes"][c] == 0
            for t in tg:
                unknown[p["group_ptr"][t]:p["group_ptr"][t + 1]] = True
        if n:
            truth = fold_probabilities(o["hyp_cost"][:n, c])
            got = o["hyp_prob"][:n, c]
            worst = max(worst, float(np.max(np.abs(got - truth) / (bound * truth))))
            for r in range(n):
                truth_marginal[o["hyp_sel"][r, tg]] += truth[r]
    assert np.isnan(o["marginal"][unknown]).all() and not np.isnan(o["marginal"][~unknown]).any(), label
    m, tm = o["marginal"][~unknown], truth_marginal[~unknown]
    assert ((tm == 0) == (m == 0)).all(), label
    if (tm > 0).any():
        worst = max(worst, float(np.max(np.abs(m[tm > 0] - tm[tm > 0]) / (bound * tm[tm > 0]))))
    for k in OUT_NAMES:
        assert not (o[k] == SENTINEL).any(), (label, k)
    return worst


def hold_case(case, o):
    """An output of a case against the reference: status, count, costs and tuples bit for bit."""
    p = case["packed"]
    for c, (status, want) in enumerate(case["want"]):
        assert int(o["status"][c]) == status, (case["label"], c, int(o["status"][c]), status)
        got = listed(p, o, c)
        assert len(got) == len(want), (case["label"], c, len(got), len(want))
        for r, (g, w) in enumerate(zip(got, want)):
            assert g[1] == w[1] and same_bits(np.float64(g[0]), np.float64(w[0])), (case["label"], c, r, g, w)
