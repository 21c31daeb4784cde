"""The yardstick of the GOSPA tests (tests/test_gospa_cpu.py, test_gospa_gpu.py): GOSPA with alpha = 2 (Rahmathullah, Garcia-Fernandez,
Svensson 2017) of one step by scipy.optimize.linear_sum_assignment on min(d, c)^p with the cut-off pairs dropped, the localisation
error of that assignment evaluated in np.longdouble as the truth; a brute force over all partial assignments for small sets; the
scenes the tests share; and the criterion.

    d_ij = sqrt(dx dx + dy dy) in float64; a pair may be assigned only if d_ij < c
    total = min over partial assignments of  sum d_ij^p + c^p / 2 (n + m - 2 |assigned|)

Criterion (derived, not measured): every term of loc is non-negative, so any float64 summation order is within (k - 1) roundings of the
exact sum, plus at most 4 per term for the subtractions, products and root:
    |loc - loc_true| <= (nAssigned + 8) eps64 loc_true        |total - total_true| <= (nAssigned + 10) eps64 total_true
the counts are exact, and on inputs without ties the match is the reference's."""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


def distances(X, Y):
    X, Y = np.asarray(X, dtype=np.float64).reshape(-1, 2), np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    dx, dy = X[:, None, 0] - Y[None, :, 0], X[:, None, 1] - Y[None, :, 1]
    return np.sqrt(dx * dx + dy * dy)


def _figures(X, Y, c, p, pairs):
    """The step's figures for a given list of assigned (estimate, truth) pairs, in np.longdouble."""
    X, Y = np.asarray(X, dtype=np.float64).reshape(-1, 2), np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    n, m, k = len(X), len(Y), len(pairs)
    loc = LD(0)
    for i, j in pairs:
        dx, dy = LD(X[i, 0]) - LD(Y[j, 0]), LD(X[i, 1]) - LD(Y[j, 1])
        d2 = dx * dx + dy * dy
        loc += d2 if p == 2 else np.sqrt(d2)
    cp = LD(c) ** p
    match = np.full(n, -1, dtype=np.int32)
    for i, j in pairs:
        match[i] = j
    return {"total": loc + cp / 2 * (n + m - 2 * k), "loc": loc, "nAssigned": k, "nMissed": m - k, "nFalse": n - k, "match": match}


def reference(X, Y, c, p=2):
    """GOSPA of one step: total and loc (np.longdouble), the counts and match [n] (the truth of every estimate or -1)."""
    d = distances(X, Y)
    pairs = []
    if d.size:
        rows, cols = linear_sum_assignment(np.minimum(d, c) ** p)
        pairs = [(int(i), int(j)) for i, j in zip(rows, cols) if d[i, j] < c]
    return _figures(X, Y, c, p, pairs)


def brute(X, Y, c, p=2):
    """The minimum over ALL partial assignments with d < c, by enumeration (sets of at most 5): the total, float64."""
    d = distances(X, Y)
    n, m = d.shape
    assert n <= 5 and m <= 5
    best = np.inf
    for k in range(min(n, m) + 1):
        for rows in itertools.combinations(range(n), k):
            for cols in itertools.permutations(range(m), k):
                if all(d[i, j] < c for i, j in zip(rows, cols)):
                    best = min(best, sum(d[i, j] ** p for i, j in zip(rows, cols)) + c ** p / 2.0 * (n + m - 2 * k))
    return best


def hold(got, want, label="", match=True):
    """The criterion on one step: got = (total, loc, nAssigned, nMissed, nFalse, match) against reference()'s dict."""
    total, loc, n_a, n_m, n_f, mt = got
    k = want["nAssigned"]
    e_loc, e_tot = abs(LD(loc) - want["loc"]), abs(LD(total) - want["total"])
    b_loc, b_tot = (k + 8) * EPS * want["loc"], (k + 10) * EPS * want["total"]
    if label:
        print("%s: total %.17g loc %.17g k %d | err loc %.3g (bound %.3g) total %.3g (bound %.3g)" % (label, total, loc, k, e_loc, b_loc, e_tot, b_tot))
    assert (int(n_a), int(n_m), int(n_f)) == (k, want["nMissed"], want["nFalse"]), (label, n_a, n_m, n_f, want)
    assert np.isfinite(loc) and np.isfinite(total) and e_loc <= b_loc and e_tot <= b_tot, (label, total, loc, want)
    if match:
        assert np.array_equal(np.asarray(mt), want["match"]), (label, mt, want["match"])


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
C_SCENE, SIGMA = 20.0, 2.5
SPACING = 317.0      # side of the square a target has to itself: the density of scenario.CONFIGS cfg3 / cfg5 (1 target per 1e5 m^2)


def sparse_scene(T, seed):
    """A tracker-like step: T targets uniform over a square of cfg3's density; 10 % of them have no estimate, the others one at
    sigma 2.5 from the target, plus 10 % T false estimates uniform over the square; the estimates shuffled.  (estimates, truths)"""
    rng = np.random.default_rng(seed)
    side = SPACING * np.sqrt(T)
    Y = rng.uniform(0.0, side, size=(T, 2))
    seen = np.ones(T, dtype=bool)
    seen[rng.choice(T, size=T // 10, replace=False)] = False
    X = np.concatenate([Y[seen] + rng.normal(0.0, SIGMA, size=(int(seen.sum()), 2)), rng.uniform(0.0, side, size=(T // 10, 2))])
    rng.shuffle(X, axis=0)
    return X, Y


def dense_scene(n=137, m=130, seed=5):
    """n estimates and m truths all inside one cut-off (a disc of diameter 0.9 c): every pair is an edge."""
    rng = np.random.default_rng(seed)

    def disc(k):
        r, th = 0.45 * C_SCENE * np.sqrt(rng.uniform(size=k)), rng.uniform(0.0, 2.0 * np.pi, size=k)
        return np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    return disc(n), disc(m)


def random_sets(rng, n, m, field=30.0):
    return rng.uniform(0.0, field, size=(n, 2)), rng.uniform(0.0, field, size=(m, 2))


def shape_cases():
    """(label, estimates, truths, c) of the set sizes both test files run: a side of 0, 1, 63, 64, 65 or 130 objects (the lane stride
    of a sweep, more than two columns per lane), n > m and m > n, on a field where a good share of the pairs are edges."""
    rng = np.random.default_rng(11)
    out = []
    for n, m in ((0, 0), (0, 3), (3, 0), (1, 1), (1, 64), (63, 64), (64, 63), (64, 64), (65, 64), (64, 65), (130, 65), (63, 130), (130, 130)):
        X, Y = random_sets(rng, n, m, field=12.0 * np.sqrt(max(n, m, 1)))
        out.append(("%dx%d" % (n, m), X, Y, 15.0))
    return out
