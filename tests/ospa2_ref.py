"""The yardstick of the OSPA(2) tests (tests/test_ospa2_cpu.py, test_ospa2_gpu.py, test_ospa2_resources.py): OSPA(2) (Beard, Vo, Vo
2020) of one window -- OSPA between the set of tracks and the set of truth trajectories with the time-averaged cut-off distance as the
base distance -- in NumPy float64 exactly as include/mht_amd.h defines it, scipy.optimize.linear_sum_assignment on D^p with the pairs
that are no edges dropped, the figures of that assignment evaluated in np.longdouble from the float64 inputs as the truth; a brute force
over all partial assignments for at most 5 a side; the scenes the tests share; and the criterion.

    members   present at one or more steps of the window [lo, hi]; n_w, m_w of them, N = max(n_w, m_w)
    D_ij      over the U steps at which at least one of i, j is present: near = both present and d < c, else far;
              no near step: D = c, no edge; else D = (c nFar + sum of the near d) / U, an edge iff D < c
    total     min over one-to-one assignments on edges of  sum D^p + c^p (N - nAssigned);  loc = sum D^p over the assigned pairs

Criterion (derived from the operation count, not measured).  Every term is non-negative.  d carries 3 roundings (the differences one
each, which the square doubles, the squares and their sum, halved by the root, and the root's own); the sum of at most W near d adds
W - 1, c nFar one, its sum with the near part one, the division one: a base distance is within W + 5 <= W + 6 roundings.  Its square
doubles that and adds one; a sum of k such terms adds k - 1; c^p (N - k) carries two and its sum with loc one:
    |loc - loc_true| <= (nAssigned + 2 W + 12) eps64 loc_true        |total - total_true| <= (nAssigned + 2 W + 14) eps64 total_true
the counts are exact, and where the optimum is unique the match is the reference's.  reference() asserts D <= (1 - 1e-9) c for every
pair with a near step: a scene where the edge test could go either way by rounding fails loudly instead of being compared."""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment

import gospa_ref

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
SPACING = gospa_ref.SPACING
C_SCENE, SIGMA, K_SCENE = 20.0, 2.5, 16


def as_run(trkXY, trkOn, truXY, truOn):
    trkXY, truXY = np.asarray(trkXY, dtype=np.float64), np.asarray(truXY, dtype=np.float64)
    trkOn, truOn = np.asarray(trkOn).astype(bool), np.asarray(truOn).astype(bool)
    K = len(trkOn)
    return trkXY.reshape(K, -1, 2), trkOn.reshape(K, -1), truXY.reshape(K, -1, 2), truOn.reshape(K, -1)


def base_distances(trkXY, trkOn, truXY, truOn, lo, hi, c, dtype=np.float64):
    """(member tracks, member truths, D [n_w, m_w], nNear [n_w, m_w]) of the window, vectorised; the near steps are always decided in
    float64 (they are part of the definition), the arithmetic on them runs in dtype."""
    X, onX, Y, onY = trkXY[lo:hi + 1], trkOn[lo:hi + 1], truXY[lo:hi + 1], truOn[lo:hi + 1]
    ti, tj = np.flatnonzero(onX.any(axis=0)), np.flatnonzero(onY.any(axis=0))
    X, onX, Y, onY = X[:, ti], onX[:, ti], Y[:, tj], onY[:, tj]
    X, Y = np.where(onX[:, :, None], X, 0.0), np.where(onY[:, :, None], Y, 0.0)      # (a position whose flag is 0 is never read)

    def dist(dt):
        dx, dy = Y[:, None, :, 0].astype(dt) - X[:, :, None, 0].astype(dt), Y[:, None, :, 1].astype(dt) - X[:, :, None, 1].astype(dt)
        return np.sqrt(dx * dx + dy * dy)
    both, either = onX[:, :, None] & onY[:, None, :], onX[:, :, None] | onY[:, None, :]
    near = both & (dist(np.float64) < c)
    U, nNear = either.sum(axis=0), near.sum(axis=0)
    s = np.where(near, dist(dtype), dtype(0)).sum(axis=0, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        D = np.where(nNear > 0, (dtype(c) * (U - nNear).astype(dtype) + s) / np.maximum(U, 1).astype(dtype), dtype(c))
    return ti, tj, D, nNear


def _figures(run, lo, hi, c, p, ti, tj, pairs):
    """The window's figures for a list of assigned (member track, member truth) pairs, in np.longdouble."""
    _, _, D, _ = base_distances(*run, lo, hi, c, dtype=LD)
    loc = LD(0)
    for a, b in pairs:
        loc += D[a, b] ** p
    N, k = max(len(ti), len(tj)), len(pairs)
    match = np.full(run[1].shape[1], -2, dtype=np.int32)
    match[ti] = -1
    for a, b in pairs:
        match[ti[a]] = tj[b]
    return {"total": loc + LD(c) ** p * (N - k), "loc": loc, "nAssigned": k, "nTracks": len(ti), "nTruths": len(tj), "match": match}


def reference(trkXY, trkOn, truXY, truOn, lo, hi, c, p=2):
    """OSPA(2) of the window [lo, hi]: total and loc (np.longdouble), nAssigned, nTracks, nTruths, match [n], and D, the float64 matrix
    of the members' base distances."""
    run = as_run(trkXY, trkOn, truXY, truOn)
    ti, tj, D, nNear = base_distances(*run, lo, hi, c)
    assert (D[nNear > 0] <= (1 - 1e-9) * c).all(), "a base distance within rounding of the cut-off: the edge test is not decidable"
    assert (D[nNear == 0] == c).all()
    edge = (nNear > 0) & (D < c)
    pairs = []
    if D.size:
        rows, cols = linear_sum_assignment(D ** p)
        pairs = [(int(a), int(b)) for a, b in zip(rows, cols) if edge[a, b]]
    out = _figures(run, lo, hi, c, p, ti, tj, pairs)
    out["D"], out["edge"] = D, edge
    return out


def brute(trkXY, trkOn, truXY, truOn, lo, hi, c, p=2):
    """The minimum over ALL partial assignments on edges, by enumeration (at most 5 members a side): the total, float64."""
    ti, tj, D, nNear = base_distances(*as_run(trkXY, trkOn, truXY, truOn), lo, hi, c)
    edge = (nNear > 0) & (D < c)
    n, m = D.shape
    assert n <= 5 and m <= 5
    N, best = max(n, m), np.inf
    for k in range(min(n, m) + 1):
        for rows in itertools.combinations(range(n), k):
            for cols in itertools.permutations(range(m), k):
                if all(edge[a, b] for a, b in zip(rows, cols)):
                    best = min(best, sum(D[a, b] ** p for a, b in zip(rows, cols)) + c ** p * (N - k))
    return best


def bounds(want, W):
    k = want["nAssigned"]
    return (k + 2 * W + 12) * EPS * want["loc"], (k + 2 * W + 14) * EPS * want["total"]


def hold(got, want, W, label="", match=True):
    """The criterion on one window of W steps: got = (total, loc, nAssigned, nTracks, nTruths, match) against reference()'s dict."""
    total, loc, n_a, n_w, m_w, mt = got
    e_loc, e_tot = abs(LD(loc) - want["loc"]), abs(LD(total) - want["total"])
    b_loc, b_tot = bounds(want, W)
    if label:
        print("%s: total %.17g loc %.17g k %d (%d x %d) | err loc %.3g (bound %.3g) total %.3g (bound %.3g)"
              % (label, total, loc, want["nAssigned"], want["nTracks"], want["nTruths"], e_loc, b_loc, e_tot, b_tot))
    assert (int(n_a), int(n_w), int(m_w)) == (want["nAssigned"], want["nTracks"], want["nTruths"]), (label, n_a, n_w, m_w, want)
    assert np.isfinite(loc) and np.isfinite(total) and e_loc <= b_loc and e_tot <= b_tot, (label, total, loc, want)
    if match:
        assert np.array_equal(np.asarray(mt), want["match"]), (label, mt, want["match"])
    else:
        mt = np.asarray(mt)
        assert np.array_equal(mt == -2, want["match"] == -2) and (mt >= 0).sum() == want["nAssigned"], (label, mt, want["match"])


def sliding(K, W, every=1):
    """[(lo, hi)] of the sliding windows of at most W steps that end at steps 0, every, 2 every, ..."""
    return [(max(0, hi - W + 1), hi) for hi in range(0, K, every)]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def poison(XY, on):
    """NaN at the cells whose flag is 0"""
    XY = np.array(XY, dtype=np.float64)
    XY[~np.asarray(on).astype(bool)] = np.nan
    return XY


def tracker_scene(T, seed, K=K_SCENE):
    """A tracker-like run: T targets at cfg3's density moving at up to 5 a step over K steps, 20 % born late and 20 % dead early; 10 % of
    them untracked, the others tracked at sigma 2.5 while present, 30 % of the tracks cut into two fragments (two tracks), 10 % of the
    steps inside tracks dropped, plus T // 10 false tracks of three steps; the tracks shuffled, NaN where a flag is 0.
    (trkXY [K, n, 2], trkOn [K, n], truXY [K, T, 2], truOn [K, T])"""
    rng = np.random.default_rng(seed)
    side = SPACING * np.sqrt(T)
    steps = np.arange(K)
    truXY = rng.uniform(0.0, side, size=(1, T, 2)) + steps[:, None, None] * rng.uniform(-5.0, 5.0, size=(1, T, 2))
    first, last = np.zeros(T, dtype=int), np.full(T, K - 1)
    late, early = rng.uniform(size=T) < 0.2, rng.uniform(size=T) < 0.2
    first[late] = rng.integers(1, K // 2, size=int(late.sum()))
    last[early] = rng.integers(K // 2, K - 1, size=int(early.sum()))
    truOn = (steps[:, None] >= first[None, :]) & (steps[:, None] <= last[None, :])
    tracked = np.ones(T, dtype=bool)
    tracked[rng.choice(T, size=(T + 9) // 10, replace=False)] = False
    cols_xy, cols_on = [], []
    for j in np.flatnonzero(tracked):
        xy = truXY[:, j] + rng.normal(0.0, SIGMA, size=(K, 2))
        on = truOn[:, j] & (rng.uniform(size=K) >= 0.1)
        if rng.uniform() < 0.3 and last[j] > first[j]:
            cut = rng.integers(first[j] + 1, last[j] + 1)
            parts = [on & (steps < cut), on & (steps >= cut)]
        else:
            parts = [on]
        for part in parts:
            cols_xy.append(xy)
            cols_on.append(part)
    for _ in range(T // 10):
        t0 = rng.integers(0, K - 2)
        cols_xy.append(np.broadcast_to(rng.uniform(0.0, side, size=(1, 2)), (K, 2)) + rng.normal(0.0, SIGMA, size=(K, 2)))
        cols_on.append((steps >= t0) & (steps < t0 + 3))
    order = rng.permutation(len(cols_xy))
    trkXY = np.stack([cols_xy[i] for i in order], axis=1)
    trkOn = np.stack([cols_on[i] for i in order], axis=1)
    return poison(trkXY, trkOn), trkOn.astype(np.uint8), poison(truXY, truOn), truOn.astype(np.uint8)


def random_run(rng, n, m, K, field=30.0, p_on=0.7):
    """n tracks and m truths uniform over a field at every step, random flags, NaN where a flag is 0"""
    trkOn, truOn = rng.uniform(size=(K, n)) < p_on, rng.uniform(size=(K, m)) < p_on
    return (poison(rng.uniform(0.0, field, size=(K, n, 2)), trkOn), trkOn.astype(np.uint8),
            poison(rng.uniform(0.0, field, size=(K, m, 2)), truOn), truOn.astype(np.uint8))


def split_track():
    """The issue's first known answer: one truth over 20 steps, two tracks with exact positions at steps 0-9 and 10-19"""
    K = 20
    truXY = np.stack([np.arange(K) * 3.0, np.arange(K) * 1.5], axis=1).reshape(K, 1, 2)
    trkOn = np.stack([np.arange(K) < 10, np.arange(K) >= 10], axis=1)
    return poison(np.repeat(truXY, 2, axis=1), trkOn), trkOn.astype(np.uint8), truXY, np.ones((K, 1), dtype=np.uint8)


def shape_runs():
    """(label, run, c) with member counts of 0, 1, 63, 64, 65 and 130 on either side, in both orientations, over K = 5 steps on a field
    where a good share of the pairs are edges; every object is present at some step, so the counts are the sizes."""
    rng = np.random.default_rng(12)
    out = []
    for n, m in ((0, 0), (0, 3), (3, 0), (1, 1), (1, 64), (64, 1), (63, 64), (64, 63), (64, 64), (65, 64), (64, 65), (130, 65), (63, 130), (130, 130)):
        field = 12.0 * np.sqrt(max(n, m, 1))
        run = list(random_run(rng, n, m, 5, field=field, p_on=0.8))
        for XY, on in ((run[0], run[1]), (run[2], run[3])):      # (everybody present at step 2)
            XY[2] = np.where(on[2][:, None] != 0, XY[2], rng.uniform(0.0, field, size=XY[2].shape))
            on[2] = 1
        out.append(("%dx%d" % (n, m), tuple(run), 15.0))
    return out
