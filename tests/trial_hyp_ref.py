"""NumPy restatement of what `mht_trial_hypotheses` adds to `mht_trial_manoeuvres` (include/mht_amd.h, csrc/mht_trial_hyp.h): the
hypothesis weights of the leaves of a target and the SEGMENTED fold of a table of candidates x leaves, per target.  The cells themselves
are tests/trial_ref.py's (`cells` calls its `manoeuvres` with the leaves as the tracks), and through it tests/encounter_ref.py's.

Twice, as those files do: in float64 with the header's order of the sums -- a piece (the part of a segment inside a tile of 256 leaves)
adds its leaves serially, a target adds its pieces in tile order -- and in np.longdouble as the truth, where the order does not show.
The truth's exp is np.longdouble's."""
import numpy as np

import trial_ref

NAMES = ("pcWorst", "pcWorstLeaf", "dcpaMin", "dcpaMinLeaf", "pcMean", "pcSel", "dcpaSel", "tcpaSel")      # the seam's fig [8][G][T]
TILE = 256


def cells(x, P, Phi, Q, K, dt, R, own, Sown, w, cand, truth=False, pc_mp=False):
    """The table over [G, L]: trial_ref.manoeuvres with the leaves as its tracks"""
    return trial_ref.manoeuvres(x, P, Phi, Q, K, dt, R, own, Sown, w, cand, truth=truth, pc_mp=pc_mp)


def segments(target, T):
    """seg [T + 1] of a non-decreasing target index per leaf: the leaves of target t are seg[t] .. seg[t + 1] - 1"""
    return np.searchsorted(np.asarray(target), np.arange(T + 1)).astype(np.int32)


def weights(cnllr, seg, dtype=np.float64):
    """(w [L], weight [L]) in `dtype`: w_l = exp(-(cnllr_l - cmin_t)) with cmin_t the smallest non-NaN cnllr of the segment, NaN for a
    leaf without a cnllr; weight_l = w_l / sum(w), the sum over the leaves with a cnllr, serially in leaf order"""
    c = np.asarray(cnllr, dtype=np.float64).astype(dtype)
    w, weight = np.full(len(c), np.nan, dtype=dtype), np.full(len(c), np.nan, dtype=dtype)
    with np.errstate(all="ignore"):
        for t in range(len(seg) - 1):
            a, e = int(seg[t]), int(seg[t + 1])
            has = ~np.isnan(c[a:e])
            if not has.any():
                continue
            cmin = c[a:e][has].min()
            total = dtype(0)
            for l in range(a, e):
                if has[l - a]:
                    w[l] = np.exp(-(c[l] - cmin))
                    total = total + w[l]
            weight[a:e] = w[a:e] / total
    return w, weight


def fold(table, cnllr, seg, sel, dtype=np.float64):
    """The per-target figures of a table (dict of [G, L] arrays tcpa, dcpa, pc at least): dict of [G, T] arrays NAMES (the leaves int64)
    plus weight [L] and nLeaves [T].  The four extrema are NumPy's nanmax / nanmin with the lowest index; the sums are in `dtype`, for
    float64 in the header's order."""
    pc, dcpa, tcpa = [np.asarray(table[k], dtype=np.float64) for k in ("pc", "dcpa", "tcpa")]
    G, T = len(pc), len(seg) - 1
    w, weight = weights(cnllr, seg, dtype)
    out = {k: np.full((G, T), np.nan, dtype=dtype if k == "pcMean" else np.float64) for k in NAMES}
    out["pcWorstLeaf"], out["dcpaMinLeaf"] = np.full((G, T), -1, dtype=np.int64), np.full((G, T), -1, dtype=np.int64)
    for t in range(T):
        a, e = int(seg[t]), int(seg[t + 1])
        for g in range(G):
            for fig, name, arg, pick in ((pc, "pcWorst", "pcWorstLeaf", np.nanmax), (dcpa, "dcpaMin", "dcpaMinLeaf", np.nanmin)):
                row = fig[g, a:e]
                if e > a and not np.isnan(row).all():
                    out[name][g, t] = pick(row)
                    out[arg][g, t] = a + int(np.flatnonzero(row == out[name][g, t])[0])
            spw, sw = dtype(0), dtype(0)
            for c in range(a // TILE, (e - 1) // TILE + 1 if e > a else 0):      # the pieces in tile order
                pw, ps = dtype(0), dtype(0)
                for l in range(max(a, c * TILE), min(e, (c + 1) * TILE)):      # a piece, serially
                    if not np.isnan(pc[g, l]) and not np.isnan(w[l]):
                        pw, ps = pw + w[l] * dtype(pc[g, l]), ps + w[l]
                spw, sw = spw + pw, sw + ps
            if sw > 0:
                out["pcMean"][g, t] = spw / sw
            if sel[t] >= 0:
                out["pcSel"][g, t], out["dcpaSel"][g, t], out["tcpaSel"][g, t] = pc[g, sel[t]], dcpa[g, sel[t]], tcpa[g, sel[t]]
    out["weight"], out["nLeaves"] = weight, np.diff(seg).astype(np.int64)
    return out


EPS = float(np.finfo(np.float64).eps)


def mean_ratio(got, truth, n_leaves):
    """The largest |got - truth| / ((2 nLeaves + 64) eps truth + 2 eps) over the cells where the truth is not NaN; the NaN cells must be
    the truth's exactly (AssertionError).  n_leaves broadcasts against the cells.  The bound: every term of the two sums is >= 0, so each
    sum carries at most (n - 1) eps of relative error; a leaf more than 40 above cmin weighs under 1e-17, so the rounding of
    cnllr - cmin contributes at most 40 eps; the rest is for the library's exp, the products and the division."""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth)
    assert np.array_equal(np.isnan(got), np.isnan(truth)), "NaN cells differ from the truth's"
    n = np.broadcast_to(np.asarray(n_leaves, dtype=np.float64), truth.shape)
    live = ~np.isnan(truth)
    if not live.any():
        return 0.0
    err = np.abs(got[live].astype(np.longdouble) - truth[live])
    bound = (2 * n[live] + 64) * EPS * np.abs(truth[live]) + 2 * EPS
    return float(np.max(err / bound))


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
# The smallest shape that can go wrong: 600 leaves over three tiles.  Segment sizes, in order: 1 and 63 (a wavefront's worth together),
# 64, 65, 0 (an empty target), 63 (it ends exactly at leaf 256), 4, 300 (it starts at leaf 260, before the boundary at 512, and with the
# leaves 260 .. 559 lies in tiles 1 and 2 -- together with the segment before it tile 1 holds two pieces), 40
SIZES = (1, 63, 64, 65, 0, 63, 4, 300, 40)
# and one that spans three tiles: 258 leaves from leaf 255 on (tiles 0, 1 and 2), for the second layout
SIZES_SPAN = (255, 258, 0, 87)
NAN_SEGMENT = 6           # of SIZES: every leaf's x is NaN
NO_SELECTED = 1           # of SIZES: sel = -1 (the empty target has -1 anyway)


def make_leaves(model, sizes, seed, special=True, nan_segment=None, no_selected=None):
    """Leaves for the segment sizes given, drawn as trial_ref.make_scene draws tracks (its special entries among the first 52): (x, P,
    cnllr, target, sel, own, Sown).  With special=True: leaf 70 has a NaN in x; every leaf of segment `nan_segment` has; leaves 130 and 131
    are identical (a tie); cnllr is NaN at leaf 140 and +inf at leaf 141; the cnllr of the segment of 300 is spread over 800, so that
    weights underflow to 0 exactly; the other segments' over 12.  sel is the leaf with the smallest cnllr of each segment, -1 for segment
    `no_selected` and for an empty one."""
    rng = np.random.default_rng(seed)
    L, T = int(sum(sizes)), len(sizes)
    x, P, own, Sown = trial_ref.make_scene(model, L, seed=seed, own_cov=x_is_six(model))
    target = np.repeat(np.arange(T), sizes).astype(np.int32)
    seg = segments(target, T)
    cnllr = rng.uniform(0.0, 12.0, L) + np.repeat(rng.uniform(-50.0, 50.0, T), sizes)
    if special:
        big = int(np.argmax(sizes))
        cnllr[seg[big]:seg[big + 1]] = np.linspace(3.0, 803.0, sizes[big])[rng.permutation(sizes[big])]
        x[70, 1] = np.nan
        if nan_segment is not None:
            x[seg[nan_segment]:seg[nan_segment + 1], 0] = np.nan
        x[131], P[131] = x[130], P[130]
        cnllr[140], cnllr[141] = np.nan, np.inf
    sel = np.full(T, -1, dtype=np.int32)
    for t in range(T):
        if sizes[t] and t != no_selected:
            c = cnllr[seg[t]:seg[t + 1]]
            sel[t] = seg[t] + int(np.nanargmin(c))
    return x, P, cnllr, target, sel, own, Sown


def x_is_six(model):
    return int(np.asarray(model.C_RADAR).shape[1]) == 6
