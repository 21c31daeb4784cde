"""Scoring a tracking result against ground truth on the device: GOSPA per step (`mht_gospa_steps`, include/mht_amd.h).

The figures of pymht_amd.smoothing (log-likelihood, NIS, the likelihood surface, the innovation sequence) need no ground truth and
say whether the FILTER is tuned; they cannot say whether the tracker found the targets.  GOSPA (generalised optimal sub-pattern
assignment, Rahmathullah, Garcia-Fernandez and Svensson 2017, alpha = 2) can: at each step one distance between the set of estimates
and the set of true positions, which splits exactly into a localisation error, a missed-target cost and a false-track cost,

    total = min over partial one-to-one assignments of  sum d_ij^p + c^p / 2 (n + m - 2 |assigned|),     gospa = total^(1/p)

with d_ij = |x_i - y_j| and only pairs with d_ij < c (strictly) assignable.  A step is an optimal assignment, the steps of a run do
not depend on each other: `gospa_steps` packs them, uploads once and solves all of them in ONE launch, one step per workgroup
(csrc/mht_gospa.hip).  There is no host fallback.  `id_switches` counts track switches from the per-step matches on the host, and
`Tracker.getGospa` scores a tracker's track histories against a scenario's truth.

Per-step GOSPA says whether the targets were found at each step, not whether they were KEPT: every step is assigned on its own, so a
track cut into two fragments scores like an unbroken one.  `ospa2_windows` scores whole tracks against whole truth trajectories, OSPA(2)
(Beard, Vo, Vo 2020) over windows of steps (`mht_ospa2_windows`, csrc/mht_ospa2.hip), and `Tracker.getOspa2` applies it to a tracker's
histories.

Neither says whether the COVARIANCE the tracker reports is honest.  `nees_nodes` takes the estimation error of every node against the
true state and its normalised square e' P^-1 e (NEES) -- over the position, over position and velocity and over the full state, from
one factorisation (`mht_nees_nodes`, csrc/mht_nees.hip) -- which sees the unmeasured states the innovation tests of
pymht_amd.smoothing.consistency cannot; `nees_consistency` runs the chi-square tests of the literature on the figures, on the host,
and `Tracker.getNees` applies both to a tracker's filtered or smoothed histories under GOSPA's pairing."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .device import Context

GOSPA_MAX_SET = 2048      # objects of one step on either side (csrc/mht_gospa.h)


def _check_cutoff(c, p):
    if isinstance(p, bool) or p not in (1, 2):
        raise ValueError("gospa: p must be 1 or 2 (got %r)" % (p,))
    if isinstance(c, bool) or not isinstance(c, (int, float, np.integer, np.floating)) or not np.isfinite(c) or not c > 0:
        raise ValueError("gospa: the cut-off c must be a finite positive number (got %r)" % (c,))
    c, p = float(c), int(p)
    cp = c * c if p == 2 else c
    if not np.isfinite(cp) or not cp > 0:
        raise ValueError("gospa: c^p must be a finite positive float64 (c = %r, p = %d)" % (c, p))
    return c, p


def _positions(sets, what):
    """Per step a contiguous [k, 2] float64 array of the first two columns; ValueError for a shape that has none or a value that is
    not finite."""
    out = []
    for s, a in enumerate(sets):
        a = np.asarray(a, dtype=np.float64)
        if a.size == 0:
            a = np.zeros((0, 2))
        if a.ndim != 2 or a.shape[1] < 2:
            raise ValueError("gospa: the %s of step %d are not a [k, >= 2] array (shape %r)" % (what, s, a.shape))
        a = np.ascontiguousarray(a[:, 0:2])
        if not np.isfinite(a).all():
            raise ValueError("gospa: the %s of step %d hold a value that is not finite" % (what, s))
        if len(a) > GOSPA_MAX_SET:
            raise ValueError("gospa: step %d has %d %s, at most %d fit" % (s, len(a), what, GOSPA_MAX_SET))
        out.append(a)
    return out


def truth_steps(truth):
    """(times [K] float64, positions per time) from either form `Tracker.getGospa` takes: a sequence of (time, positions), or a pair
    (times, positions per time) -- told apart by the first entry, which is a 1-D array of numbers only in the pair."""
    if len(truth) == 2:
        try:
            times = np.asarray(truth[0], dtype=np.float64)
        except (ValueError, TypeError):      # (a (time, positions) entry is ragged)
            times = None
        if times is not None and times.ndim == 1 and not np.isscalar(truth[1]) and len(truth[1]) == len(times):
            return times, list(truth[1])
    for s, entry in enumerate(truth):
        if len(entry) != 2 or np.ndim(entry[0]) != 0:
            raise ValueError("gospa: entry %d of the truth is not (time, positions)" % s)
    return np.array([float(t) for t, _ in truth], dtype=np.float64), [y for _, y in truth]


def gospa_steps(est, truth, c, p=2, device=0, ctx=None):
    """GOSPA of every step of a run.

    est, truth   sequences of equal length, one [k, 2] array per step: the estimated and the true positions (arrays with more columns
                 are allowed, only the first two are read; empty arrays are allowed; at most 2048 objects a side and step)
    c, p         the cut-off (finite, positive) and the exponent (1 or 2)
    device, ctx  the GPU ordinal, or an existing pymht_amd.device.Context (a Tracker's) to run on
    ValueError for a value that is not finite, a length mismatch, a bad c or p -- before any device is needed.
    Returns a dict of arrays over the steps:
        total          the minimum above;  gospa = total^(1/p)
        localisation   sum d^p over the assigned pairs
        missed, false  c^p / 2 nMissed, c^p / 2 nFalse          (total = localisation + missed + false)
        nAssigned, nMissed, nFalse     int32; nAssigned + nMissed truths, nAssigned + nFalse estimates
    and `match`, a list of int32 arrays per step: the truth (its row in the step's array) assigned to every estimate, or -1.
    A pair at d == c exactly is not assigned.  One upload, one launch (`mht_gospa_steps`), no host fallback; RuntimeError should a
    step's search run into its iteration bound."""
    c, p = _check_cutoff(c, p)
    if len(est) != len(truth):
        raise ValueError("gospa: %d steps of estimates and %d steps of truth" % (len(est), len(truth)))
    X, Y = _positions(est, "estimates"), _positions(truth, "truths")
    n_steps = len(X)
    cp = c * c if p == 2 else c
    if n_steps == 0:
        e = np.zeros(0)
        i = np.zeros(0, dtype=np.int32)
        return {"gospa": e, "total": e.copy(), "localisation": e.copy(), "missed": e.copy(), "false": e.copy(), "nAssigned": i,
                "nMissed": i.copy(), "nFalse": i.copy(), "match": []}
    est_off = np.zeros(n_steps + 1, dtype=np.int64)
    tru_off = np.zeros(n_steps + 1, dtype=np.int64)
    np.cumsum([len(a) for a in X], out=est_off[1:])
    np.cumsum([len(a) for a in Y], out=tru_off[1:])
    n_est, n_tru = int(est_off[-1]), int(tru_off[-1])
    if max(n_est, n_tru) >= 2 ** 31:
        raise ValueError("gospa: %d estimates and %d truths in one call, the offsets are 32-bit" % (n_est, n_tru))
    est_off, tru_off = est_off.astype(np.int32), tru_off.astype(np.int32)
    own = ctx is None
    if own:
        ctx = Context(device)
    try:
        dev, lib = ctx.device, ctx.lib
        xy = torch.from_numpy(np.concatenate(X + Y, axis=0).reshape(-1)).to(dev)      # the one upload: estimates, then truths
        step_d = torch.empty((n_steps, 2), dtype=torch.float64, device=dev)
        count_d = torch.empty((n_steps, 3), dtype=torch.int32, device=dev)
        match_d = torch.empty(max(n_est, 1), dtype=torch.int32, device=dev)
        need = int(lib.mht_gospa_work_bytes(n_steps, n_est, n_tru))
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()      # (the upload ran on torch's stream)
        _lib.check(lib.mht_gospa_steps(ctx.handle, n_steps, est_off.ctypes.data_as(C.c_void_p), xy.data_ptr(),
                                       tru_off.ctypes.data_as(C.c_void_p), xy.data_ptr() + 16 * n_est, c, p, step_d.data_ptr(),
                                       count_d.data_ptr(), match_d.data_ptr(), work.data_ptr(), need), lib)
        step, count, match = step_d.cpu().numpy(), count_d.cpu().numpy(), match_d.cpu().numpy()
    finally:
        if own:
            ctx.close()
    bad = np.flatnonzero(~np.isfinite(step[:, 0]))
    if len(bad):
        raise RuntimeError("gospa: the assignment search of step %d ran into its iteration bound (%d estimates, %d truths)"
                           % (bad[0], len(X[bad[0]]), len(Y[bad[0]])))
    total = step[:, 0].copy()
    return {"gospa": total if p == 1 else np.sqrt(total), "total": total, "localisation": step[:, 1].copy(),
            "missed": cp / 2.0 * count[:, 1], "false": cp / 2.0 * count[:, 2],
            "nAssigned": count[:, 0].copy(), "nMissed": count[:, 1].copy(), "nFalse": count[:, 2].copy(),
            "match": [match[est_off[s]:est_off[s + 1]].copy() for s in range(n_steps)]}


def id_switches(match, estIds, truthIds=None):
    """Track switches of a run, host only: for each truth identity the number of times the identity of the estimate assigned to it
    differs from the identity of the estimate it was LAST assigned to (steps at which the truth is unassigned are skipped over:
    losing a target and finding it again under the same identity is no switch).

    match      per step an int array over the step's estimates: the truth (row of the step's truth array) or -1 (`gospa_steps`)
    estIds     per step the identities of the step's estimates (any hashable, e.g. track IDs), the same lengths as `match`
    truthIds   per step the identities of the step's truths indexed by row; default: a truth's identity is its row index
    Returns (total, perTruth): the sum, and a dict truth identity -> switches over the identities that were ever assigned."""
    if len(match) != len(estIds) or (truthIds is not None and len(truthIds) != len(match)):
        raise ValueError("id_switches: match, estIds and truthIds must have one entry per step")
    last, per = {}, {}
    for s, (mt, ids) in enumerate(zip(match, estIds)):
        mt = np.asarray(mt).reshape(-1)
        if len(mt) != len(ids):
            raise ValueError("id_switches: step %d has %d matches and %d estimate identities" % (s, len(mt), len(ids)))
        for e in np.flatnonzero(mt >= 0):
            row = int(mt[e])
            who = row if truthIds is None else truthIds[s][row]
            eid = ids[int(e)]
            per.setdefault(who, 0)
            if who in last and last[who] != eid:
                per[who] += 1
            last[who] = eid
    return sum(per.values()), per


# ---- OSPA(2): whole tracks against whole truth trajectories ---------------------------------------------------------------------------
def _run_arrays(XY, on, what):
    """([K, n, 2] float64 contiguous, [K, n] uint8 contiguous) of one side; ValueError for a bad shape, flags that are neither bool nor
    integers, or a position that is not finite at a cell whose flag is set"""
    XY = np.asarray(XY, dtype=np.float64)
    on = np.asarray(on)
    if XY.ndim != 3 or XY.shape[2] != 2:
        raise ValueError("ospa2: %sXY is not a [K, n, 2] array (shape %r)" % (what, XY.shape))
    if on.dtype != np.bool_ and not np.issubdtype(on.dtype, np.integer):
        raise ValueError("ospa2: the flags %sOn must be bool or integers (dtype %s)" % (what, on.dtype))
    if on.shape != XY.shape[:2]:
        raise ValueError("ospa2: %sOn has shape %r, %sXY has %r" % (what, on.shape, what, XY.shape))
    on = np.ascontiguousarray(on != 0)
    if XY.shape[1] > GOSPA_MAX_SET:
        raise ValueError("ospa2: %d %ss, at most %d fit" % (XY.shape[1], what, GOSPA_MAX_SET))
    if not np.isfinite(XY[on]).all():
        raise ValueError("ospa2: %sXY holds a value that is not finite at a cell whose flag is set" % what)
    return np.ascontiguousarray(XY), on.astype(np.uint8)


def _windows(K, window, windows, every):
    """[n_win, 2] int32 (lo, hi) from the three forms ospa2_windows takes"""
    if window is not None and windows is not None:
        raise ValueError("ospa2: window and windows are mutually exclusive")
    if windows is not None:
        try:
            w = np.asarray(windows)
            ok = w.size == 0 or (w.ndim == 2 and w.shape[1] == 2 and np.issubdtype(w.dtype, np.integer))
        except (ValueError, TypeError):
            ok = False
        if not ok:
            raise ValueError("ospa2: windows must be a list of (lo, hi) pairs of integers, one per window")
        w = w.reshape(-1, 2).astype(np.int64)
        bad = np.flatnonzero((w[:, 0] < 0) | (w[:, 1] >= K) | (w[:, 0] > w[:, 1]))
        if len(bad):
            raise ValueError("ospa2: window %d is [%d, %d], the run has steps 0 .. %d" % (bad[0], w[bad[0], 0], w[bad[0], 1], K - 1))
        return w.astype(np.int32)
    if window is None:
        return np.array([[0, K - 1]] if K > 0 else [], dtype=np.int32).reshape(-1, 2)
    for name, v in (("window", window), ("every", every)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("ospa2: %s must be a positive integer (got %r); a sliding window needs window and every" % (name, v))
    hi = np.arange(0, K, int(every), dtype=np.int64)
    return np.stack([np.maximum(0, hi - int(window) + 1), hi], axis=1).astype(np.int32)


def ospa2_windows(trackXY, trackOn, truthXY, truthOn, c, p=2, window=None, windows=None, every=1, maxWorkBytes=1 << 30, device=0, ctx=None):
    """OSPA(2) between the tracks and the truth trajectories of a run, over windows of its steps.

    trackXY, trackOn   [K, n, 2] positions and [K, n] presence flags (bool or integers) of n tracks over K steps; gaps are allowed, and a
                       position whose flag is 0 is never read (it may be NaN)
    truthXY, truthOn   [K, m, 2] and [K, m]: the same for m truth trajectories            (at most 2048 a side)
    c, p               the cut-off (finite, positive) and the exponent (1 or 2)
    window, windows, every     window=None: ONE window, the whole run.  window=W: sliding windows that end at steps 0, every, 2 every, ..,
                       a window near the start being shorter (lo = max(0, hi - W + 1)).  windows=[(lo, hi), ..]: explicit, inclusive.
    maxWorkBytes       the windows go to the device in chunks whose workspace (one n x m float64 matrix per window) stays within this
    device, ctx        the GPU ordinal, or an existing pymht_amd.device.Context (a Tracker's) to run on
    For one window: a track or truth is a MEMBER if it is present at one or more of its steps (n_w, m_w of them, N = max(n_w, m_w)).
    The base distance D_ij of two members: over the U steps at which at least one of them is present, a step is near if both are present
    and |x_i - y_j| < c, else far; no near step: D = c and the pair cannot be assigned; else D = (c nFar + sum of the near distances) / U.
        total = min over one-to-one assignments of  sum D_ij^p + c^p (N - nAssigned),     ospa2 = (total / N)^(1/p)   (0 if N = 0)
    A track that covers half of a truth's life is assigned at D = c / 2 at best, and its other fragment pays c^p: what per-step GOSPA
    cannot see.  ValueError for shapes, flag dtypes, a value that is not finite at a cell whose flag is set, a bad c, p or window, more
    than 2048 a side, or one window whose workspace exceeds maxWorkBytes -- before any device is needed.
    Returns a dict of arrays over the windows:
        ospa2, total       as above
        localisation       sum D^p over the assigned pairs;  cardinality = c^p (N - nAssigned)        (total = localisation + cardinality)
        nAssigned, nTracks, nTruths      int32: assigned pairs, n_w, m_w
        windows            [n_win, 2] int32: lo, hi
        match              [n_win, n] int32: the truth assigned to every track, -1 for an unassigned member, -2 for a track that is no
                           member of the window
    One upload of positions and flags, three launches per chunk (`mht_ospa2_windows`), no host fallback; RuntimeError should a window's
    search run into its iteration bound."""
    c, p = _check_cutoff(c, p)
    X, onX = _run_arrays(trackXY, trackOn, "track")
    Y, onY = _run_arrays(truthXY, truthOn, "truth")
    if len(X) != len(Y):
        raise ValueError("ospa2: %d steps of tracks and %d steps of truths" % (len(X), len(Y)))
    K, n, m = len(X), X.shape[1], Y.shape[1]
    win = _windows(K, window, windows, every)
    n_win = len(win)
    if isinstance(maxWorkBytes, bool) or not isinstance(maxWorkBytes, (int, np.integer)) or maxWorkBytes < 0:
        raise ValueError("ospa2: maxWorkBytes must be a non-negative integer (got %r)" % (maxWorkBytes,))
    cp = c * c if p == 2 else c
    total, loc = np.zeros(n_win), np.zeros(n_win)
    count, match = np.zeros((n_win, 3), dtype=np.int32), np.zeros((n_win, n), dtype=np.int32)
    if n_win:
        lib = ctx.lib if ctx is not None else _lib.load()
        need = lambda k: int(lib.mht_ospa2_work_bytes(n, m, K, k))
        if need(1) > maxWorkBytes:
            raise ValueError("ospa2: one window of %d tracks x %d truths needs %d bytes of workspace, maxWorkBytes is %d" % (n, m, need(1), maxWorkBytes))
        chunk = int(min(n_win, max(1, maxWorkBytes // need(1))))
        while chunk < n_win and need(chunk + 1) <= maxWorkBytes:      # (the sizer rounds to 256 bytes per array, not per window)
            chunk += 1
        while need(chunk) > maxWorkBytes:
            chunk -= 1
        own = ctx is None
        if own:
            ctx = Context(device)
        try:
            dev, lib = ctx.device, ctx.lib
            xy = torch.from_numpy(np.concatenate([X.reshape(-1), Y.reshape(-1)])).to(dev)      # the one upload of the positions ..
            on = torch.from_numpy(np.concatenate([onX.reshape(-1), onY.reshape(-1)])).to(dev)      # .. and of the flags
            work = torch.empty(need(chunk), dtype=torch.uint8, device=dev)
            win_d = torch.empty((chunk, 2), dtype=torch.float64, device=dev)
            count_d = torch.empty((chunk, 3), dtype=torch.int32, device=dev)
            match_d = torch.empty((chunk, max(n, 1)), dtype=torch.int32, device=dev)
            torch.cuda.current_stream(dev).synchronize()      # (the upload ran on torch's stream)
            for w0 in range(0, n_win, chunk):
                k = min(chunk, n_win - w0)
                lo, hi = np.ascontiguousarray(win[w0:w0 + k, 0]), np.ascontiguousarray(win[w0:w0 + k, 1])
                _lib.check(lib.mht_ospa2_windows(ctx.handle, K, n, xy.data_ptr(), on.data_ptr(), m, xy.data_ptr() + 16 * K * n, on.data_ptr() + K * n,
                                                 k, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), c, p, win_d.data_ptr(),
                                                 count_d.data_ptr(), match_d.data_ptr(), work.data_ptr(), need(k)), lib)
                out = win_d[:k].cpu().numpy()
                total[w0:w0 + k], loc[w0:w0 + k] = out[:, 0], out[:, 1]
                count[w0:w0 + k] = count_d[:k].cpu().numpy()
                if n:
                    match[w0:w0 + k] = match_d.reshape(-1)[:k * n].reshape(k, n).cpu().numpy()
        finally:
            if own:
                ctx.close()
        bad = np.flatnonzero(~np.isfinite(total))
        if len(bad):
            raise RuntimeError("ospa2: the assignment search of window %d [%d, %d] ran into its iteration bound (%d tracks, %d truths)"
                               % (bad[0], win[bad[0], 0], win[bad[0], 1], count[bad[0], 1], count[bad[0], 2]))
    N = np.maximum(count[:, 1], count[:, 2])
    mean = np.divide(total, N, out=np.zeros(n_win), where=N > 0)
    return {"ospa2": mean if p == 1 else np.sqrt(mean), "total": total, "localisation": loc, "cardinality": cp * (N - count[:, 0]),
            "nAssigned": count[:, 0].copy(), "nTracks": count[:, 1].copy(), "nTruths": count[:, 2].copy(), "windows": win, "match": match}


def truth_trajectories(Y, truthIds=None):
    """([K, m, 2] float64, [K, m] uint8) of the truth of a run from its per-step arrays (`truth_steps`).  Without truthIds a truth's
    identity is its row index and every step needs the same number of rows; with truthIds (per step the identities of the step's rows,
    any hashable, as `id_switches` takes them) the trajectories are the identities in order of first appearance.  A row whose first two
    columns are NaN is absent at that step."""
    rows = []
    for s, y in enumerate(Y):
        y = np.asarray(y, dtype=np.float64)
        if y.size == 0:
            y = np.zeros((0, 2))
        if y.ndim != 2 or y.shape[1] < 2:
            raise ValueError("ospa2: the truths of step %d are not a [k, >= 2] array (shape %r)" % (s, y.shape))
        rows.append(y[:, 0:2])
    K = len(rows)
    if truthIds is None:
        if len({len(y) for y in rows}) > 1:
            raise ValueError("ospa2: a truth's identity is its row index, so every step needs the same number of rows (got %s); or give truthIds"
                             % sorted({len(y) for y in rows}))
        XY = np.stack(rows) if K else np.zeros((0, 0, 2))
    else:
        if len(truthIds) != K:
            raise ValueError("ospa2: truthIds must have one entry per step")
        col = {}
        for s, ids in enumerate(truthIds):
            if len(ids) != len(rows[s]):
                raise ValueError("ospa2: step %d has %d truths and %d identities" % (s, len(rows[s]), len(ids)))
            if len(set(ids)) != len(ids):
                raise ValueError("ospa2: step %d names an identity twice" % s)
            for who in ids:
                col.setdefault(who, len(col))
        XY = np.full((K, len(col), 2), np.nan)
        for s, ids in enumerate(truthIds):
            for r, who in enumerate(ids):
                XY[s, col[who]] = rows[s][r]
    on = ~(np.isnan(XY[:, :, 0]) & np.isnan(XY[:, :, 1]))
    return XY, on.astype(np.uint8)


# ---- NEES: is the reported covariance honest? ------------------------------------------------------------------------------------------
def _nees_launch(ctx, nx, n, L_max, D, x_d, P_d, truth, present):
    """One `mht_nees_nodes` call on states that lie on the device in the seams' layouts (x_d [L_max, nx, n], P_d [L_max, ns, n] packed):
    truth [L_max, nx, n] float64 and present [L_max, n] uint8 go up, out [L_max, nx + 3, n] comes down."""
    dev, lib = ctx.device, ctx.lib
    t_d = torch.from_numpy(np.ascontiguousarray(truth, dtype=np.float64)).to(dev)
    p_d = torch.from_numpy(np.ascontiguousarray(present, dtype=np.uint8)).to(dev)
    out_d = torch.empty((L_max, nx + 3, n), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()      # (the uploads ran on torch's stream)
    _lib.check(lib.mht_nees_nodes(ctx.handle, nx, n, L_max, D, x_d.data_ptr(), P_d.data_ptr(), t_d.data_ptr(), p_d.data_ptr(), out_d.data_ptr()), lib)
    return out_d.cpu().numpy()


def _nees_dict(rows, nx):
    """One track's dict from its rows [L, nx + 3] as the seam lays them out"""
    return {"error": rows[:, :nx].copy(), "nees2": rows[:, nx].copy(), "nees4": rows[:, nx + 1].copy(), "nees": rows[:, nx + 2].copy()}


def nees_nodes(x, P, truth, device=0, ctx=None):
    """The estimation error and the normalised estimation error squared (NEES) of every node of a batch of tracks against ground truth.

    x, P, truth   per track x [L, nx] (nx 4 or 6, the same for all), P [L, nx, nx] symmetric (the upper triangle is read) -- as
                  `smoothing.filter_tracks` and `smoothing.smooth_tracks` return them -- and truth [L, D] with D one of 2, 4, nx, the
                  same for all: the leading components [x, y, vx, vy, ...] of the true state at the node.  A NaN row of truth: the
                  node has no truth (not scored)
    device, ctx   the GPU ordinal, or an existing pymht_amd.device.Context (a Tracker's) to run on
    ValueError for shapes that do not fit -- before any device is needed; an empty list gives an empty list.
    Returns per track a dict of float64 arrays with a row per node:
        error [L, nx]   x - truth on the leading D components, NaN beyond
        nees2 [L]       the position error under the marginal position covariance, e' P_2^-1 e: chi-square, 2 degrees of freedom,
                        when P is honest
        nees4 [L]       position and velocity, 4 degrees of freedom (NaN if D < 4)
        nees [L]        the full state, nx degrees of freedom (NaN if D < nx; nees4's figure at nx = 4)
    From one Cholesky factorisation P = U' U per node: with U' y = e the sum of y_j^2 over j < d is the NEES of the leading d components,
    exactly.  A node without truth, or whose x or P holds a NaN, is NaN throughout; a pivot j that is not positive gives NaN in every
    figure that includes component j and leaves the figures in front of it.  One upload, one launch (`mht_nees_nodes`), no host
    fallback.  `nees_consistency` runs the tests on the result."""
    if not (len(x) == len(P) == len(truth)):
        raise ValueError("nees: %d tracks of states, %d of covariances and %d of truth" % (len(x), len(P), len(truth)))
    n = len(x)
    if n == 0:
        return []
    X = [np.asarray(a, dtype=np.float64) for a in x]
    nx = X[0].shape[1] if X[0].ndim == 2 else -1
    if nx not in (4, 6):
        raise ValueError("nees: the states are [L, 4] or [L, 6] arrays (track 0 has shape %r)" % (X[0].shape,))
    Pm = [np.asarray(a, dtype=np.float64) for a in P]
    T = [np.asarray(a, dtype=np.float64) for a in truth]
    D = T[0].shape[1] if T[0].ndim == 2 else -1
    if D not in (2, 4, nx):
        raise ValueError("nees: the truth carries 2, 4 or nx = %d leading components of the state (track 0 has shape %r)" % (nx, T[0].shape))
    for t in range(n):
        L = len(X[t])
        if X[t].shape != (L, nx) or Pm[t].shape != (L, nx, nx) or T[t].shape != (L, D) or L < 1:
            raise ValueError("nees: track %d has shapes %r, %r and %r; [L, %d], [L, %d, %d] and [L, %d] with L >= 1 are wanted"
                             % (t, X[t].shape, Pm[t].shape, T[t].shape, nx, nx, nx, D))
    lens = np.array([len(a) for a in X])
    L_max, ns = int(lens.max()), nx * (nx + 1) // 2
    iu = np.triu_indices(nx)
    xp, Pp = np.full((L_max, nx, n), np.nan), np.full((L_max, ns, n), np.nan)      # (rows behind a track's end: NaN, as the seams write them)
    tp, pp = np.zeros((L_max, nx, n)), np.zeros((L_max, n), dtype=np.uint8)
    for t in range(n):
        L = lens[t]
        there = ~np.isnan(T[t]).any(axis=1)
        xp[:L, :, t], Pp[:L, :, t] = X[t], Pm[t][:, iu[0], iu[1]]
        tp[:L, :D, t], pp[:L, t] = np.where(there[:, None], T[t], 0.0), there
    own = ctx is None
    if own:
        ctx = Context(device, nx=nx)
    try:
        up = lambda a: torch.from_numpy(a).to(ctx.device)
        out = _nees_launch(ctx, nx, n, L_max, D, up(xp), up(Pp), tp, pp)
    finally:
        if own:
            ctx.close()
    return [_nees_dict(np.ascontiguousarray(out[:lens[t], :, t]), nx) for t in range(n)]


def nees_consistency(results, alpha=0.05):
    """The NEES tests of the tracking literature (Bar-Shalom, Li, Kirubarajan: Estimation with Applications to Tracking and Navigation,
    ch. 5.4) on the dicts of `nees_nodes`, host only, float64.  A cell is a node with truth (a finite error[0]).  A result may carry
    `step` [L] (int; negative: no step): the step of the run each node belongs to (`Tracker.getNees` fills it in); without it a node's
    step is its row.  Returns a dict:
        alpha, nCells
        rmsPosition     sqrt of the mean of e_x^2 + e_y^2 over the cells;  rmsVelocity: of e_vx^2 + e_vy^2 over the cells that carry it
        dims            {dof: figures} for dof in 2, 4, nx where the truth carries that many components, each a dict of
          n               the cells
          mean            the NEES summed over the cells, divided by dof n: 1 when the covariance is honest
          interval        (lo, hi) = chi2.ppf([alpha/2, 1 - alpha/2], dof n) / (dof n)
          inside          lo <= mean <= hi.  Above: the covariance is too small (optimistic), or the estimate is biased; below: too
                          large (pessimistic)
          outlierFraction the share of cells above chi2.ppf(1 - alpha, dof): alpha when the covariance is honest
          perStep         {"step", "n", "mean", "lo", "hi", "inside"}: arrays over the steps that have a cell -- the same test per
                          step, pooled over the step's tracks
    The PER-STEP test is Bar-Shalom's test proper: the tracks of a step are independent, so the sum of their NEES is chi-square with
    dof n degrees of freedom.  The POOLED figures add up all cells, and consecutive errors of one track are correlated (the filter's
    error is a first-order process): the sum over a track is NOT chi-square with dof L degrees of freedom, its spread is wider, so the
    pooled interval is approximate -- too narrow -- and is a summary, not a test of exact size.  A cell whose figure is NaN (a P that is
    not positive definite) makes the means that include it NaN and their verdicts None, as a NaN nis does in smoothing.consistency;
    without cells the figures are NaN and the verdicts None.  alpha outside (0, 1) raises ValueError."""
    from scipy.stats import chi2
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not 0.0 < float(alpha) < 1.0:
        raise ValueError("nees: alpha is a probability strictly between 0 and 1 (got %r)" % (alpha,))
    alpha = float(alpha)
    nan = float("nan")
    err, figs, steps = [], {"nees2": [], "nees4": [], "nees": []}, []
    nx = None
    for r in results:
        e = np.asarray(r["error"], dtype=np.float64)
        if e.ndim != 2 or (nx is not None and e.shape[1] != nx):
            raise ValueError("nees: the results do not have one state dimension")
        nx = e.shape[1]
        cell = np.isfinite(e[:, 0])
        step = np.asarray(r["step"], dtype=np.int64) if "step" in r else np.arange(len(e), dtype=np.int64)
        cell &= step >= 0
        err.append(e[cell])
        steps.append(step[cell])
        for k in figs:
            figs[k].append(np.asarray(r[k], dtype=np.float64)[cell])
    out = {"alpha": alpha, "nCells": 0, "rmsPosition": nan, "rmsVelocity": nan, "dims": {}}
    if nx is None:
        return out
    err, steps = np.concatenate(err), np.concatenate(steps)
    out["nCells"] = int(len(err))
    if len(err) == 0:
        return out
    out["rmsPosition"] = float(np.sqrt(np.mean(np.sum(err[:, 0:2] ** 2, axis=1))))
    vel = np.isfinite(err[:, 3])
    if vel.any():
        out["rmsVelocity"] = float(np.sqrt(np.mean(np.sum(err[vel, 2:4] ** 2, axis=1))))
    for dof, key in ((2, "nees2"), (4, "nees4"), (nx, "nees")):
        carried = np.isfinite(err[:, dof - 1])      # (the truth of the cell carries dof components)
        if dof in out["dims"] or not carried.any():
            continue
        q, st = np.concatenate(figs[key])[carried], steps[carried]
        n = int(len(q))
        lo, hi = (float(v) / (dof * n) for v in chi2.ppf([alpha / 2.0, 1.0 - alpha / 2.0], dof * n))
        mean = float(np.sum(q)) / (dof * n)
        fig = {"n": n, "mean": mean, "interval": (lo, hi), "inside": None, "outlierFraction": nan}
        if np.isfinite(mean):
            fig["inside"] = bool(lo <= mean <= hi)
            fig["outlierFraction"] = float(np.sum(q > float(chi2.ppf(1.0 - alpha, dof)))) / n
        which = np.unique(st)
        cnt = np.array([int(np.sum(st == s)) for s in which], dtype=np.int64)
        with np.errstate(invalid="ignore"):
            m = np.array([np.sum(q[st == s]) for s in which], dtype=np.float64) / (dof * cnt)
        slo, shi = chi2.ppf(alpha / 2.0, dof * cnt) / (dof * cnt), chi2.ppf(1.0 - alpha / 2.0, dof * cnt) / (dof * cnt)
        fig["perStep"] = {"step": which, "n": cnt, "mean": m, "lo": slo, "hi": shi,
                          "inside": np.array([None if not np.isfinite(v) else bool(a <= v <= b) for v, a, b in zip(m, slo, shi)], dtype=object)}
        out["dims"][dof] = fig
    return out


# ---- encounters: who comes close to whom within the next minutes? ------------------------------------------------------------------
ENCOUNTER_NAMES = ("tcpa", "dcpa", "md2", "pc", "tpc")      # the order of the seam's out [5][first][n]
ENCOUNTER_MAX_STEPS = 64                                    # csrc/mht_encounter.h


def encounter_model(model, dt):
    """(nx, Phi(dt), Q(dt)) of a tracker's model module for `encounters`, in float64 -- the float32 matrices the model returns, widened.
    A constant-turn model raises NotImplementedError: its transition depends on the state (models/ct.py), and it is not propagated
    with Phi(T, 0) in its place."""
    if getattr(model, "transition", None) == "ct":
        raise NotImplementedError("encounters: the transition of model %r depends on the state (Phi(T, w) per hypothesis, models/ct.py); "
                                  "the linear propagation does not apply" % getattr(model, "__name__", model))
    nx = int(np.asarray(model.C_RADAR).shape[1])
    if nx not in (4, 6):
        raise ValueError("encounters: 4- or 6-state models (got %d states)" % nx)
    widen = lambda m: np.ascontiguousarray(np.asarray(m, dtype=np.float32).astype(np.float64).reshape(nx, nx))
    return nx, widen(model.Phi(float(dt))), widen(model.Q(float(dt)))


def _encounter_empty(first, n):
    return {k: np.full((first, n), np.nan) for k in ENCOUNTER_NAMES}


def encounters(x, P, Phi, Q, steps, dt, radius, first=None, device=0, ctx=None):
    """Which of n tracks come close to each other within the next steps * dt seconds, and how sure is that?

    x, P       the entries at one common time: x [n, nx] (nx 4 or 6, the state [x, y, vx, vy, ...]) and P [n, nx, nx] symmetric (the
               upper triangle is read) -- e.g. the last rows of `smoothing.filter_tracks`
    Phi, Q     [nx, nx]: the linear model of ONE step of dt seconds (of Q the upper triangle is read)
    steps, dt  1 .. 64 steps of dt > 0 seconds: the horizon is steps * dt
    radius     the safety radius R > 0, in the units of the positions
    first      None: all pairs.  Else 0 .. n: only the pairs (i, j) with i < first -- first=1 with the own ship as entry 0 gives the own
               ship against everyone
    device, ctx   the GPU ordinal, or an existing pymht_amd.device.Context (a Tracker's) to run on
    ValueError for arguments that do not fit -- before any device is needed.  Fewer than two entries, or first=0, give empty
    ([first, n], all NaN) arrays and no device call.
    Returns a dict of float64 [first, n] arrays, NaN where j <= i; with d_k the difference of the two propagated positions
    (x_k = Phi x_{k-1}, P_k = Phi P_{k-1} Phi' + Q) and Sigma_k the SUM of their position covariances -- the tracks are taken as
    independent, cross-correlation between them is not modelled:
        tcpa, dcpa   the closest point of approach of the piecewise-linear path through d_0 .. d_steps: its (earliest) time and its
                     distance.  The exact CPA within the horizon for a constant-velocity model; for a constant-acceleration model the
                     piecewise-linear figure
        md2          the smallest d_k' Sigma_k^-1 d_k over the steps
        pc, tpc      the largest probability over the steps that the two are within `radius` of each other, and the time k dt of the
                     (earliest) largest.  pc_k is the mass of N(d_k, Sigma_k) inside the disc, BY A RULE (csrc/mht_encounter.h: closed-form
                     eigen-decomposition, a clip at 8 sigma along the narrow axis beyond which pc_k is 0 exactly, a 64-node
                     Gauss-Legendre rule): good to about 1e-6 absolute against the exact mass, not exact
    A NaN in an entry makes the figures of its pairs NaN; a Sigma_k that is not positive definite makes pc, tpc and md2 of the pair NaN
    and leaves tcpa and dcpa.  One upload, one call of `mht_encounters` (two launches), no host fallback."""
    X, Pm = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    Phi, Q = np.asarray(Phi, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    nx = X.shape[1] if X.ndim == 2 else -1
    if nx not in (4, 6):
        raise ValueError("encounters: the states are an [n, 4] or [n, 6] array (got shape %r)" % (X.shape,))
    n = len(X)
    if Pm.shape != (n, nx, nx) or Phi.shape != (nx, nx) or Q.shape != (nx, nx):
        raise ValueError("encounters: P, Phi and Q have shapes %r, %r and %r; [%d, %d, %d] and twice [%d, %d] are wanted"
                         % (Pm.shape, Phi.shape, Q.shape, n, nx, nx, nx, nx))
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= ENCOUNTER_MAX_STEPS:
        raise ValueError("encounters: steps is an integer in 1 .. %d (got %r)" % (ENCOUNTER_MAX_STEPS, steps))
    for name, v in (("dt", dt), ("radius", radius)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not v > 0:
            raise ValueError("encounters: %s must be a finite positive number (got %r)" % (name, v))
    if first is None:
        first = n
    if isinstance(first, bool) or not isinstance(first, (int, np.integer)) or not 0 <= first <= n:
        raise ValueError("encounters: first is an integer in 0 .. n = %d (got %r)" % (n, first))
    if not (np.isfinite(Phi).all() and np.isfinite(Q).all()):
        raise ValueError("encounters: Phi and Q must be finite")
    first, steps = int(first), int(steps)
    if n < 2 or first == 0:
        return _encounter_empty(first, n)
    iu = np.triu_indices(nx)
    xp, Pp = np.ascontiguousarray(X.T), np.ascontiguousarray(Pm[:, iu[0], iu[1]].T)
    Phi, Q = np.ascontiguousarray(Phi), np.ascontiguousarray(Q)
    own = ctx is None
    if own:
        ctx = Context(device, nx=nx)
    try:
        dev, lib = ctx.device, ctx.lib
        x_d, P_d = torch.from_numpy(xp).to(dev), torch.from_numpy(Pp).to(dev)
        need = int(lib.mht_encounter_work_bytes(n, steps))
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        out_d = torch.empty((len(ENCOUNTER_NAMES), first, n), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()      # (the uploads ran on torch's stream)
        _lib.check(lib.mht_encounters(ctx.handle, nx, n, first, steps, float(dt), float(radius), Phi.ctypes.data, Q.ctypes.data,
                                      x_d.data_ptr(), P_d.data_ptr(), out_d.data_ptr(), work.data_ptr(), need), lib)
        out = out_d.cpu().numpy()
    finally:
        if own:
            ctx.close()
    return {k: np.ascontiguousarray(out[f]) for f, k in enumerate(ENCOUNTER_NAMES)}


# ---- trial manoeuvres: and if the own ship alters course or speed? ------------------------------------------------------------------
TRIAL_MAX_CANDIDATES = 4096                                    # MHT_TRIAL_MAX_CANDIDATES, include/mht_amd.h
TRIAL_SUMMARY_NAMES = ("pcMax", "pcArg", "dcpaMin", "dcpaArg")      # the order of the seam's summary [4][G]


def _trial_number(name, v, positive=True):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or (positive and not v > 0):
        raise ValueError("trial_manoeuvres: %s must be a finite%s number (got %r)" % (name, " positive" if positive else "", v))
    return float(v)


def trial_candidates(candidates):
    """The candidates as a contiguous float64 [G, 3] array of (dpsi, f, t0), checked: 1 .. TRIAL_MAX_CANDIDATES rows, every figure finite
    or NaN, |dpsi| <= pi, f >= 0, t0 >= 0.  ValueError otherwise."""
    try:
        cand = np.ascontiguousarray(candidates, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("trial_manoeuvres: the candidates are a [G, 3] array of (dpsi, f, t0) (got %r)" % (candidates,))
    if cand.ndim != 2 or cand.shape[1] != 3 or not 1 <= len(cand) <= TRIAL_MAX_CANDIDATES:
        raise ValueError("trial_manoeuvres: the candidates are a [G, 3] array of (dpsi, f, t0), G in 1 .. %d (got shape %r)" % (TRIAL_MAX_CANDIDATES, cand.shape))
    with np.errstate(invalid="ignore"):
        if np.isinf(cand).any() or (np.abs(cand[:, 0]) > np.pi).any() or (cand[:, 1] < 0).any() or (cand[:, 2] < 0).any():
            raise ValueError("trial_manoeuvres: a candidate is (dpsi, f, t0) with |dpsi| <= pi, f >= 0 and t0 >= 0, each finite or NaN")
    return cand


def _trial_empty(G, n):
    out = {k: np.full((G, n), np.nan) for k in ENCOUNTER_NAMES}
    out.update(pcMax=np.full(G, np.nan), pcArg=np.full(G, -1, dtype=np.int64), dcpaMin=np.full(G, np.nan), dcpaArg=np.full(G, -1, dtype=np.int64))
    return out


def trial_manoeuvres(x, P, Phi, Q, steps, dt, radius, own, candidates, turnRate, ownCovariance=None, device=0, ctx=None):
    """And if the own ship alters course or speed?  G candidate manoeuvres, each held against every one of n tracks over the next
    steps * dt seconds, in one device call: the tracks are propagated once, the table of candidates x tracks is filled in one launch
    and folded to the worst track per candidate.

    x, P, Phi, Q, steps, dt, radius   the tracks, the model of one step and the safety radius, as for `encounters`; the own ship is NOT
               one of the entries
    own        [x, y, vx, vy]: the own ship's position p0 and velocity v0 at the current scan
    candidates [G, 3] rows (dpsi, f, t0), G in 1 .. 4096: the course change in radians, positive counter-clockwise in the tracker's axes,
               |dpsi| <= pi; the speed factor f >= 0; the delay t0 >= 0 in seconds
    turnRate   w > 0 in rad/s, for all candidates
    ownCovariance   None (zeros: a known own position) or the own ship's 2 x 2 position covariance, constant over the horizon
    device, ctx   the GPU ordinal, or an existing pymht_amd.device.Context (a Tracker's) to run on
    The manoeuvre (csrc/mht_trial.h): the own ship stands on until t0, p(t) = p0 + t v0; then turns at rate sign(dpsi) w and speed
    f |v0| -- the speed changes at t0 at once, ARPA's convention -- until te = t0 + |dpsi| / w,
    p(t) = p(t0) + f [sw, -sg cw; sg cw, sw] v0 with sw = sin(w (t - t0)) / w and cw = (1 - cos(w (t - t0))) / w; then runs straight,
    p(t) = p(te) + (t - te) f Rot(dpsi) v0.  dpsi = 0 skips the arc, a t0 beyond the horizon is "stand on", a turn may end beyond
    the horizon.  Positions are closed forms at t = k dt.  A NaN in a candidate, in `own` or in the covariance makes that candidate's
    row NaN.
    ValueError for arguments that do not fit -- before any device is needed.  No track: empty [G, 0] arrays and no device call.
    Returns a dict: `encounters`' five figures as float64 [G, n] arrays (cell (g, j): candidate g against track j, d_k = own - track,
    pc by the same rule, good to about 1e-6, not exact; the two are taken as independent), and per candidate `pcMax` with `pcArg` -- the
    largest pc of the row and its track -- and `dcpaMin` with `dcpaArg`, [G], the indices int64: NaN cells do not take part, equal
    figures go to the lowest track, a row without a figure gives NaN and -1; and `candidates`, the [G, 3] array as it was used.  One
    upload, one call of `mht_trial_manoeuvres` (four launches), no host fallback."""
    X, Pm = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    Phi, Q = np.asarray(Phi, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    nx = X.shape[1] if X.ndim == 2 else -1
    if nx not in (4, 6):
        raise ValueError("trial_manoeuvres: the states are an [n, 4] or [n, 6] array (got shape %r)" % (X.shape,))
    n = len(X)
    if Pm.shape != (n, nx, nx) or Phi.shape != (nx, nx) or Q.shape != (nx, nx):
        raise ValueError("trial_manoeuvres: P, Phi and Q have shapes %r, %r and %r; [%d, %d, %d] and twice [%d, %d] are wanted"
                         % (Pm.shape, Phi.shape, Q.shape, n, nx, nx, nx, nx))
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= ENCOUNTER_MAX_STEPS:
        raise ValueError("trial_manoeuvres: steps is an integer in 1 .. %d (got %r)" % (ENCOUNTER_MAX_STEPS, steps))
    dt, radius, w = _trial_number("dt", dt), _trial_number("radius", radius), _trial_number("turnRate", turnRate)
    if not (np.isfinite(Phi).all() and np.isfinite(Q).all()):
        raise ValueError("trial_manoeuvres: Phi and Q must be finite")
    try:
        o = np.ascontiguousarray(own, dtype=np.float64)
    except (TypeError, ValueError):
        o = np.zeros(0)
    if o.shape != (4,) or np.isinf(o).any():
        raise ValueError("trial_manoeuvres: own is [x, y, vx, vy], finite or NaN (got %r)" % (own,))
    cov = np.zeros((2, 2)) if ownCovariance is None else np.asarray(ownCovariance, dtype=np.float64)
    if cov.shape != (2, 2) or np.isinf(cov).any() or not (cov[0, 1] == cov[1, 0] or np.isnan(cov).any()):
        raise ValueError("trial_manoeuvres: ownCovariance is a symmetric 2 x 2 matrix, finite or NaN (got %r)" % (ownCovariance,))
    so = np.array([cov[0, 0], cov[0, 1] if cov[1, 0] == cov[1, 0] else np.nan, cov[1, 1]])      # (a NaN below the diagonal counts as well)
    cand = trial_candidates(candidates)
    G, steps = len(cand), int(steps)
    if n == 0:
        out = _trial_empty(G, 0)
        out["candidates"] = cand
        return out
    iu = np.triu_indices(nx)
    xp, Pp = np.ascontiguousarray(X.T), np.ascontiguousarray(Pm[:, iu[0], iu[1]].T)
    Phi, Q = np.ascontiguousarray(Phi), np.ascontiguousarray(Q)
    mine = ctx is None
    if mine:
        ctx = Context(device, nx=nx)
    try:
        dev, lib = ctx.device, ctx.lib
        x_d, P_d = torch.from_numpy(xp).to(dev), torch.from_numpy(Pp).to(dev)
        need = int(lib.mht_trial_work_bytes(n, G, steps))
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        out_d = torch.empty((len(ENCOUNTER_NAMES), G, n), dtype=torch.float64, device=dev)
        sum_d = torch.empty((len(TRIAL_SUMMARY_NAMES), G), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()      # (the uploads ran on torch's stream)
        _lib.check(lib.mht_trial_manoeuvres(ctx.handle, nx, n, G, steps, dt, radius, Phi.ctypes.data, Q.ctypes.data, x_d.data_ptr(), P_d.data_ptr(),
                                            o.ctypes.data, so.ctypes.data, w, cand.ctypes.data, out_d.data_ptr(), sum_d.data_ptr(), work.data_ptr(), need), lib)
        out, summary = out_d.cpu().numpy(), sum_d.cpu().numpy()
    finally:
        if mine:
            ctx.close()
    res = {k: np.ascontiguousarray(out[f]) for f, k in enumerate(ENCOUNTER_NAMES)}
    res.update(pcMax=summary[0].copy(), pcArg=summary[1].astype(np.int64), dcpaMin=summary[2].copy(), dcpaArg=summary[3].astype(np.int64), candidates=cand)
    return res


# ---- trial manoeuvres against every live hypothesis: the best hypothesis is not the only one -----------------------------------------
TRIAL_HYP_NAMES = ("pcWorst", "pcWorstLeaf", "dcpaMin", "dcpaMinLeaf", "pcMean", "pcSel", "dcpaSel", "tcpaSel")      # the seam's fig [8][G][T]


def _trial_hyp_empty(G, T, L, cand, leafTable):
    out = {k: np.full((G, T), np.nan) for k in TRIAL_HYP_NAMES}
    out["pcWorstLeaf"], out["dcpaMinLeaf"] = np.full((G, T), -1, dtype=np.int64), np.full((G, T), -1, dtype=np.int64)
    out.update(weight=np.full(L, np.nan), nLeaves=np.zeros(T, dtype=np.int64), candidates=cand)
    if leafTable:
        out.update({k: np.full((G, L), np.nan) for k in ENCOUNTER_NAMES})
    return out


def trial_hypotheses(x, P, cnllr, target, Phi, Q, steps, dt, radius, own, candidates, turnRate, selected=None, ownCovariance=None, leafTable=False,
                     device=0, ctx=None):
    """`trial_manoeuvres` held against EVERY LIVE HYPOTHESIS of every target instead of one state per track: the entries are the L leaves
    of the forest, and the candidates' rows are folded per target.  A multi-hypothesis tracker keeps, per target, the alternatives "that
    plot was clutter" and "it took the other plot"; the best of them is not the only one, and a second leaf nearly as likely may give a
    very different pc.

    x, P, cnllr, target   the leaves in `Tracker.leafBatch()`'s layout: x [L, nx], P [L, nx, nx], the cumulative NLLR [L] (a LOWER one is
               the better hypothesis; NaN: the leaf has no weight; +inf: weight 0; -inf is refused) and the NON-DECREASING target index
               [L] of every leaf.  A target index that no leaf carries is an empty target
    selected   None, or [T]: per target the index (into the L leaves) of its selected leaf, inside the target's leaves, or -1.  Given, it
               also sets the number of targets T (otherwise T = target[-1] + 1)
    leafTable  True: the five [G, L] tables of `trial_manoeuvres` are returned as well (5 G L doubles on the device and on the host);
               the per-target figures do not need them to exist
    Phi, Q, steps, dt, radius, own, candidates, turnRate, ownCovariance, device, ctx   as for `trial_manoeuvres`
    ValueError for arguments that do not fit -- before any device is needed.  No leaf: empty arrays and no device call.
    Returns a dict of [G, T] arrays (csrc/mht_trial_hyp.h states the operations), a cell (g, l) being `trial_manoeuvres`' cell of
    candidate g against leaf l, bit for bit:
        pcWorst, pcWorstLeaf   the largest pc over the target's leaves and its leaf (int64, an index into the L leaves)
        dcpaMin, dcpaMinLeaf   the smallest dcpa and its leaf.  NaN cells take no part, equal figures go to the lowest leaf, no figure
                               gives NaN and -1
        pcMean                 sum(w_l pc_l) / sum(w_l) over the leaves with a pc and a cnllr, w_l = exp(-(cnllr_l - cmin_t)) with cmin_t
                               the target's smallest cnllr; NaN where there is no such leaf.  A target of one leaf has pcMean = pc
        pcSel, dcpaSel, tcpaSel   the cell of the selected leaf: what the best-hypothesis view reports, next to what it hides.  NaN
                               where the target has none
    and `weight` [L], w_l / sum(w) within the leaf's target (NaN without a cnllr), `nLeaves` [T] (int64) and `candidates` [G, 3].
    THE WEIGHTS NORMALISE INSIDE ONE TARGET.  The exclusion constraints between targets, which the ILP enforces, are ignored: this is
    the usual track-oriented approximation of the hypothesis probabilities, not the probability of a global hypothesis.  pc is by
    `encounters`' rule, good to about 1e-6, not exact; the own ship and the leaves are taken as independent.
    One upload, one call of `mht_trial_hypotheses` (five launches), no host fallback."""
    X, Pm = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    Phi, Q = np.asarray(Phi, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    nx = X.shape[1] if X.ndim == 2 else -1
    if nx not in (4, 6):
        raise ValueError("trial_hypotheses: the states are an [L, 4] or [L, 6] array (got shape %r)" % (X.shape,))
    L = len(X)
    if Pm.shape != (L, nx, nx) or Phi.shape != (nx, nx) or Q.shape != (nx, nx):
        raise ValueError("trial_hypotheses: P, Phi and Q have shapes %r, %r and %r; [%d, %d, %d] and twice [%d, %d] are wanted"
                         % (Pm.shape, Phi.shape, Q.shape, L, nx, nx, nx, nx))
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= ENCOUNTER_MAX_STEPS:
        raise ValueError("trial_hypotheses: steps is an integer in 1 .. %d (got %r)" % (ENCOUNTER_MAX_STEPS, steps))
    try:
        dt, radius, w = _trial_number("dt", dt), _trial_number("radius", radius), _trial_number("turnRate", turnRate)
        cand = trial_candidates(candidates)
    except ValueError as exc:
        raise ValueError(str(exc).replace("trial_manoeuvres", "trial_hypotheses", 1))
    if not (np.isfinite(Phi).all() and np.isfinite(Q).all()):
        raise ValueError("trial_hypotheses: Phi and Q must be finite")
    try:
        o = np.ascontiguousarray(own, dtype=np.float64)
    except (TypeError, ValueError):
        o = np.zeros(0)
    if o.shape != (4,) or np.isinf(o).any():
        raise ValueError("trial_hypotheses: own is [x, y, vx, vy], finite or NaN (got %r)" % (own,))
    cov = np.zeros((2, 2)) if ownCovariance is None else np.asarray(ownCovariance, dtype=np.float64)
    if cov.shape != (2, 2) or np.isinf(cov).any() or not (cov[0, 1] == cov[1, 0] or np.isnan(cov).any()):
        raise ValueError("trial_hypotheses: ownCovariance is a symmetric 2 x 2 matrix, finite or NaN (got %r)" % (ownCovariance,))
    so = np.array([cov[0, 0], cov[0, 1] if cov[1, 0] == cov[1, 0] else np.nan, cov[1, 1]])      # (a NaN below the diagonal counts as well)
    cn = np.ascontiguousarray(cnllr, dtype=np.float64)
    if cn.shape != (L,) or (cn == -np.inf).any():
        raise ValueError("trial_hypotheses: cnllr is an [L] = [%d] array without -inf (got shape %r)" % (L, cn.shape))
    tg = np.asarray(target)
    if tg.shape != (L,) or not np.issubdtype(tg.dtype, np.integer) or (L and (tg[0] < 0 or (np.diff(tg) < 0).any())):
        raise ValueError("trial_hypotheses: target is a non-decreasing [L] = [%d] array of target indices >= 0 (got %r)" % (L, target))
    T = int(tg[-1]) + 1 if L else 0
    if selected is not None:
        sl = np.asarray(selected)
        if sl.ndim != 1 or not np.issubdtype(sl.dtype, np.integer) or len(sl) < T:
            raise ValueError("trial_hypotheses: selected is an integer array with one entry per target, %d at least (got %r)" % (T, selected))
        T = len(sl)
    else:
        sl = np.full(T, -1)
    seg = np.searchsorted(tg, np.arange(T + 1)).astype(np.int32)      # the leaves of target t: seg[t] .. seg[t + 1] - 1
    sl = np.ascontiguousarray(sl, dtype=np.int32)
    if ((sl != -1) & ((sl < seg[:-1]) | (sl >= seg[1:]))).any():
        raise ValueError("trial_hypotheses: selected[t] is -1 or the index of a leaf of target t (got %r)" % (selected,))
    G, steps = len(cand), int(steps)
    if L == 0:
        return _trial_hyp_empty(G, T, 0, cand, leafTable)
    iu = np.triu_indices(nx)
    xp, Pp = np.ascontiguousarray(X.T), np.ascontiguousarray(Pm[:, iu[0], iu[1]].T)
    Phi, Q = np.ascontiguousarray(Phi), np.ascontiguousarray(Q)
    mine = ctx is None
    if mine:
        ctx = Context(device, nx=nx)
    try:
        dev, lib = ctx.device, ctx.lib
        x_d, P_d, c_d = torch.from_numpy(xp).to(dev), torch.from_numpy(Pp).to(dev), torch.from_numpy(cn).to(dev)
        need = int(lib.mht_trial_hyp_work_bytes(L, T, G, steps))
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        tab_d = torch.empty((len(ENCOUNTER_NAMES), G, L), dtype=torch.float64, device=dev) if leafTable else None
        fig_d = torch.empty((len(TRIAL_HYP_NAMES), G, T), dtype=torch.float64, device=dev)
        wgt_d = torch.empty(L, dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()      # (the uploads ran on torch's stream)
        _lib.check(lib.mht_trial_hypotheses(ctx.handle, nx, L, T, G, steps, dt, radius, Phi.ctypes.data, Q.ctypes.data, x_d.data_ptr(), P_d.data_ptr(),
                                            c_d.data_ptr(), seg.ctypes.data, sl.ctypes.data, o.ctypes.data, so.ctypes.data, w, cand.ctypes.data,
                                            tab_d.data_ptr() if leafTable else None, fig_d.data_ptr(), wgt_d.data_ptr(), work.data_ptr(), need), lib)
        fig, weight = fig_d.cpu().numpy(), wgt_d.cpu().numpy()
        table = tab_d.cpu().numpy() if leafTable else None
    finally:
        if mine:
            ctx.close()
    res = {k: np.ascontiguousarray(fig[f]) for f, k in enumerate(TRIAL_HYP_NAMES)}
    res["pcWorstLeaf"], res["dcpaMinLeaf"] = res["pcWorstLeaf"].astype(np.int64), res["dcpaMinLeaf"].astype(np.int64)
    res.update(weight=weight, nLeaves=np.diff(seg).astype(np.int64), candidates=cand)
    if leafTable:
        res.update({k: np.ascontiguousarray(table[f]) for f, k in enumerate(ENCOUNTER_NAMES)})
    return res


def trial_best(pcMax, dcpaMin):
    """The safest candidate of a summary: the smallest pcMax, then the largest dcpaMin, then the lowest index.  A candidate whose pcMax is
    NaN -- no cell of its row has a pc -- is not eligible (nothing is known about it); among equal pcMax a NaN dcpaMin ranks last.
    None if no candidate is eligible."""
    pc, d = np.asarray(pcMax, dtype=np.float64), np.asarray(dcpaMin, dtype=np.float64)
    best = None
    for g in range(len(pc)):
        if np.isnan(pc[g]):
            continue
        dg = -np.inf if np.isnan(d[g]) else d[g]
        if best is None or pc[g] < best[0] or (pc[g] == best[0] and dg > best[1]):
            best = (pc[g], dg, g)
    return None if best is None else best[2]


# ---- encounters by Monte Carlo: at any time of the horizon, for a mixture, and for the constant-turn model ------------------------------
MC_MAX_PATHS, MC_MAX_STEPS, MC_MAX_PARTICLES, MC_WARP = 64, 64, 1 << 20, 64      # MHT_MC_*, include/mht_amd.h
MC_OK, MC_NAN, MC_NOT_PSD = 0, 1, 2
MC_COUNT_NAMES = ("within", "ever", "valid", "status")


def mc_own_paths(own, candidates, turnRate, steps, dt):
    """The own ship's positions at t = k dt, k = 0 .. steps, for every candidate manoeuvre (dpsi, f, t0): float64 [G, steps + 1, 2].  The
    manoeuvre of `trial_manoeuvres` (csrc/mht_trial.h: stand on until t0, an arc at rate sign(dpsi) turnRate and speed f |v0| until
    te = t0 + |dpsi| / turnRate, then straight), in NumPy, every operation in the header's order.  A NaN in a candidate or in `own`
    makes that candidate's path NaN.  ValueError as `trial_manoeuvres` raises them."""
    try:
        w, dt = _trial_number("turnRate", turnRate), _trial_number("dt", dt)
        cand = trial_candidates(candidates)
    except ValueError as exc:
        raise ValueError(str(exc).replace("trial_manoeuvres", "mc_own_paths", 1))
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= MC_MAX_STEPS:
        raise ValueError("mc_own_paths: steps is an integer in 1 .. %d (got %r)" % (MC_MAX_STEPS, steps))
    try:
        o = np.ascontiguousarray(own, dtype=np.float64)
    except (TypeError, ValueError):
        o = np.zeros(0)
    if o.shape != (4,) or np.isinf(o).any():
        raise ValueError("mc_own_paths: own is [x, y, vx, vy], finite or NaN (got %r)" % (own,))
    p0x, p0y, v0x, v0y = o
    dpsi, f, t0 = cand[:, 0], cand[:, 1], cand[:, 2]
    bad = np.isnan(cand).any(axis=1) | np.isnan(o).any()
    out = np.zeros((len(cand), int(steps) + 1, 2))
    with np.errstate(all="ignore"):
        ad = np.abs(dpsi)
        sg = np.where(dpsi > 0, 1.0, np.where(dpsi < 0, -1.0, 0.0))
        te = t0 + ad / w
        ax, ay = p0x + t0 * v0x, p0y + t0 * v0y
        se, ce = np.sin(ad), np.cos(ad)
        swe, cwe = se / w, (1.0 - ce) / w
        bx, by = ax + f * (swe * v0x - (sg * cwe) * v0y), ay + f * ((sg * cwe) * v0x + swe * v0y)
        ux, uy = f * (ce * v0x - (sg * se) * v0y), f * ((sg * se) * v0x + ce * v0y)
        for k in range(int(steps) + 1):
            t = float(k) * dt
            tau = t - t0
            sn, cs = np.sin(w * tau), np.cos(w * tau)
            sw, cw = sn / w, (1.0 - cs) / w
            arc_x, arc_y = ax + f * (sw * v0x - (sg * cw) * v0y), ay + f * ((sg * cw) * v0x + sw * v0y)
            r = t - te
            out[:, k, 0] = np.where(t <= t0, p0x + t * v0x, np.where(t <= te, arc_x, bx + r * ux))
            out[:, k, 1] = np.where(t <= t0, p0y + t * v0y, np.where(t <= te, arc_y, by + r * uy))
    out[bad] = np.nan
    return out


def mc_standard_error(p, valid):
    """sqrt(max(p (1 - p), 1 / S) / S): the binomial standard error of a share p of S particles, floored at one particle so that a
    count of 0 or S does not claim certainty.  NaN where valid is 0."""
    S = np.asarray(valid, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(S > 0, np.sqrt(np.fmax(p * (1.0 - p), 1.0 / S) / S), np.nan)


def _mc_arguments(who, x, P, target, weight, Phi, Q, steps, dt, radius, particles, seed, transition):
    """What `mc_encounters` and `mc_pair_encounters` share: every check of the model, the sizes and the seed (ValueError under the
    caller's name `who`), the components grouped by target with a STABLE sort, and the cdf of the weights inside every target.  A dict:
    x, P, Phi, Q (float64 arrays), nx, L, steps, S, order [L], targets [T], first [T + 1] (int32), cdf [L], T."""
    X, Pm = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    Phi, Q = np.asarray(Phi, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    nx = X.shape[1] if X.ndim == 2 else -1
    if nx not in (4, 6):
        raise ValueError("%s: the states are an [L, 4] or [L, 6] array (got shape %r)" % (who, X.shape))
    L = len(X)
    if transition not in ("linear", "ct") or (transition == "ct" and nx != 6):
        raise ValueError("%s: transition is \"linear\" or, with six states, \"ct\" (got %r with %d states)" % (who, transition, nx))
    if Pm.shape != (L, nx, nx) or Phi.shape != (nx, nx) or Q.shape != (nx, nx):
        raise ValueError("%s: P, Phi and Q have shapes %r, %r and %r; [%d, %d, %d] and twice [%d, %d] are wanted"
                         % (who, Pm.shape, Phi.shape, Q.shape, L, nx, nx, nx, nx))
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= MC_MAX_STEPS:
        raise ValueError("%s: steps is an integer in 1 .. %d (got %r)" % (who, MC_MAX_STEPS, steps))
    for name, v in (("dt", dt), ("radius", radius)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not v > 0:
            raise ValueError("%s: %s must be a finite positive number (got %r)" % (who, name, v))
    if isinstance(particles, bool) or not isinstance(particles, (int, np.integer)) or not MC_WARP <= particles <= MC_MAX_PARTICLES or particles % MC_WARP:
        raise ValueError("%s: particles is a multiple of %d in %d .. %d (got %r)" % (who, MC_WARP, MC_WARP, MC_MAX_PARTICLES, particles))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
        raise ValueError("%s: seed is an integer in 0 .. 2^64 - 1 (got %r)" % (who, seed))
    if not (np.isfinite(Q).all() and (transition == "ct" or np.isfinite(Phi).all())):
        raise ValueError("%s: Phi and Q must be finite" % who)
    tg, wt = np.asarray(target), np.asarray(weight, dtype=np.float64)
    if tg.shape != (L,) or not np.issubdtype(tg.dtype, np.integer):
        raise ValueError("%s: target is an [L] = [%d] array of integers (got %r)" % (who, L, target))
    if wt.shape != (L,) or (wt < 0).any():
        raise ValueError("%s: weight is an [L] = [%d] array of numbers >= 0 (got %r)" % (who, L, weight))
    order = np.argsort(tg, kind="stable")
    targets, start = np.unique(tg[order], return_index=True)
    T = len(targets)
    first = np.append(start, L).astype(np.int32)
    cdf = np.zeros(L)
    for t in range(T):
        w = wt[order[first[t]:first[t + 1]]]
        total = w.sum()
        if not np.isfinite(total) or not total > 0:
            raise ValueError("%s: the weights of target %d are all 0 or not finite" % (who, int(targets[t])))
        cdf[first[t]:first[t + 1]] = np.cumsum(w / total)
        cdf[first[t + 1] - 1] = 1.0
    return dict(x=X, P=Pm, Phi=Phi, Q=Q, nx=nx, L=L, steps=int(steps), S=int(particles), order=order, targets=targets, first=first, cdf=cdf, T=T)


def _mc_call(a, sizer, seam, extra, mid, shapes, dt, radius, seed, transition, device, ctx, sized=1):
    """The device call `mc_encounters` and `mc_pair_encounters` share, on `_mc_arguments`' dict `a`: x and P packed in `order`, one
    upload (with `extra`, the seam's own device input: the own paths or the pairs' ranks), the work buffer of `sizer`, one int32 tensor
    per entry of `shapes` (name -> shape, in the seam's order), the call of `seam` with `mid` as its middle size argument (G or n),
    and the arrays read back: uint32 counts, `status` int32.  A context of its own where `ctx` is None.  `mc_zone_encounters` calls
    with two device inputs (`extra` a tuple), two middle sizes (`mid` a tuple, of which the sizer takes the first) and no radius
    (None: the seam has none); `mc_domain_encounters` with three of each, of which its sizer takes the first `sized` = 2 middle sizes."""
    nx, L, T, steps, S, order = a["nx"], a["L"], a["T"], a["steps"], a["S"], a["order"]
    extras = extra if isinstance(extra, tuple) else (extra,)
    mids = mid if isinstance(mid, tuple) else (mid,)
    scalars = (int(seed), float(dt)) + (() if radius is None else (float(radius),))
    iu = np.triu_indices(nx)
    xp, Pp = np.ascontiguousarray(a["x"][order].T), np.ascontiguousarray(a["P"][order][:, iu[0], iu[1]].T)
    Phi, Q = np.ascontiguousarray(a["Phi"]), np.ascontiguousarray(a["Q"])
    mine = ctx is None
    if mine:
        ctx = Context(device, nx=nx)
    try:
        dev, lib = ctx.device, ctx.lib
        x_d, P_d, f_d, c_d, *e_d = [torch.from_numpy(v).to(dev) for v in (xp, Pp, a["first"], a["cdf"]) + extras]
        need = int(getattr(lib, sizer)(nx, L, T, *mids[:sized], steps, S))
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        # (uint32 counts in int32 tensors: the same bits)
        out = {name: torch.empty(shape, dtype=torch.int32, device=dev) for name, shape in shapes.items()}
        torch.cuda.current_stream(dev).synchronize()      # (the uploads ran on torch's stream)
        _lib.check(getattr(lib, seam)(ctx.handle, nx, 1 if transition == "ct" else 0, L, T, *mids, steps, S, *scalars, Phi.ctypes.data,
                                      Q.ctypes.data, x_d.data_ptr(), P_d.data_ptr(), f_d.data_ptr(), c_d.data_ptr(), *[t.data_ptr() for t in e_d],
                                      *[t.data_ptr() for t in out.values()], work.data_ptr(), need), lib)
        return {name: t.cpu().numpy() if name == "status" else t.cpu().numpy().view(np.uint32) for name, t in out.items()}
    finally:
        if mine:
            ctx.close()


def mc_encounters(x, P, target, weight, Phi, Q, steps, dt, radius, ownPaths, particles=4096, seed=0, transition="linear", device=0, ctx=None):
    """Encounters by MONTE CARLO: every target is the Gaussian mixture of its components, `particles` particles per target are drawn from
    it, walked over steps * dt seconds WITH the model's process noise, and held against G paths of the own ship
    (csrc/mht_mc.h states the method).  It answers what the Gaussian rule of `encounters` cannot: the probability of coming within
    `radius` AT ANY TIME of the horizon (a first-passage figure over correlated steps, not the largest per-step mass), a target whose
    hypotheses disagree (a mixture is sampled as what it is, not averaged cell by cell), and the constant-turn model, walked with
    Phi(dt, w) at every particle's own turn rate.

    x, P       the components: x [L, nx] (nx 4 or 6), P [L, nx, nx] symmetric (the upper triangle is read); a P may be singular or 0
    target     [L] integers, any order: the target of every component.  The targets of the result are the distinct values, ascending;
               the components are grouped by a STABLE sort, which the result returns as `order`
    weight     [L] >= 0: the components' weights inside their target (any scale).  A target whose weights are all 0, or whose sum is
               not finite, raises ValueError
    Phi, Q     [nx, nx] of one step of dt seconds; Q positive SEMIdefinite (models/ct.Q has rank 3).  transition="ct": Phi is not read
    steps, dt, radius   1 .. 64 steps of dt > 0 seconds; the safety radius > 0
    ownPaths   [G, steps + 1, 2], G in 1 .. 64, finite: the own ship's position at every step, e.g. `mc_own_paths`
    particles  S, a multiple of 64 in 64 .. 2^20;  seed: 0 .. 2^64 - 1 -- one seed, one result, bit for bit (Philox4x32-10, counter
               (particle, step, rank of the target, block): a target's stream does not depend on which component a particle picks)
    transition "linear", or "ct": models/ct.py's six states, x+ = Phi(dt, x[4]) x + noise
    ValueError for arguments that do not fit -- before any device is needed.  No component: empty arrays and no device call.
    Returns a dict.  As the device wrote them: `within` [G, steps + 1, T] and `ever` [G, T] (uint32 counts), `valid` [T] (S for a
    scored target, else 0) and `status` [T] (0; 1: a NaN in a component; 2: a P that is not positive semidefinite).  Derived on the
    host, NaN where valid is 0: `pc` = within / valid; `pcMax` [G, T] and `tpc`, the largest pc over the steps and the time k dt of the
    EARLIEST largest; `pEver` = ever / valid; `sePcMax` and `sePEver`, sqrt(max(p (1 - p), 1 / S) / S) -- a Monte-Carlo figure is not
    to be read without its error bar.  And `targets` [T], `first` [T + 1], `cdf` [L] and `order` [L] as they were used.
    Pairs of targets: `mc_pair_encounters`.  Out of scope: an own-ship covariance, correlation between targets, the time of the first
    violation (`firstAt`, which the pair engine has), more than 2^20 particles.
    One upload, one call of `mht_mc_encounters` (three launches), no host fallback."""
    a = _mc_arguments("mc_encounters", x, P, target, weight, Phi, Q, steps, dt, radius, particles, seed, transition)
    L, steps, order, targets, first, cdf, T = a["L"], a["steps"], a["order"], a["targets"], a["first"], a["cdf"], a["T"]
    try:
        own = np.ascontiguousarray(ownPaths, dtype=np.float64)
    except (TypeError, ValueError):
        own = np.zeros(0)
    if own.ndim != 3 or own.shape[1:] != (steps + 1, 2) or not 1 <= len(own) <= MC_MAX_PATHS or not np.isfinite(own).all():
        raise ValueError("mc_encounters: ownPaths is a finite [G, steps + 1, 2] = [G, %d, 2] array, G in 1 .. %d (got shape %r)" % (steps + 1, MC_MAX_PATHS, own.shape))
    G = len(own)
    res = dict(targets=targets.astype(np.int64), first=first, cdf=cdf, order=order.astype(np.int64))
    if L == 0:
        res.update(within=np.zeros((G, steps + 1, 0), dtype=np.uint32), ever=np.zeros((G, 0), dtype=np.uint32), valid=np.zeros(0, dtype=np.uint32),
                   status=np.zeros(0, dtype=np.int32))
    else:
        res.update(_mc_call(a, "mht_mc_work_bytes", "mht_mc_encounters", own, G, dict(within=(G, steps + 1, T), ever=(G, T), valid=(T,), status=(T,)), dt, radius, seed,
                            transition, device, ctx))
    res.update(mc_derive(res["within"], res["ever"], res["valid"], float(dt)))
    return res


def mc_derive(within, ever, valid, dt):
    """The host's figures of `mc_encounters` from its counts: pc, pcMax, tpc, pEver, sePcMax, sePEver (NaN where valid is 0)"""
    v = np.asarray(valid, dtype=np.float64)
    with np.errstate(all="ignore"):
        pc = np.where(v > 0, within / v, np.nan)
        p_ever = np.where(v > 0, ever / v, np.nan)
    G, K1, T = pc.shape
    pc_max, tpc = np.full((G, T), np.nan), np.full((G, T), np.nan)
    if T:
        scored = v > 0
        arg = np.argmax(np.where(scored, pc, -1.0), axis=1)      # (the first of equal largest)
        pc_max = np.where(scored, np.take_along_axis(pc, arg[:, None, :], axis=1)[:, 0, :], np.nan)
        tpc = np.where(scored, arg * dt, np.nan)
    return dict(pc=pc, pcMax=pc_max, tpc=tpc, pEver=p_ever, sePcMax=mc_standard_error(pc_max, v), sePEver=mc_standard_error(p_ever, v))


# ---- encounters by Monte Carlo between pairs of targets ---------------------------------------------------------------------------------
MC_MAX_PAIRS = 1 << 20      # MHT_MC_MAX_PAIRS, include/mht_amd.h
MC_PAIR_COUNT_NAMES = ("within", "firstAt", "ever", "valid", "status")


def mc_pair_derive(within, firstAt, ever, valid, dt):
    """The host's figures of `mc_pair_encounters` from its counts (within, firstAt [K + 1, n]; ever, valid [n]): pc, pcMax, tpc, pEver,
    sePcMax, sePEver by `mc_derive`'s rules, and pEverBy [K + 1, n] = cumsum(firstAt) / valid.  NaN where valid is 0."""
    d = mc_derive(np.asarray(within)[None], np.asarray(ever)[None], valid, dt)
    out = {k: v[0] for k, v in d.items()}
    v = np.asarray(valid, dtype=np.float64)
    with np.errstate(all="ignore"):
        out["pEverBy"] = np.where(v > 0, np.cumsum(np.asarray(firstAt, dtype=np.int64), axis=0) / v, np.nan)
    return out


def mc_pair_encounters(x, P, target, weight, Phi, Q, steps, dt, radius, pairs, particles=4096, seed=0, transition="linear", device=0, ctx=None):
    """Encounters by MONTE CARLO between PAIRS OF TARGETS: what a VTS operator or a fleet monitor asks for, with the engine of
    `mc_encounters` (csrc/mht_mc_pair.h states the definition).  Every target is the Gaussian mixture of its components; particle p of
    target a is held against particle p of target b, both walked over steps * dt seconds with the model's process noise -- exactly the
    particles `mc_encounters` walks for the same seed, the constant-turn model with Phi(dt, w) at every particle's own turn rate
    included.  With d_k the difference of the two positions at step k, a pair's relative path is the piecewise-linear one through
    d_0 .. d_K.

    x, P, target, weight, Phi, Q, steps, dt, radius, particles, seed, transition   as for `mc_encounters`
    pairs      [n, 2] integers, n <= 2^20: pairs of target VALUES, as they appear in `target`.  Duplicates and both orders of a pair
               are allowed (and give equal counts).  A pair that names a target not present, or one target twice, raises ValueError
    ValueError for arguments that do not fit -- before any device is needed.  No pair or no component: empty arrays, no device call.
    Returns a dict.  As the device wrote them: `within` [steps + 1, n] (the particles within `radius` at step k), `firstAt`
    [steps + 1, n] (the particles whose relative path comes inside `radius` FIRST at step k -- at the step or on the segment that ends
    in it: the distribution of the time to the first violation), `ever` [n] = the sum of firstAt over the steps, `valid` [n] (S for a
    scored pair, else 0) and `status` [n] (0; 1: either target has a NaN in a component; 2: either target has a P that is not positive
    semidefinite).  Derived on the host, NaN where valid is 0: `pc`, `pcMax`, `tpc`, `pEver`, `sePcMax`, `sePEver` by `mc_derive`'s
    rules, and `pEverBy` [steps + 1, n] = cumsum(firstAt) / valid, the probability of having come within `radius` by the time k dt
    (its last row is pEver).  And `pairs` [n, 2] as given, `targets` [T], `first` [T + 1], `cdf` [L] and `order` [L] as they were used.
    Out of scope: correlation between targets (the particles of two targets are independent), an own-ship covariance, pairs across
    `trial_hypotheses`' Gaussian cells, and `firstAt` for the own-ship engine `mc_encounters`.
    One upload, one call of `mht_mc_pair_encounters` (three launches), no host fallback; no particle position is stored, a target in
    many pairs is walked once per pair."""
    who = "mc_pair_encounters"
    a = _mc_arguments(who, x, P, target, weight, Phi, Q, steps, dt, radius, particles, seed, transition)
    L, steps, order, targets, first, cdf, T = a["L"], a["steps"], a["order"], a["targets"], a["first"], a["cdf"], a["T"]
    try:
        pr = np.asarray(pairs)
    except (TypeError, ValueError):
        pr = np.zeros(0)
    if pr.size == 0:
        pr = np.zeros((0, 2), dtype=np.int64)
    if pr.ndim != 2 or pr.shape[1] != 2 or not np.issubdtype(pr.dtype, np.integer) or len(pr) > MC_MAX_PAIRS:
        raise ValueError("%s: pairs is an [n, 2] array of integers, n <= %d (got %r)" % (who, MC_MAX_PAIRS, getattr(pr, "shape", pairs)))
    pr = pr.astype(np.int64)
    n = len(pr)
    rank = np.searchsorted(targets, pr) if T else np.zeros_like(pr)
    there = (targets[np.minimum(rank, T - 1)] == pr) if T else np.zeros(pr.shape, dtype=bool)
    if not there.all():
        j = int(np.flatnonzero(~there.all(axis=1))[0])
        raise ValueError("%s: pair %d is (%d, %d), and target %d has no component" % (who, j, pr[j, 0], pr[j, 1], pr[j][~there[j]][0]))
    if n and (pr[:, 0] == pr[:, 1]).any():
        j = int(np.flatnonzero(pr[:, 0] == pr[:, 1])[0])
        raise ValueError("%s: pair %d names target %d twice" % (who, j, pr[j, 0]))
    res = dict(pairs=pr, targets=targets.astype(np.int64), first=first, cdf=cdf, order=order.astype(np.int64))
    if L == 0 or n == 0:
        res.update(within=np.zeros((steps + 1, 0), dtype=np.uint32), firstAt=np.zeros((steps + 1, 0), dtype=np.uint32), ever=np.zeros(0, dtype=np.uint32),
                   valid=np.zeros(0, dtype=np.uint32), status=np.zeros(0, dtype=np.int32))
    else:
        res.update(_mc_call(a, "mht_mc_pair_work_bytes", "mht_mc_pair_encounters", np.ascontiguousarray(rank, dtype=np.int32), n,
                            dict(within=(steps + 1, n), firstAt=(steps + 1, n), ever=(n,), valid=(n,), status=(n,)), dt, radius, seed, transition, device, ctx))
    res.update(mc_pair_derive(res["within"], res["firstAt"], res["ever"], res["valid"], float(dt)))
    return res


def mc_pair_screen(x, target, weight, horizon, distance, block=256):
    """Which pairs of targets are worth a Monte-Carlo run: A PRE-FILTER, NOT A FIGURE -- a pair it drops gets no result at all, so
    choose `distance` generously (several safety radii plus the spread of the targets' hypotheses over the horizon).  Per target the
    weight-normalised mean of x[:, :4] = [x, y, vx, vy] over its components; per pair the distance at the clamped closest point of
    approach of the two STRAIGHT-LINE motions over [0, horizon]: with r and v the differences of the mean positions and velocities,
    t* = clamp(-(r . v) / (v . v), 0, horizon) (0 for v = 0) and d = |r + t* v|.  For constant-turn targets the straight line is only
    a guide: more generous still.  Host NumPy, a block of rows at a time (2 000 targets need no dense cube).

    x [L, >= 4], target [L] integers, weight [L] >= 0; horizon >= 0 and distance > 0, finite.
    Returns the pairs with d < distance as [n, 2] int64 target VALUES, a < b, ascending.  A target whose mean is NaN (a NaN component of
    positive weight, or weights that are all 0) is in no pair."""
    who = "mc_pair_screen"
    X, tg, wt = np.asarray(x, dtype=np.float64), np.asarray(target), np.asarray(weight, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] < 4:
        raise ValueError("%s: the states are an [L, 4] array or wider (got shape %r)" % (who, X.shape))
    L = len(X)
    if tg.shape != (L,) or not np.issubdtype(tg.dtype, np.integer):
        raise ValueError("%s: target is an [L] = [%d] array of integers (got %r)" % (who, L, target))
    if wt.shape != (L,) or not (wt >= 0).all():
        raise ValueError("%s: weight is an [L] = [%d] array of numbers >= 0 (got %r)" % (who, L, weight))
    for name, v, low in (("horizon", horizon, True), ("distance", distance, False)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not (v >= 0 if low else v > 0):
            raise ValueError("%s: %s must be a finite number %s 0 (got %r)" % (who, name, ">=" if low else ">", v))
    targets, inv = np.unique(tg, return_inverse=True)
    T = len(targets)
    mean = np.zeros((T, 4))
    total = np.zeros(T)
    for i in range(4):
        # (a component of weight 0 does not enter, whatever its state: 0 * NaN would)
        np.add.at(mean[:, i], inv, np.where(wt > 0, wt * X[:, i], 0.0))
    np.add.at(total, inv, wt)
    with np.errstate(all="ignore"):
        mean = mean / total[:, None]
    ok = np.isfinite(mean).all(axis=1)
    h, d2max = float(horizon), float(distance) * float(distance)
    keep = []
    for lo in range(0, T, int(block)):
        hi = min(lo + int(block), T)
        r = mean[lo:hi, None, :2] - mean[None, :, :2]
        v = mean[lo:hi, None, 2:] - mean[None, :, 2:]
        rv, vv = r[..., 0] * v[..., 0] + r[..., 1] * v[..., 1], v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]
        with np.errstate(all="ignore"):
            ts = np.where(vv > 0, np.fmin(np.fmax(-rv / np.where(vv > 0, vv, 1.0), 0.0), h), 0.0)
            cx, cy = r[..., 0] + ts * v[..., 0], r[..., 1] + ts * v[..., 1]
            near = cx * cx + cy * cy < d2max
        near &= ok[lo:hi, None] & ok[None, :] & (np.arange(lo, hi)[:, None] < np.arange(T)[None, :])
        a, b = np.nonzero(near)
        keep.append(np.stack([targets[a + lo], targets[b]], axis=1))
    out = np.concatenate(keep, axis=0) if keep else np.zeros((0, 2))
    return np.ascontiguousarray(out, dtype=np.int64).reshape(-1, 2)


# ---- guard zones by Monte Carlo: targets entering polygons, with entry times ---------------------------------------------------------
MC_ZONE_MAX_ZONES, MC_ZONE_MAX_VERTS = 32, 1024      # MHT_MC_ZONE_*, include/mht_amd.h


def mc_zone_pack(zones, who="mc_zone_pack"):
    """A list of polygons, each a finite [V, 2] array with V >= 3, as `mht_mc_zone_encounters` takes them: (zoneFirst int32 [Z + 1],
    zoneXY float64 [nVert, 2]).  At most 32 zones and 1 024 vertices in all.  ValueError (under the caller's name `who`) otherwise."""
    if isinstance(zones, np.ndarray) and zones.ndim != 3:
        raise ValueError("%s: zones is a LIST of [V, 2] arrays, one per zone (got an array of shape %r)" % (who, zones.shape))
    try:
        polys = [np.asarray(z, dtype=np.float64) for z in zones]
    except (TypeError, ValueError):
        raise ValueError("%s: zones is a list of [V, 2] arrays of numbers (got %r)" % (who, zones))
    if len(polys) > MC_ZONE_MAX_ZONES:
        raise ValueError("%s: at most %d zones (got %d)" % (who, MC_ZONE_MAX_ZONES, len(polys)))
    for z, poly in enumerate(polys):
        if poly.ndim != 2 or poly.shape[1] != 2 or len(poly) < 3:
            raise ValueError("%s: zone %d is a [V, 2] array with V >= 3 (got shape %r)" % (who, z, poly.shape))
        if not np.isfinite(poly).all():
            raise ValueError("%s: zone %d has a vertex that is not finite" % (who, z))
    first = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
    if first[-1] > MC_ZONE_MAX_VERTS:
        raise ValueError("%s: at most %d vertices in all zones together (got %d)" % (who, MC_ZONE_MAX_VERTS, int(first[-1])))
    xy = np.concatenate(polys, axis=0) if polys else np.zeros((0, 2))
    return first, np.ascontiguousarray(xy, dtype=np.float64)


def mc_zone_derive(inside, firstAt, ever, valid, dt):
    """The host's figures of `mc_zone_encounters` from its counts (inside, firstAt [Z, K + 1, T]; ever [Z, T]; valid [T]): pInside =
    inside / valid; pInsideMax [Z, T] and tInside, the largest pInside over the steps and the time k dt of the EARLIEST largest; pEver =
    ever / valid; pEverBy [Z, K + 1, T] = cumsum(firstAt) / valid, the probability of having entered by the time k dt (its last row is
    pEver); sePInsideMax and sePEver by `mc_standard_error`.  NaN where valid is 0."""
    d = mc_derive(inside, ever, valid, dt)
    v = np.asarray(valid, dtype=np.float64)
    with np.errstate(all="ignore"):
        by = np.where(v > 0, np.cumsum(np.asarray(firstAt, dtype=np.int64), axis=1) / v, np.nan)
    return dict(pInside=d["pc"], pInsideMax=d["pcMax"], tInside=d["tpc"], pEver=d["pEver"], pEverBy=by, sePInsideMax=d["sePcMax"], sePEver=d["sePEver"])


def mc_zone_encounters(x, P, target, weight, Phi, Q, steps, dt, zones, particles=4096, seed=0, transition="linear", device=0, ctx=None):
    """GUARD ZONES by MONTE CARLO: will a target enter a PLACE -- a restricted area, a shoal contour, an anchorage, a traffic-separation
    zone --, with what probability within the horizon, and when.  The engine is `mc_encounters`' (csrc/mht_mc_zone.h states the
    definition): every target is the Gaussian mixture of its components, its particles are walked over steps * dt seconds with the
    model's process noise -- exactly the particles `mc_encounters` and `mc_pair_encounters` walk for the same seed, the constant-turn
    model with Phi(dt, w) at every particle's own turn rate included -- and held against every zone: a point-in-polygon test at every
    step (the zone's box, then the crossing number) and the path segment between two steps against the zone's edges, so that a zone
    thinner than one step's travel is not stepped over.

    x, P, target, weight, Phi, Q, steps, dt, particles, seed, transition   as for `mc_encounters`; there is no radius
    zones      a list of at most 32 simple polygons, each a finite [V, 2] array of vertices in metres, V >= 3, at most 1 024 vertices
               in all; either orientation, concave polygons included; the edge from the last vertex to the first is implied
    ValueError for arguments that do not fit -- before any device is needed.  No zone or no component: empty arrays, no device call.
    Returns a dict.  As the device wrote them: `inside` [Z, steps + 1, T] (the particles inside the zone at step k), `firstAt`
    [Z, steps + 1, T] (the particles that are inside the zone, or whose segment k - 1 -> k meets an edge of it, FIRST at step k: the
    distribution of the time of entry), `ever` [Z, T] = the sum of firstAt over the steps, `valid` [T] and `status` [T] as for
    `mc_encounters`.  Derived on the host by `mc_zone_derive`, NaN where valid is 0: `pInside`, `pInsideMax`, `tInside`, `pEver`,
    `pEverBy`, `sePInsideMax`, `sePEver`.  And `zoneFirst` [Z + 1], `zoneXY` [nVert, 2], `targets` [T], `first` [T + 1], `cdf` [L] and
    `order` [L] as they were used.
    Zones that move with the own ship (a polygonal ship domain) are `mc_domain_encounters`' case.  Out of scope: open gates and
    polylines (a thin quadrilateral serves), holes, geodetic coordinates, the dwell time inside a zone.
    One upload, one call of `mht_mc_zone_encounters` (three launches), no host fallback."""
    who = "mc_zone_encounters"
    a = _mc_arguments(who, x, P, target, weight, Phi, Q, steps, dt, 1.0, particles, seed, transition)
    L, steps, order, targets, first, cdf, T = a["L"], a["steps"], a["order"], a["targets"], a["first"], a["cdf"], a["T"]
    zf, zxy = mc_zone_pack(zones, who)
    Z = len(zf) - 1
    res = dict(zoneFirst=zf, zoneXY=zxy, targets=targets.astype(np.int64), first=first, cdf=cdf, order=order.astype(np.int64))
    if L == 0 or Z == 0:
        T = T if Z else 0
        res.update(inside=np.zeros((Z, steps + 1, T), dtype=np.uint32), firstAt=np.zeros((Z, steps + 1, T), dtype=np.uint32), ever=np.zeros((Z, T), dtype=np.uint32),
                   valid=np.zeros(T, dtype=np.uint32), status=np.zeros(T, dtype=np.int32))
    else:
        res.update(_mc_call(a, "mht_mc_zone_work_bytes", "mht_mc_zone_encounters", (zf, zxy), (Z, len(zxy)),
                            dict(inside=(Z, steps + 1, T), firstAt=(Z, steps + 1, T), ever=(Z, T), valid=(T,), status=(T,)), dt, None, seed, transition, device, ctx))
    res.update(mc_zone_derive(res["inside"], res["firstAt"], res["ever"], res["valid"], float(dt)))
    return res


# ---- ship domains by Monte Carlo: a polygon carried along the own ship's paths ---------------------------------------------------------
MC_DOMAIN_MAX_DOMAINS, MC_DOMAIN_MAX_VERTS, MC_DOMAIN_MAX_CELLS = 4, 256, 64      # MHT_MC_DOMAIN_*, include/mht_amd.h
MC_DOMAIN_COUNT_NAMES = ("inside", "firstAt", "ever", "valid", "status")


def mc_own_poses(own, candidates, turnRate, steps, dt):
    """The own ship's POSES at t = k dt, k = 0 .. steps, for every candidate manoeuvre (dpsi, f, t0): float64 [G, steps + 1, 4] =
    (x, y, ux, uy).  Columns 0:2 are `mc_own_paths`' positions, bit for bit (it is called, not restated); columns 2:4 are the unit
    heading vector: u0 = v0 / hypot(v0x, v0y) rotated by the manoeuvre's own angle -- 0 until t0, sg w (t - t0) on the arc,
    sg |dpsi| after te = t0 + |dpsi| / w, counter-clockwise for dpsi > 0 as csrc/mht_trial.h defines a candidate --, with sin and cos of
    those angles.  An own ship of speed 0 has no heading: ValueError (a stationary ship with a guard ring is `mc_zone_encounters`'
    case).  A NaN in a candidate or in `own` makes that candidate's poses NaN.  ValueError otherwise as `mc_own_paths` raises them."""
    try:
        paths = mc_own_paths(own, candidates, turnRate, steps, dt)
    except ValueError as exc:
        raise ValueError(str(exc).replace("mc_own_paths", "mc_own_poses", 1))
    w, dt = float(turnRate), float(dt)
    cand = trial_candidates(candidates)
    _, _, v0x, v0y = np.ascontiguousarray(own, dtype=np.float64)
    speed = np.hypot(v0x, v0y)
    if speed == 0:
        raise ValueError("mc_own_poses: an own ship of speed 0 has no heading (got own = %r)" % (own,))
    u0x, u0y = v0x / speed, v0y / speed
    dpsi, t0 = cand[:, 0], cand[:, 2]
    out = np.zeros((len(cand), int(steps) + 1, 4))
    out[:, :, :2] = paths
    with np.errstate(all="ignore"):
        ad = np.abs(dpsi)
        sg = np.where(dpsi > 0, 1.0, np.where(dpsi < 0, -1.0, 0.0))
        te = t0 + ad / w
        for k in range(int(steps) + 1):
            t = float(k) * dt
            ang = np.where(t <= t0, 0.0, np.where(t <= te, sg * (w * (t - t0)), sg * ad))
            s, c = np.sin(ang), np.cos(ang)
            out[:, k, 2] = c * u0x - s * u0y
            out[:, k, 3] = s * u0x + c * u0y
    out[np.isnan(paths).any(axis=(1, 2))] = np.nan
    return out


def mc_domain_pack(domains, who="mc_domain_pack"):
    """A list of polygons in the own ship's BODY FRAME (first coordinate to the right of the heading, second ahead; drawn bow-up), each a
    finite [V, 2] array with V >= 3, as `mht_mc_domain_encounters` takes them: (domFirst int32 [nDomain + 1], domXY float64 [nVert, 2]).
    At most 4 domains and 256 vertices in all.  ValueError (under the caller's name `who`) otherwise."""
    if isinstance(domains, np.ndarray) and domains.ndim != 3:
        raise ValueError("%s: domains is a LIST of [V, 2] arrays, one per domain (got an array of shape %r)" % (who, domains.shape))
    try:
        polys = [np.asarray(d, dtype=np.float64) for d in domains]
    except (TypeError, ValueError):
        raise ValueError("%s: domains is a list of [V, 2] arrays of numbers (got %r)" % (who, domains))
    if len(polys) > MC_DOMAIN_MAX_DOMAINS:
        raise ValueError("%s: at most %d domains (got %d)" % (who, MC_DOMAIN_MAX_DOMAINS, len(polys)))
    for d, poly in enumerate(polys):
        if poly.ndim != 2 or poly.shape[1] != 2 or len(poly) < 3:
            raise ValueError("%s: domain %d is a [V, 2] array with V >= 3 (got shape %r)" % (who, d, poly.shape))
        if not np.isfinite(poly).all():
            raise ValueError("%s: domain %d has a vertex that is not finite" % (who, d))
    first = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
    if first[-1] > MC_DOMAIN_MAX_VERTS:
        raise ValueError("%s: at most %d vertices in all domains together (got %d)" % (who, MC_DOMAIN_MAX_VERTS, int(first[-1])))
    xy = np.concatenate(polys, axis=0) if polys else np.zeros((0, 2))
    return first, np.ascontiguousarray(xy, dtype=np.float64)


def mc_domain_derive(inside, firstAt, ever, valid, dt):
    """The host's figures of `mc_domain_encounters` from its counts (inside, firstAt [nDomain, G, K + 1, T]; ever [nDomain, G, T]; valid
    [T]): `mc_zone_derive`'s fields -- pInside, pInsideMax, tInside, pEver, pEverBy, sePInsideMax, sePEver, NaN where valid is 0 -- over
    the cell axes [nDomain, G]."""
    inside, firstAt, ever = np.asarray(inside), np.asarray(firstAt), np.asarray(ever)
    D, G, K1, T = inside.shape
    d = mc_zone_derive(inside.reshape(D * G, K1, T), firstAt.reshape(D * G, K1, T), ever.reshape(D * G, T), valid, dt)
    return {k: v.reshape((D, G) + v.shape[1:]) for k, v in d.items()}


def mc_domain_encounters(x, P, target, weight, Phi, Q, steps, dt, domains, ownPoses, particles=4096, seed=0, transition="linear", device=0, ctx=None):
    """SHIP DOMAINS by MONTE CARLO: will a target enter the safety region AROUND THE OWN SHIP -- a polygon, longer ahead than astern and
    usually wider to starboard than to port, that translates and rotates with the ship --, with what probability within the horizon,
    and when, for every candidate path of the own ship.  A disc (`mc_encounters`) cannot tell "passes 300 m astern" from "passes 300 m
    ahead", and a fixed zone (`mc_zone_encounters`) cannot follow a candidate manoeuvre.  The engine is theirs (csrc/mht_mc_domain.h
    states the definition): exactly the particles they walk for the same seed, taken into the own ship's body frame under the pose of
    every (path, step) and held there against every domain with `mc_zone_encounters`' geometry -- a point-in-polygon test at every step
    and the segment between two steps against the domain's edges.

    x, P, target, weight, Phi, Q, steps, dt, particles, seed, transition   as for `mc_encounters`; there is no radius
    domains    a list of at most 4 simple polygons IN THE BODY FRAME, each a finite [V, 2] array of vertices in metres, V >= 3, at most
               256 vertices in all: THE FIRST COORDINATE IS TO THE RIGHT OF THE HEADING, THE SECOND AHEAD (x east, y north: starboard
               and ahead; a domain is drawn bow-up).  Either orientation, concave allowed, no holes
    ownPoses   [G, steps + 1, 4] = (x, y, ux, uy), finite, G >= 1 and nDomain * G <= 64: the own ship's position and UNIT heading vector
               (|ux^2 + uy^2 - 1| <= 1e-9) at every step, e.g. `mc_own_poses`
    THE BODY-FRAME PATH BETWEEN TWO STEPS IS TAKEN AS STRAIGHT, from the point under pose k - 1 to the point under pose k: exact where the
    own ship does not turn between the two steps, a chord of a curved path on a step inside an arc.  Shorter steps during a manoeuvre
    are the remedy.
    ValueError for arguments that do not fit -- before any device is needed.  No component: empty arrays and no device call.
    Returns a dict.  As the device wrote them: `inside` and `firstAt` [nDomain, G, steps + 1, T], `ever` [nDomain, G, T] (the counts of
    `mc_zone_encounters` per (domain, path)), `valid` [T] and `status` [T].  Derived on the host by `mc_domain_derive`, NaN where valid
    is 0: `pInside`, `pInsideMax`, `tInside`, `pEver`, `pEverBy`, `sePInsideMax`, `sePEver`.  And `domFirst`, `domXY`, `ownPoses`,
    `targets` [T], `first` [T + 1], `cdf` [L] and `order` [L] as they were used.
    Out of scope: domains around targets or between pairs of targets, a domain that scales with speed, the own ship's covariance, a
    curved body-frame path inside a turning step, holes, more than 64 cells, a stationary own ship.
    One upload, one call of `mht_mc_domain_encounters` (three launches), no host fallback."""
    who = "mc_domain_encounters"
    a = _mc_arguments(who, x, P, target, weight, Phi, Q, steps, dt, 1.0, particles, seed, transition)
    L, steps, order, targets, first, cdf, T = a["L"], a["steps"], a["order"], a["targets"], a["first"], a["cdf"], a["T"]
    df, dxy = mc_domain_pack(domains, who)
    D = len(df) - 1
    if D < 1:
        raise ValueError("%s: one domain at least is wanted" % who)
    try:
        pose = np.ascontiguousarray(ownPoses, dtype=np.float64)
    except (TypeError, ValueError):
        pose = np.zeros(0)
    if pose.ndim != 3 or pose.shape[1:] != (steps + 1, 4) or len(pose) < 1 or not np.isfinite(pose).all():
        raise ValueError("%s: ownPoses is a finite [G, steps + 1, 4] = [G, %d, 4] array, G >= 1 (got shape %r)" % (who, steps + 1, pose.shape))
    G = len(pose)
    if D * G > MC_DOMAIN_MAX_CELLS:
        raise ValueError("%s: at most %d cells, nDomain * G (got %d domains x %d paths)" % (who, MC_DOMAIN_MAX_CELLS, D, G))
    if (np.abs(pose[..., 2] * pose[..., 2] + pose[..., 3] * pose[..., 3] - 1.0) > 1e-9).any():
        raise ValueError("%s: every heading (ownPoses[..., 2:4]) is a unit vector, |ux^2 + uy^2 - 1| <= 1e-9" % who)
    res = dict(domFirst=df, domXY=dxy, ownPoses=pose, targets=targets.astype(np.int64), first=first, cdf=cdf, order=order.astype(np.int64))
    if L == 0:
        res.update(inside=np.zeros((D, G, steps + 1, 0), dtype=np.uint32), firstAt=np.zeros((D, G, steps + 1, 0), dtype=np.uint32),
                   ever=np.zeros((D, G, 0), dtype=np.uint32), valid=np.zeros(0, dtype=np.uint32), status=np.zeros(0, dtype=np.int32))
    else:
        res.update(_mc_call(a, "mht_mc_domain_work_bytes", "mht_mc_domain_encounters", (pose, df, dxy), (G, D, len(dxy)),
                            dict(inside=(D, G, steps + 1, T), firstAt=(D, G, steps + 1, T), ever=(D, G, T), valid=(T,), status=(T,)), dt, None, seed, transition, device,
                            ctx, sized=2))
    res.update(mc_domain_derive(res["inside"], res["firstAt"], res["ever"], res["valid"], float(dt)))
    return res


# ---- the k best global hypotheses ---------------------------------------------------------------------------------------------------
KBEST_MAX_K, KBEST_MAX_TARGETS, KBEST_MAX_COLUMNS, KBEST_MAX_DEPTH, KBEST_MAX_ROWS = 64, 32, 1024, 16, 2048      # MHT_KBEST_*, include/mht_amd.h
KBEST_OK, KBEST_NODE_LIMIT, KBEST_TOO_LARGE, KBEST_BAD_ROWS = 0, 1, 2, 3


def k_best_prep(target, rows):
    """Host preparation of k_best_hypotheses (NumPy and SciPy): the clusters and the cluster-local row ids.

    target [L] non-decreasing target indices, rows [L, D] keys >= 0 or -1.  Two targets belong together when leaves of theirs share a
    key; the clusters are the connected components.  Returns (group_ptr [T + 1], cluster_ptr [C + 1], cluster_targets [T] -- the
    clusters in order of their smallest target, ascending inside --, local [D, L] int32: every key replaced by its rank among the keys
    of its cluster, -1 kept)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    tg = np.asarray(target, dtype=np.int64)
    R = np.asarray(rows, dtype=np.int64).reshape(len(tg), -1)
    L, D = R.shape
    T = int(tg[-1]) + 1 if L else 0
    group_ptr = np.searchsorted(tg, np.arange(T + 1)).astype(np.int32)
    leaf, d = np.nonzero(R >= 0)
    keys, kid = np.unique(R[leaf, d], return_inverse=True)
    nK = len(keys)
    g = coo_matrix((np.ones(len(leaf), dtype=np.int8), (tg[leaf], T + kid)), shape=(T + nK, T + nK))
    _, lab = connected_components(g, directed=False)
    # clusters in order of their smallest target
    first = np.full(lab.max() + 1 if len(lab) else 0, T, dtype=np.int64)
    np.minimum.at(first, lab[:T], np.arange(T))
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(first), dtype=np.int64)
    rank[order] = np.arange(len(first))
    tc = rank[lab[:T]]                                  # cluster of every target, 0 .. C - 1
    C_ = int(tc.max()) + 1 if T else 0
    cluster_targets = np.argsort(tc, kind="stable").astype(np.int32)
    cluster_ptr = np.searchsorted(tc[cluster_targets], np.arange(C_ + 1)).astype(np.int32)
    # a key's local id: its rank among the keys of its cluster (the keys are sorted, so the rank is by value)
    kc = rank[lab[T:]]
    ko = np.argsort(kc, kind="stable")
    start = np.searchsorted(kc[ko], np.arange(C_ + 1))
    loc = np.empty(nK, dtype=np.int64)
    loc[ko] = np.arange(nK) - start[kc[ko]]
    local = np.full((max(D, 1), max(L, 1)), -1, dtype=np.int32)
    local[d, leaf] = loc[kid]
    return group_ptr, cluster_ptr, cluster_targets, local


def k_best_hypotheses(cost, target, rows, k, nodeLimit=1 << 20, device=0, ctx=None):
    """The k best GLOBAL hypotheses of every cluster of a leaf set, and what they say about every leaf.

    cost [L]     the cost of every leaf (a Tracker's: cnllr), in leafBatch() order; a leaf whose cost is not finite is never picked
    target [L]   its target index, non-decreasing
    rows [L, D]  the keys of the plots on its window path: arbitrary non-negative integers, -1 for none
    k            1 .. 64 hypotheses listed per cluster;  nodeLimit  sibling tests after which a cluster's search stops
    device, ctx  the GPU ordinal, or an existing pymht_amd.device.Context (a Tracker's) to run on
    A global hypothesis picks one leaf per target so that no two picked leaves share a key; its cost is the float64 sum of the picked
    costs in target order.  The clusters are the connected components of targets whose leaves share a key -- FINER than the scan's
    gating clusters, which join targets that merely gated the same plot at some scan.  Host preparation (k_best_prep) relabels the keys
    per cluster; one device call follows (`mht_kbest_hypotheses`, a branch and bound per cluster, no host fallback).
    Returns a dict:
        clusters         list of int arrays: the targets of every cluster, ascending
        count [C]        hypotheses listed (fewer than k: no more exist);  status [C]: 0 exact, 1 the node limit fired (the best found so
                         far, not certified), 2 not searched (more than 32 targets, 1024 leaves or 16 keys per leaf), 3 not searched
                         (more than 2048 distinct keys);  nodes [C] sibling tests made
        cost [C, k]      ascending, ties by the tuple of leaf indices;  prob [C, k] = exp(-(cost - cost[:, :1])) normalised over the k
                         LISTED hypotheses -- truncated, not the probability among all;  NaN beyond count
        selection [k, T] the leaf of every target in hypothesis r of its cluster, -1 beyond count
        leafProbability [L]  the sum of prob over the listed hypotheses that hold the leaf, equally truncated; 0 for a leaf in none
    Clusters that were not searched are flagged, not guessed: their counts are 0 and their leafProbability is NaN.
    Empty input gives empty arrays and no device call."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= KBEST_MAX_K:
        raise ValueError("k_best_hypotheses: k is an integer in 1 .. %d (got %r)" % (KBEST_MAX_K, k))
    if isinstance(nodeLimit, bool) or not isinstance(nodeLimit, (int, np.integer)) or not 1 <= nodeLimit < 2 ** 31:
        raise ValueError("k_best_hypotheses: nodeLimit is an integer in 1 .. 2^31 - 1 (got %r)" % (nodeLimit,))
    cn = np.ascontiguousarray(cost, dtype=np.float64)
    if cn.ndim != 1:
        raise ValueError("k_best_hypotheses: cost is an [L] array (got shape %r)" % (cn.shape,))
    L = len(cn)
    tg = np.asarray(target)
    if tg.shape != (L,) or (L and (not np.issubdtype(tg.dtype, np.integer) or tg[0] < 0 or (np.diff(tg) < 0).any())):
        raise ValueError("k_best_hypotheses: target is a non-decreasing [L] = [%d] array of target indices >= 0" % L)
    R = np.asarray(rows)
    if R.ndim != 2 or R.shape[0] != L or (R.size and (not np.issubdtype(R.dtype, np.integer) or (R < -1).any())):
        raise ValueError("k_best_hypotheses: rows is an [L, D] = [%d, D] integer array of keys >= 0 or -1" % L)
    k, D = int(k), int(R.shape[1])
    if L == 0:
        return {"clusters": [], "count": np.zeros(0, dtype=np.int32), "status": np.zeros(0, dtype=np.int32), "nodes": np.zeros(0, dtype=np.int32),
                "cost": np.zeros((0, k)), "prob": np.zeros((0, k)), "selection": np.zeros((k, 0), dtype=np.int64), "leafProbability": np.zeros(0)}
    group_ptr, cluster_ptr, cluster_targets, local = k_best_prep(tg, R)
    T, nC = len(group_ptr) - 1, len(cluster_ptr) - 1
    mine = ctx is None
    if mine:
        ctx = Context(device)
    try:
        dev, lib = ctx.device, ctx.lib
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        gp_d, cp_d, ct_d, rw_d, c_d = up(group_ptr), up(cluster_ptr), up(cluster_targets), up(local), up(cn)
        ints = torch.empty((3, nC), dtype=torch.int32, device=dev)
        hyp = torch.empty((2, k, nC), dtype=torch.float64, device=dev)
        sel_d = torch.empty((k, T), dtype=torch.int32, device=dev)
        mar_d = torch.empty(L, dtype=torch.float64, device=dev)
        need = int(lib.mht_kbest_work_bytes(L, T, nC, D, k))
        work = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()      # (the uploads ran on torch's stream)
        _lib.check(lib.mht_kbest_hypotheses(ctx.handle, L, T, nC, D, k, int(nodeLimit), gp_d.data_ptr(), rw_d.data_ptr(), c_d.data_ptr(), cp_d.data_ptr(),
                                            ct_d.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), hyp[0].data_ptr(), hyp[1].data_ptr(),
                                            sel_d.data_ptr(), mar_d.data_ptr(), work.data_ptr(), need), lib)
        _lib.check(lib.mht_synchronize(ctx.handle), lib)
        ints, hyp, sel, mar = ints.cpu().numpy(), hyp.cpu().numpy(), sel_d.cpu().numpy(), mar_d.cpu().numpy()
    finally:
        if mine:
            ctx.close()
    return {"clusters": [cluster_targets[cluster_ptr[c]:cluster_ptr[c + 1]].astype(np.int64) for c in range(nC)],
            "count": ints[0].copy(), "status": ints[1].copy(), "nodes": ints[2].copy(), "cost": np.ascontiguousarray(hyp[0].T),
            "prob": np.ascontiguousarray(hyp[1].T), "selection": sel.astype(np.int64), "leafProbability": mar}
