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
histories."""
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
