"""Scoring a tracking result against ground truth on the device: GOSPA per step (`mht_gospa_steps`, include/mht_amd.h).

The figures of pymht_amd.smoothing (log-likelihood, NIS, the likelihood surface, the innovation sequence) need no ground truth and
say whether the FILTER is tuned; they cannot say whether the tracker found the targets.  GOSPA (generalised optimal sub-pattern
assignment, Rahmathullah, Garcia-Fernandez and Svensson 2017, alpha = 2) can: at each step one distance between the set of estimates
and the set of true positions, which splits exactly into a localisation error, a missed-target cost and a false-track cost,

    total = min over partial one-to-one assignments of  sum d_ij^p + c^p / 2 (n + m - 2 |assigned|),     gospa = total^(1/p)

with d_ij = |x_i - y_j| and only pairs with d_ij < c (strictly) assignable.  A step is an optimal assignment, the steps of a run do
not depend on each other: `gospa_steps` packs them, uploads once and solves all of them in ONE launch, one step per workgroup
(csrc/mht_gospa.hip).  There is no host fallback.  `id_switches` counts track switches from the per-step matches on the host, and
`Tracker.getGospa` scores a tracker's track histories against a scenario's truth."""
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
