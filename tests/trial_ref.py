"""NumPy restatement of what `mht_trial_manoeuvres` computes (include/mht_amd.h, csrc/mht_trial.h): the path of a manoeuvring own ship
per candidate (dpsi, f, t0), every sum in the order the header writes it, the table of candidates x tracks, and the fold of a row to
its worst track.  The tracks' propagation and the five figures of a cell are tests/encounter_ref.py's, imported: a candidate is an
entry whose trajectory is the closed form here instead of the linear propagation, and `manoeuvres` hands encounter_ref.encounters the
trajectories of candidates (entries 0 .. G - 1, first = G) and tracks (behind them) in place of its own propagation.

Twice, as that file does: in float64 (the yardstick) and as the truth in np.longdouble (pc: mpmath at 30 digits, or with pc_mp=False the
float64 rule on the longdouble d_k and Sigma_k).  A result is a dict of [G, n] arrays tcpa, dcpa, md2, pc, tpc and pck [K + 1, G, n]."""
import numpy as np

import encounter_ref as ref

NAMES = ref.NAMES
SUMMARY = ("pcMax", "pcArg", "dcpaMin", "dcpaArg")


def candidate_path(own, Sown, w, cand, K, dt, dtype=np.float64):
    """own [4] (p0, v0), Sown [3] (xx, xy, yy), w, cand [G, 3] (dpsi, f, t0): pos [K + 1, G, 2], S [K + 1, G, 3] in `dtype`, the header's
    operations in the header's order.  A NaN in a candidate, in own or in Sown makes the candidate NaN throughout."""
    own, Sown, cand = [np.asarray(v, dtype=np.float64).astype(dtype) for v in (own, Sown, cand)]
    w, dt = dtype(w), dtype(dt)
    G = len(cand)
    p0x, p0y, v0x, v0y = own
    dpsi, f, t0 = cand[:, 0], cand[:, 1], cand[:, 2]
    bad = np.isnan(cand).any(axis=1) | np.isnan(own).any() | np.isnan(Sown).any()
    one, zero = dtype(1), dtype(0)
    pos, S = np.zeros((K + 1, G, 2), dtype=dtype), np.zeros((K + 1, G, 3), dtype=dtype)
    with np.errstate(all="ignore"):
        ad = np.abs(dpsi)
        sg = np.where(dpsi > 0, one, np.where(dpsi < 0, -one, zero)).astype(dtype)
        te = t0 + ad / w
        ax, ay = p0x + t0 * v0x, p0y + t0 * v0y
        se, ce = np.sin(ad), np.cos(ad)
        swe, cwe = se / w, (one - ce) / w
        bx, by = ax + f * (swe * v0x - (sg * cwe) * v0y), ay + f * ((sg * cwe) * v0x + swe * v0y)
        ux, uy = f * (ce * v0x - (sg * se) * v0y), f * ((sg * se) * v0x + ce * v0y)
        for k in range(K + 1):
            t = dtype(k) * dt
            tau = t - t0
            s, c = np.sin(w * tau), np.cos(w * tau)
            sw, cw = s / w, (one - c) / w
            arc_x, arc_y = ax + f * (sw * v0x - (sg * cw) * v0y), ay + f * ((sg * cw) * v0x + sw * v0y)
            r = t - te
            pos[k, :, 0] = np.where(t <= t0, p0x + t * v0x, np.where(t <= te, arc_x, bx + r * ux))
            pos[k, :, 1] = np.where(t <= t0, p0y + t * v0y, np.where(t <= te, arc_y, by + r * uy))
            S[k] = Sown[None, :]
    pos[:, bad], S[:, bad] = np.nan, np.nan
    return pos, S


def path_branches(own, w, cand):
    """ONE candidate in np.longdouble: (t0, te, [stand_on, arc, straight]) -- the three branches of the manoeuvre's statement as functions
    of t, each valid on its own interval and evaluable at its ends, written from the statement (not in the header's operation order)."""
    L = np.longdouble
    p0, v0 = np.asarray(own[:2], dtype=np.float64).astype(L), np.asarray(own[2:], dtype=np.float64).astype(L)
    dpsi, f, t0 = [L(v) for v in cand]
    w = L(w)
    sg = L(np.sign(float(dpsi)))
    te = t0 + abs(dpsi) / w

    def arc(t):
        sw, cw = np.sin(w * (t - t0)) / w, (1 - np.cos(w * (t - t0))) / w
        return p0 + t0 * v0 + f * np.array([sw * v0[0] - sg * cw * v0[1], sg * cw * v0[0] + sw * v0[1]])
    rot = np.array([[np.cos(dpsi), -np.sin(dpsi)], [np.sin(dpsi), np.cos(dpsi)]])
    return t0, te, [lambda t: p0 + L(t) * v0, lambda t: arc(L(t)), lambda t: arc(te) + (L(t) - te) * f * (rot @ v0)]


def manoeuvres(x, P, Phi, Q, K, dt, R, own, Sown, w, cand, truth=False, pc_mp=True):
    """The seam's table over [G, n], float64 or (truth=True) np.longdouble; the figures are encounter_ref.encounters' on the trajectories
    of the candidates and the tracks."""
    dtype = np.longdouble if truth else np.float64
    x, P, cand = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64), np.asarray(cand, dtype=np.float64)
    G, n = len(cand), len(x)
    tp, tS = ref.propagate(x, P, Phi, Q, K, dtype)
    cp, cS = candidate_path(own, Sown, w, cand, K, dt, dtype)
    pos, S = np.concatenate([cp, tp], axis=1), np.concatenate([cS, tS], axis=1)
    kept = ref.propagate
    ref.propagate = lambda *a, **kw: (pos, S)      # (encounters looks its propagation up in its module: these are the trajectories it pairs)
    try:
        full = ref.encounters(np.zeros((G + n, x.shape[1])), None, Phi, Q, K, dt, R, first=G, truth=truth, pc_mp=pc_mp)
    finally:
        ref.propagate = kept
    return {k: np.ascontiguousarray(v[..., G:]) for k, v in full.items()}


def fold(pc, dcpa):
    """The summary of a table: per row the largest pc and the smallest dcpa with their (lowest) track index, NaN cells left out; NaN and
    -1 for a row without a figure.  Returns the dict pcMax, pcArg, dcpaMin, dcpaArg (indices int64)."""
    G = len(pc)
    out = dict(pcMax=np.full(G, np.nan), pcArg=np.full(G, -1, dtype=np.int64), dcpaMin=np.full(G, np.nan), dcpaArg=np.full(G, -1, dtype=np.int64))
    for g in range(G):
        if not np.isnan(pc[g]).all():
            out["pcMax"][g] = np.nanmax(pc[g])
            out["pcArg"][g] = int(np.flatnonzero(pc[g] == out["pcMax"][g])[0])
        if not np.isnan(dcpa[g]).all():
            out["dcpaMin"][g] = np.nanmin(dcpa[g])
            out["dcpaArg"][g] = int(np.flatnonzero(dcpa[g] == out["dcpaMin"][g])[0])
    return out


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
TURN_RATE = 0.05                      # rad/s: 40 degrees take 14 s, three steps of 5 s
DEG40 = 40.0 * np.pi / 180.0
# stand on; 40 degrees to port at once; 40 degrees to starboard after 5 s; half speed; a delay beyond any horizon here
CANDIDATES = np.array([[0.0, 1.0, 0.0], [DEG40, 1.0, 0.0], [-DEG40, 1.0, 5.0], [0.0, 0.5, 0.0], [DEG40, 0.7, 1000.0]])
OWN_COV = np.array([9.0, 2.0, 16.0])


def make_scene(model, n, seed, own_cov=True):
    """encounter_ref.make_batch with its special entries (a NaN in x, a NaN in P, identical states, P = 0, ...) as the tracks, and an
    own ship at 6.7 m/s that, standing on, meets the TWINS after 20 s: (x, P, own [4], Sown [3]).  own_cov=False: Sown = 0, so that the
    tracks with P = 0 have a Sigma_0 that is not positive definite."""
    x, P = ref.make_batch(model, n, seed)
    v0 = np.array([6.0, 3.0])
    p0 = x[ref.TWINS[0], :2] + 20.0 * x[ref.TWINS[0], 2:4] - 20.0 * v0
    if x.shape[1] == 6:
        p0 = p0 + 200.0 * x[ref.TWINS[0], 4:6]
    return x, P, np.concatenate([p0, v0]), (OWN_COV.copy() if own_cov else np.zeros(3))
