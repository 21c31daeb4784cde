"""What the tests of the grid score seams (`mht_score_tracks_grid`, `mht_score_tracks_ct_grid`) share: the grids, a stand-in model that
carries one candidate, tests/smooth_score_ref.py evaluated per candidate on that module's accuracy batches (once, cached, left unchanged
by its callers), and the synthetic batch of the truth-recovery test with its float64 surface."""
import numpy as np

import smooth_ref as sr
import smooth_score_ref as ref

POW2 = (0.25, 0.5, 1.0, 2.0, 4.0)      # exact in float32 and float64: a candidate is then a model the plain seams can be handed
ODD = (0.3, 1.7)                       # not representable: the candidate's float64 product is not a float32


def stand_in(model, Qc, Rc):
    """`model` with candidate (Qc, Rc) in place of its Q(T) and R_RADAR()."""
    class Candidate:
        __name__ = "candidate of " + model.__name__
        Phi, C_RADAR, P0 = staticmethod(model.Phi), model.C_RADAR, model.P0
        Q = staticmethod(lambda T: Qc)
        R_RADAR = staticmethod(lambda: Rc)
    if hasattr(model, "transition"):
        Candidate.transition = model.transition
    return Candidate


_cache = {}


def reference(kind, model, period, scales=ODD):
    """(tracks, Q, R, truth, f64) for smooth_score_ref's accuracy batch of `kind` ("linear", "ct") under noise_grid(scales, scales):
    truth[g][t] and f64[g][t] the reference's dicts of track t under candidate g in np.longdouble and float64."""
    from pymht_amd.smoothing import noise_grid
    key = (kind, model.__name__, period, tuple(scales))
    if key not in _cache:
        Q, R = noise_grid(model, period, scales, scales)
        if kind == "linear":
            tracks = ref.linear_batch(model, period)[0]
            run = lambda g, t, dtype: ref.score(model.Phi(period), Q[g], model.C_RADAR, R[g], *t, dtype=dtype)
        else:
            tracks = ref.ct_batch(model, period)[0]
            run = lambda g, t, dtype: ref.score_ct(float(period), Q[g], model.C_RADAR, R[g], *t, dtype=dtype)
        both = [[[run(g, t, dtype) for t in tracks] for g in range(len(Q))] for dtype in (np.longdouble, np.float64)]
        _cache[key] = (tracks, Q, R, both[0], both[1])
    return _cache[key]


def rows_as_dicts(ll, nis, nobs):
    """The seams' (ll [G, n], nis [G, n], nObs [n]) as [g][t] dicts like the reference's."""
    return [[dict(ll=ll[g, t], nis=nis[g, t], nobs=int(nobs[t]), nais=0) for t in range(ll.shape[1])] for g in range(ll.shape[0])]


def hold(label, got, truth, f64, factor=8.0):
    """The project's criterion per candidate row: e <= factor max(e_np, eps64) for ll and nis, counts exact.  Returns the largest ratios."""
    worst = {"ll": 0.0, "nis": 0.0}
    for g, (gr, tr, fr) in enumerate(zip(got, truth, f64)):
        res = ref.ratios(gr, tr, fr, ("ll", "nis"))
        print("%s, candidate %d: " % (label, g) + " | ".join("%s e %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
        for k, (e, e_np, ratio) in res.items():
            assert np.isfinite(e) and ratio <= factor, "candidate %d %s: e %.3g > %g x max(e_np %.3g, eps)" % (g, k, e, factor, e_np)
            worst[k] = max(worst[k], ratio)
        assert all(a["nobs"] == b["nobs"] for a, b in zip(gr, tr))
    return worst


# ---- recovery of the truth: tracks simulated from pv with Q_true = 4 Q and R_true = R / 4, scored over {1/4, 1, 4}^2 ---------------------
RECOVERY_SCALES = (0.25, 1.0, 4.0)
RECOVERY_TRUE = (2, 0)      # (iq, ir): qScale 4, rScale 1/4
RECOVERY_TRACKS, RECOVERY_NODES, RECOVERY_SEED = 60, 30, 11      # (1 800 nodes x 9 cells of the float64 reference: two to three seconds, the most a test should take)


def recovery_batch(model, period):
    """(tracks, surface [3, 3]): the float64 reference's pooled log-likelihood of every cell, summed over the tracks in float64."""
    from pymht_amd.smoothing import noise_grid
    key = ("recovery", model.__name__, period)
    if key not in _cache:
        true = stand_in(model, 4.0 * np.asarray(model.Q(period), dtype=np.float64), 0.25 * np.asarray(model.R_RADAR(), dtype=np.float64))
        tracks = sr.make_batch(true, period, [RECOVERY_NODES] * RECOVERY_TRACKS, seed=RECOVERY_SEED, p_detect=0.9)
        Q, R = noise_grid(model, period, RECOVERY_SCALES, RECOVERY_SCALES)
        A, Cm = model.Phi(period), model.C_RADAR
        surface = np.array([np.sum(np.array([ref.score(A, Q[g], Cm, R[g], *t)["ll"] for t in tracks], dtype=np.float64)) for g in range(9)])
        _cache[key] = (tracks, surface.reshape(3, 3))
    return _cache[key]
