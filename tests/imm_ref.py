"""NumPy restatement of what `mht_imm_tracks` and `mht_imm_tracks_ct` compute (include/mht_amd.h): the interacting-multiple-model filter
over the forward recursions of tests/filter_ref.py -- their advance and radar update expression for expression, so that with one mode
the states are filter_ref's bit for bit -- parametrised by dtype like them: float64 is the yardstick, np.longdouble the truth.

Inputs: the model's A (or T for Phi(T, w)) and C; r modes (Q_j, R_j); a row-stochastic Pi [r, r], Pi[i, j] = P(mode j at k | mode i at
k - 1); mu0 [r].  Node 0: every mode holds (x_init, P_init), mu = mu0, the combined state is (x_init, P_init).  Node k >= 1, sums over i
ascending:
  cbar_j = sum_i Pi[i, j] mu_i;  cbar_j > 0: w_ij = Pi[i, j] mu_i / cbar_j, x0_j = sum_i w_ij x_i,
  P0_j = sum_i w_ij (P_i + (x_i - x0_j)(x_i - x0_j)');  cbar_j == 0: mode j keeps its own (x_j, P_j)
  mode j advances (x0_j, P0_j) under Q_j (constant turn: Phi at x0_j[4]);  with a plot it updates under R_j, lam_j = ln N(z; C xp_j, S_j),
  m = max_j lam_j, u_j = cbar_j exp(lam_j - m), s = sum_j u_j, mu_j = u_j / s, ll += m + ln s, nobs += 1;  without one mu_j = cbar_j
  x = sum_j mu_j x_j,  P = sum_j mu_j (P_j + (x_j - x)(x_j - x)')
A det S that is not positive in some mode makes the track's ll NaN.

A result is a dict mu [L, r], x [L, n], P [L, n, n], ll (0-d array), nobs (int).
"""
import numpy as np

import filter_ref as fr
import smooth_ct_ref as cr
import smooth_ref as sr
import smooth_score_ref as scr
from smooth_trace_ref import ratios, same_nan  # noqa: F401  (the criterion's helpers, re-exported for the tests)

NAMES = ("mu", "x", "P", "ll")


def _moments(w, xs, Ps, dtype):
    """sum_i w_i x_i and sum_i w_i (P_i + (x_i - x)(x_i - x)'), i ascending"""
    x = w[0] * xs[0]
    for i in range(1, len(w)):
        x = x + w[i] * xs[i]
    P = None
    for i in range(len(w)):
        d = xs[i] - x
        term = w[i] * (Ps[i] + np.outer(d, d))
        P = term if P is None else P + term
    return x, P


def imm(transition, C, Qs, Rs, Pi, mu0, x_init, P_init, z, dtype=np.float64):
    """transition: a matrix A (the linear model) or a float T (the constant-turn model's period).  Qs [r, n, n], Rs [r, 2, 2]."""
    cast = lambda m: np.asarray(m, dtype=np.float64).astype(dtype)
    ct = np.ndim(transition) == 0
    A = None if ct else cast(transition)
    C, Pi, mu = cast(C), cast(Pi), cast(mu0)
    Qs, Rs = [cast(q) for q in Qs], [cast(q) for q in Rs]
    r = len(Qs)
    has = sr.detected(z)
    xs, Ps = [cast(x_init) for _ in range(r)], [cast(P_init) for _ in range(r)]
    out_mu, out_x, out_P = [mu.copy()], [cast(x_init)], [cast(P_init)]
    ll, nobs, poison = dtype(0), 0, False
    for k in range(1, len(z)):
        cbar, x0, P0 = [], [], []
        for j in range(r):
            c = Pi[0, j] * mu[0]
            for i in range(1, r):
                c = c + Pi[i, j] * mu[i]
            cbar.append(c)
            if c > 0:
                xm, Pm = _moments([Pi[i, j] * mu[i] / c for i in range(r)], xs, Ps, dtype)
            else:
                xm, Pm = xs[j], Ps[j]
            x0.append(xm)
            P0.append(Pm)
        lam = []
        for j in range(r):
            Aj = cr.phi(transition, x0[j][4], dtype) if ct else A
            x = Aj @ x0[j]
            P = Aj @ P0[j] @ Aj.T + Qs[j]
            if has[k]:
                zk = cast(z[k])
                S = C @ P @ C.T + Rs[j]
                if S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1] > 0:
                    with np.errstate(invalid="ignore"):      # (an indefinite S with a positive determinant: NaN, which is what it is)
                        lam.append(scr._term(zk - C @ x, S, dtype)[1])
                else:
                    lam.append(dtype(np.nan))
                x, P = fr._radar(C, Rs[j], x, P, zk)
            xs[j], Ps[j] = x, P
        if has[k]:
            poison = poison or bool(np.isnan(np.array(lam, dtype=dtype)).any())
            m = max(lam) if not poison else dtype(np.nan)
            u = [cbar[j] * np.exp(lam[j] - m) for j in range(r)]
            s = u[0]
            for j in range(1, r):
                s = s + u[j]
            mu = np.array([u[j] / s for j in range(r)], dtype=dtype)
            ll = ll + (m + np.log(s))
            nobs += 1
        else:
            mu = np.array(cbar, dtype=dtype)
        x, P = _moments(mu, xs, Ps, dtype)
        out_mu.append(mu.copy())
        out_x.append(x)
        out_P.append(P)
    L, n = len(z), len(out_x[0])
    return dict(mu=np.array(out_mu, dtype=dtype).reshape(L, r), x=np.array(out_x, dtype=dtype).reshape(L, n),
                P=np.array(out_P, dtype=dtype).reshape(L, n, n), ll=np.asarray(ll, dtype=dtype), nobs=nobs)


def transition_and_C(kind, model, period):
    """(A or T, C) of a batch of `kind` ("linear", "ct")"""
    return (float(period) if kind == "ct" else model.Phi(period)), model.C_RADAR


def modes(model, period, q_scales, r_scales=None):
    """(Qs [r, n, n], Rs [r, 2, 2]) float64: the model's float32 matrices times float64 scales, as smoothing.noise_grid makes candidates"""
    n = int(np.asarray(model.C_RADAR).shape[1])
    Q32 = np.asarray(model.Q(float(period)), dtype=np.float32).astype(np.float64).reshape(n, n)
    R32 = np.asarray(model.R_RADAR(), dtype=np.float32).astype(np.float64).reshape(2, 2)
    r_scales = [1.0] * len(q_scales) if r_scales is None else r_scales
    return np.array([float(s) * Q32 for s in q_scales]), np.array([float(s) * R32 for s in r_scales])


def sticky(r, stay=0.95):
    return np.array([[1.0]]) if r == 1 else np.full((r, r), (1.0 - stay) / (r - 1)) + np.eye(r) * (stay - (1.0 - stay) / (r - 1))


# r -> (qScales, rScales, Pi, mu0) the accuracy tests run: the three-mode chain has zeros (its outer modes do not reach each other), the
# four-mode one scales R too; "blocked": two modes the second of which is never entered (cbar_1 == 0 from node 1 on: it keeps its own)
SETUPS = {
    1: ((1.0,), (1.0,), np.array([[1.0]]), np.array([1.0])),
    2: ((1.0, 16.0), (1.0, 1.0), sticky(2), np.array([0.5, 0.5])),
    3: ((0.25, 1.0, 16.0), (1.0, 1.0, 1.0), np.array([[0.9, 0.1, 0.0], [0.05, 0.9, 0.05], [0.0, 0.1, 0.9]]), np.array([0.5, 0.3, 0.2])),
    4: ((0.25, 1.0, 4.0, 16.0), (1.0, 2.0, 0.5, 1.0), sticky(4, 0.91), np.array([0.4, 0.3, 0.2, 0.1])),
    "blocked": ((1.0, 16.0), (1.0, 1.0), np.array([[1.0, 0.0], [1.0, 0.0]]), np.array([0.5, 0.5])),
}


def setup(model, period, key):
    """(Qs, Rs, Pi, mu0) of SETUPS[key] for `model`"""
    q, r, Pi, mu0 = SETUPS[key]
    return modes(model, period, q, r) + (Pi, mu0)


def run(kind, model, period, track, key, dtype=np.float64):
    return imm(*transition_and_C(kind, model, period), *setup(model, period, key), *track, dtype=dtype)


_cache = {}


def reference(kind, model, period, n, seed, key):
    """(tracks, truth, f64) of filter_ref.edge_batch(kind, ..) under SETUPS[key], evaluated once and shared: per track the filter in
    np.longdouble and in float64.  Callers leave them unchanged."""
    at = (kind, model.__name__, period, n, seed, key)
    if at not in _cache:
        tracks = fr.edge_batch(kind, model, period, n, seed)
        _cache[at] = (tracks, [run(kind, model, period, t, key, np.longdouble) for t in tracks], [run(kind, model, period, t, key, np.float64) for t in tracks])
    return _cache[at]


def manoeuvre_batch(model, period, n_tracks=40, length=60, seed=5, loud=(20, 40), factor=64.0, p_detect=0.9):
    """Tracks that steam straight, manoeuvre and steam on: smooth_trace_ref.simulate with the process noise `factor` Q on the nodes
    loud[0] <= k < loud[1] and Q elsewhere.  List of (x_init, P_init, z)."""
    rng = np.random.default_rng(seed)
    A, Q, C, R = [np.asarray(m, dtype=np.float64) for m in sr.model_matrices(model, period)]
    P0 = np.asarray(model.P0, dtype=np.float64)
    n = A.shape[0]
    tracks = []
    for _ in range(n_tracks):
        x = np.zeros(n)
        x[:2] = rng.uniform(-15000, 15000, 2)
        x[2:4] = rng.uniform(-12, 12, 2)
        x_init = x + rng.multivariate_normal(np.zeros(n), P0)
        z = np.full((length, 2), np.nan)
        w = rng.multivariate_normal(np.zeros(n), Q, size=length - 1)
        e = rng.multivariate_normal(np.zeros(2), R, size=length - 1)
        seen = rng.random(length - 1) < p_detect
        for k in range(1, length):
            x = A @ x + (np.sqrt(factor) if loud[0] <= k < loud[1] else 1.0) * w[k - 1]
            if seen[k - 1]:
                z[k] = C @ x + e[k - 1]
        tracks.append((x_init, P0, z))
    return tracks
