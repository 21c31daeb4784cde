"""NumPy restatement of what `mht_imm_smooth_tracks` and `mht_imm_smooth_tracks_ct` compute (include/mht_amd.h): the fixed-interval IMM
smoother -- the filter of tests/imm_ref.py walked forward with every mode's own state kept, then the mode-matched RTS pass of
csrc/mht_imm_smooth.h walked backward -- over the expressions of imm_ref, filter_ref and smooth_ref, so that with one mode the states
are smooth_ref.rts' (smooth_ct_ref.rts_ct's) bit for bit.  Parametrised by dtype like them: float64 is the yardstick, np.longdouble the
truth.  The recursion restates Nadarajah, Tharmarasa, McDonald and Kirubarajan (2012) for modes that share the state space.

Backward, last node: xs_j = xf_j, Ps_j = Pf_j, mus = mu, (xs, Ps) the filter's combined state.  Node k = L - 2 .. 0, sums over i ascending:
  back-mix  d_j = sum_i Pi[j, i] mus_i(k+1);  d_j > 0: b_i = Pi[j, i] mus_i(k+1) / d_j, (x0_j, P0_j) the moments of the smoothed states of
            node k + 1 under b;  d_j == 0: mode j's own
  terms     A_j = A or Phi(T, xf_j(k)[4]), xp_j = A_j xf_j(k), M_j = A_j Pf_j(k) A_j';  lam_ji = -1/2 |L^-1 (xs_i(k+1) - xp_j)|^2 - sum ln L_ee
            with L L' = M_j + Q_i;  m_j = max lam_ji over Pi[j, i] > 0;  lnL_j = m_j + ln sum_{i: Pi[j, i] > 0} Pi[j, i] exp(lam_ji - m_j)
  step      Pp = M_j + Q_j, G = Pf_j A_j' Pp^-1, xs_j(k) = xf_j + G (x0_j - xp_j), Ps_j(k) = Pf_j + G (P0_j - Pp) G'
  weigh     top = max lnL_j over mu_j(k) > 0, u_j = mu_j(k) exp(lnL_j - top) (0 where mu_j(k) == 0), mus_j(k) = u_j / sum_j u_j
  combine   the moments of the (xs_j(k), Ps_j(k)) under mus(k)

A result is a dict mus [L, r], muf [L, r], xs [L, n], Ps [L, n, n], ll (0-d array), nobs (int).
"""
import numpy as np

import filter_ref as fr
import imm_ref as ir
import smooth_ct_ref as cr
import smooth_ref as sr
import smooth_score_ref as scr
from smooth_trace_ref import ratios, same_nan  # noqa: F401  (the criterion's helpers, re-exported for the tests)

NAMES = ("mus", "muf", "xs", "Ps", "ll")


def _chol(M, dtype):
    """Lower Cholesky factor in M's dtype (np.linalg has none for np.longdouble)"""
    n = M.shape[0]
    L = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        for j in range(i + 1):
            s = M[i, j]
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    return L


def _lam(v, M, dtype):
    """-1/2 |L^-1 v|^2 - sum ln L_ee, L L' = M"""
    L = _chol(M, dtype)
    n = len(v)
    y = np.zeros(n, dtype=dtype)
    for e in range(n):
        s = v[e]
        for c in range(e):
            s = s - L[e, c] * y[c]
        y[e] = s / L[e, e]
    ld = np.log(L[0, 0])
    for e in range(1, n):
        ld = ld + np.log(L[e, e])
    return -(y @ y) / dtype(2) - ld


def forward(transition, C, Qs, Rs, Pi, mu0, x_init, P_init, z, dtype=np.float64):
    """imm_ref.imm, statement for statement, keeping per node every mode's own (xf_j, Pf_j) and mu: (xf [L][r], Pf [L][r], mu [L], ll, nobs)"""
    cast = lambda m: np.asarray(m, dtype=np.float64).astype(dtype)
    ct = np.ndim(transition) == 0
    A = None if ct else cast(transition)
    C, Pi, mu = cast(C), cast(Pi), cast(mu0)
    Qs, Rs = [cast(q) for q in Qs], [cast(q) for q in Rs]
    r = len(Qs)
    has = sr.detected(z)
    xs, Ps = [cast(x_init) for _ in range(r)], [cast(P_init) for _ in range(r)]
    keep_x, keep_P, keep_mu = [list(xs)], [list(Ps)], [mu.copy()]
    ll, nobs, poison = dtype(0), 0, False
    for k in range(1, len(z)):
        cbar, x0, P0 = [], [], []
        for j in range(r):
            c = Pi[0, j] * mu[0]
            for i in range(1, r):
                c = c + Pi[i, j] * mu[i]
            cbar.append(c)
            if c > 0:
                xm, Pm = ir._moments([Pi[i, j] * mu[i] / c for i in range(r)], xs, Ps, dtype)
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
                    with np.errstate(invalid="ignore"):
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
        keep_x.append(list(xs))
        keep_P.append(list(Ps))
        keep_mu.append(mu.copy())
    return keep_x, keep_P, keep_mu, ll, nobs


def imm_smooth(transition, C, Qs, Rs, Pi, mu0, x_init, P_init, z, dtype=np.float64):
    """transition: a matrix A (the linear model) or a float T (the constant-turn model's period).  Qs [r, n, n], Rs [r, 2, 2]."""
    cast = lambda m: np.asarray(m, dtype=np.float64).astype(dtype)
    xf, Pf, muf, ll, nobs = forward(transition, C, Qs, Rs, Pi, mu0, x_init, P_init, z, dtype)
    ct = np.ndim(transition) == 0
    A = None if ct else cast(transition)
    Pi = cast(Pi)
    Qs = [cast(q) for q in Qs]
    r, L, n = len(Qs), len(z), len(xf[0][0])
    xs, Ps, mus = list(xf[-1]), list(Pf[-1]), muf[-1].copy()
    out_mu, out_x, out_P = [None] * L, [None] * L, [None] * L
    out_mu[-1] = mus.copy()
    out_x[-1], out_P[-1] = (xs[0], Ps[0]) if L == 1 else ir._moments(mus, xs, Ps, dtype)
    for k in range(L - 2, -1, -1):
        new_x, new_P, lnL = [], [], []
        for j in range(r):
            d = Pi[j, 0] * mus[0]
            for i in range(1, r):
                d = d + Pi[j, i] * mus[i]
            if d > 0:
                x0, P0 = ir._moments([Pi[j, i] * mus[i] / d for i in range(r)], xs, Ps, dtype)
            else:
                x0, P0 = xs[j], Ps[j]
            Aj = cr.phi(transition, xf[k][j][4], dtype) if ct else A
            xp = Aj @ xf[k][j]
            M = Aj @ Pf[k][j] @ Aj.T
            with np.errstate(invalid="ignore", divide="ignore"):
                lam = [_lam(xs[i] - xp, M + Qs[i], dtype) for i in range(r)]
                m = max(lam[i] for i in range(r) if Pi[j, i] > 0)
                s = dtype(0)
                for i in range(r):
                    if Pi[j, i] > 0:
                        s = s + Pi[j, i] * np.exp(lam[i] - m)
                lnL.append(m + np.log(s))
            Pp = M + Qs[j]
            G = Pf[k][j] @ Aj.T @ sr.inv(Pp)
            new_x.append(xf[k][j] + G @ (x0 - xp))
            new_P.append(Pf[k][j] + G @ (P0 - Pp) @ G.T)
        with np.errstate(invalid="ignore"):
            top = max(lnL[j] for j in range(r) if muf[k][j] > 0)
            u = [muf[k][j] * np.exp(lnL[j] - top) if muf[k][j] > 0 else dtype(0) for j in range(r)]
        s = u[0]
        for j in range(1, r):
            s = s + u[j]
        mus = np.array([u[j] / s for j in range(r)], dtype=dtype)
        xs, Ps = new_x, new_P
        out_mu[k] = mus.copy()
        out_x[k], out_P[k] = ir._moments(mus, xs, Ps, dtype)
    return dict(mus=np.array(out_mu, dtype=dtype).reshape(L, r), muf=np.array(muf, dtype=dtype).reshape(L, r),
                xs=np.array(out_x, dtype=dtype).reshape(L, n), Ps=np.array(out_P, dtype=dtype).reshape(L, n, n),
                ll=np.asarray(ll, dtype=dtype), nobs=nobs)


def run(kind, model, period, track, key, dtype=np.float64):
    return imm_smooth(*ir.transition_and_C(kind, model, period), *ir.setup(model, period, key), *track, dtype=dtype)


_cache = {}


def reference(kind, model, period, n, seed, key):
    """(tracks, truth, f64) of filter_ref.edge_batch(kind, ..) under imm_ref.SETUPS[key], evaluated once and shared: per track the
    smoother in np.longdouble and in float64.  Callers leave them unchanged."""
    at = (kind, model.__name__, period, n, seed, key)
    if at not in _cache:
        tracks = fr.edge_batch(kind, model, period, n, seed)
        _cache[at] = (tracks, [run(kind, model, period, t, key, np.longdouble) for t in tracks], [run(kind, model, period, t, key, np.float64) for t in tracks])
    return _cache[at]


def manoeuvre_batch_with_truth(model, period, n_tracks=40, length=60, seed=5, loud=(20, 40), factor=64.0, p_detect=0.9):
    """imm_ref.manoeuvre_batch's recipe, draw for draw, keeping the true states: (tracks, truth [n_tracks][length, n]); truth[.][0] is the
    state the initial estimate was drawn around."""
    rng = np.random.default_rng(seed)
    A, Q, C, R = [np.asarray(m, dtype=np.float64) for m in sr.model_matrices(model, period)]
    P0 = np.asarray(model.P0, dtype=np.float64)
    n = A.shape[0]
    tracks, truth = [], []
    for _ in range(n_tracks):
        x = np.zeros(n)
        x[:2] = rng.uniform(-15000, 15000, 2)
        x[2:4] = rng.uniform(-12, 12, 2)
        x_init = x + rng.multivariate_normal(np.zeros(n), P0)
        z = np.full((length, 2), np.nan)
        w = rng.multivariate_normal(np.zeros(n), Q, size=length - 1)
        e = rng.multivariate_normal(np.zeros(2), R, size=length - 1)
        seen = rng.random(length - 1) < p_detect
        states = [x.copy()]
        for k in range(1, length):
            x = A @ x + (np.sqrt(factor) if loud[0] <= k < loud[1] else 1.0) * w[k - 1]
            if seen[k - 1]:
                z[k] = C @ x + e[k - 1]
            states.append(x.copy())
        tracks.append((x_init, P0, z))
        truth.append(np.array(states))
    return tracks, truth
