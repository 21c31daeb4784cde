"""NumPy restatement of what `mht_score_tracks`, `mht_score_tracks_ct`, `mht_score_tracks_ais` and the trace of
`mht_smooth_tracks_em_ll` compute (include/mht_amd.h): the forward recursions of tests/smooth_ref.py, smooth_ct_ref.py, smooth_ais_ref.py
and the EM loop of smooth_em_ref.py, expression for expression, with the sums of the score taken on the way.  Parametrised by dtype like
those modules: float64 is the yardstick, np.longdouble the truth.

Node 0 is the initial state and is not an observation.  For every node k >= 1 with a radar plot, v = z_k - C xp_k, S = C Pp_k C' + R:
  nis += v' S^-1 v;  ll -= 1/2 (ln det S + v' S^-1 v + 2 ln 2 pi);  nobs += 1
and for a node with an AIS message, at the message's time, v = m - xp, S = Pp + r I4:
  nis_ais += v' S^-1 v;  ll -= 1/2 (ln det S + v' S^-1 v + 4 ln 2 pi);  nais += 1
ln det S comes from a hand-written Cholesky factor and S^-1 from smooth_ref.inv, so nothing falls back to float64 LAPACK.
"""
import numpy as np

import smooth_ais_ref as ar
import smooth_ct_ref as cr
import smooth_em_ref as er
import smooth_ref as sr
from smooth_ref import detected, err, inv  # noqa: F401


def logdet(S):
    """ln det of the symmetric positive definite S through S = U' U, in S's dtype."""
    n = S.shape[0]
    U = np.zeros_like(S)
    for i in range(n):
        d = S[i, i] - U[:i, i] @ U[:i, i]
        U[i, i] = np.sqrt(d)
        for j in range(i + 1, n):
            U[i, j] = (S[i, j] - U[:i, i] @ U[:i, j]) / U[i, i]
    return 2 * np.sum(np.log(np.diag(U)))


def _term(v, S, dtype):
    """(v' S^-1 v, ln N(v; 0, S)) in `dtype`."""
    ln2pi = np.log(dtype(8) * np.arctan(dtype(1)))
    q = v @ inv(S) @ v
    return q, -(logdet(S) + q + dtype(len(v)) * ln2pi) / dtype(2)


def _empty(dtype):
    return dict(ll=dtype(0), nis=dtype(0), nobs=0, nis_ais=dtype(0), nais=0)


def _radar(out, C, R, x, P, zk, dtype):
    """The radar update of smooth_ref.rts with the node's terms added to `out`."""
    S = C @ P @ C.T + R
    q, ln = _term(zk - C @ x, S, dtype)
    out["nis"], out["ll"], out["nobs"] = out["nis"] + q, out["ll"] + ln, out["nobs"] + 1
    K = P @ C.T @ inv(S)
    return x + K @ (zk - C @ x), P - K @ C @ P


def _score(A, Q, C, R, x, P, zz, has, dtype):
    """The linear score of arrays that are in `dtype` already (zz[k] a 2-vector in `dtype` where has[k])."""
    out = _empty(dtype)
    for k in range(1, len(zz)):
        x = A @ x
        P = A @ P @ A.T + Q
        if has[k]:
            x, P = _radar(out, C, R, x, P, zz[k], dtype)
    return out


def score(A, Q, C, R, x_init, P_init, z, dtype=np.float64):
    """The linear model (smooth_ref.rts's forward pass).  z: entry 0 ignored, entry k >= 1 a 2-vector or None / NaN."""
    A, Q, C, R = [np.asarray(m, dtype=np.float64).astype(dtype) for m in (A, Q, C, R)]
    x = np.asarray(x_init, dtype=np.float64).astype(dtype)
    P = np.asarray(P_init, dtype=np.float64).astype(dtype)
    has = detected(z)
    zz = [None if not has[k] else np.asarray(z[k], dtype=np.float64).astype(dtype) for k in range(len(z))]
    return _score(A, Q, C, R, x, P, zz, has, dtype)


def score_ct(T, Q, C, R, x_init, P_init, z, dtype=np.float64):
    """The constant-turn model (smooth_ct_ref.rts_ct's forward pass): A_k = Phi(T, w) at the filtered turn rate of the node in front."""
    Q, C, R = [np.asarray(m, dtype=np.float64).astype(dtype) for m in (Q, C, R)]
    x = np.asarray(x_init, dtype=np.float64).astype(dtype)
    P = np.asarray(P_init, dtype=np.float64).astype(dtype)
    has = detected(z)
    out = _empty(dtype)
    for k in range(1, len(z)):
        A = cr.phi(T, x[4], dtype)
        x = A @ x
        P = A @ P @ A.T + Q
        if has[k]:
            x, P = _radar(out, C, R, x, P, np.asarray(z[k], dtype=np.float64).astype(dtype), dtype)
    return out


def score_ais(model, period, x_init, P_init, z, ais, dtype=np.float64):
    """The AIS-aware model (smooth_ais_ref.rts_ais's forward pass)."""
    cast = lambda m: np.asarray(m, dtype=np.float64).astype(dtype)
    A, Q, C, R = [cast(m) for m in sr.model_matrices(model, period)]
    x, P = cast(x_init), cast(P_init)
    has = detected(z)
    eye = np.eye(4, dtype=dtype)
    out = _empty(dtype)
    for k in range(1, len(z)):
        if ais[k] is None:
            x = A @ x
            P = A @ P @ A.T + Q
        else:
            dT1, dT2, m, high = ais[k]
            A1, Q1, A2, Q2 = cast(model.Phi(dT1)), cast(model.Q(dT1)), cast(model.Phi(dT2)), cast(model.Q(dT2))
            xp = A1 @ x
            Pp = A1 @ P @ A1.T + Q1
            S = Pp + dtype(ar.SIGMA2[bool(high)]) * eye
            q, ln = _term(cast(m) - xp, S, dtype)
            out["nis_ais"], out["ll"], out["nais"] = out["nis_ais"] + q, out["ll"] + ln, out["nais"] + 1
            K = Pp @ inv(S)
            x = xp + K @ (cast(m) - xp)
            P = Pp - K @ Pp
            xp = A2 @ x
            P = A2 @ P @ A2.T + Q2
            x = xp
        if has[k]:
            x, P = _radar(out, C, R, x, P, cast(z[k]), dtype)
    return out


def em_trace(A, Q, C, R, x_init, P_init, z, n_iter, dtype=np.float64):
    """smooth_em_ref.em's loop with the log-likelihood under every theta_i recorded: ll [n_iter + 1] in `dtype`; theta_0 the arguments,
    theta_{n_iter} what the output walk runs under.  A track of one node learns nothing: equal rows."""
    A, Q, C, R = [np.asarray(m, dtype=np.float64).astype(dtype) for m in (A, Q, C, R)]
    x0 = np.asarray(x_init, dtype=np.float64).astype(dtype)
    P0 = np.asarray(P_init, dtype=np.float64).astype(dtype)
    L, n = len(z), x0.shape[0]
    has = detected(z)
    has[0] = False
    zz = [None if not has[k] else np.asarray(z[k], dtype=np.float64).astype(dtype) for k in range(L)]
    trace = [_score(A, Q, C, R, x0, P0, zz, has, dtype)["ll"]]
    for _ in range(n_iter):
        if L > 1:
            xs, Ps, G = er.e_step(A, Q, C, R, x0, P0, zz, has)
            SQ = np.zeros((n, n), dtype=dtype)
            for k in range(L - 1):
                e = xs[k + 1] - A @ xs[k]
                X = Ps[k + 1] @ G[k].T
                SQ = SQ + (np.outer(e, e) + A @ Ps[k] @ A.T + Ps[k + 1] - X @ A.T - A @ X.T)
            Q = SQ / dtype(L - 1)
            n_obs = int(has.sum())
            if n_obs > 0:
                SR = np.zeros((2, 2), dtype=dtype)
                for k in range(1, L):
                    if has[k]:
                        r = zz[k] - C @ xs[k]
                        SR = SR + (np.outer(r, r) + C @ Ps[k] @ C.T)
                R = SR / dtype(n_obs)
            x0, P0 = xs[0], Ps[0]
        trace.append(_score(A, Q, C, R, x0, P0, zz, has, dtype)["ll"])
    return np.array(trace, dtype=dtype)


def linear_batch(model, period):
    """smooth_em_ref.accuracy_batch: (tracks, one-node index, never-detected index, always-detected index)."""
    return er.accuracy_batch(model, period)


def ct_batch(model, period):
    """A smooth_ct_ref.make_batch of the lengths and detection probabilities of smooth_em_ref.accuracy_batch (same three special tracks)."""
    lengths = [2, 3, 4, 5, 6, 8] + [int(v) for v in np.random.default_rng(3).integers(8, 61, 24)] + [1, 6, 20]
    p_detect = [0.8] * 30 + [0.8, 0.0, 1.0]
    return cr.make_batch(model, period, lengths, seed=17, p_detect=p_detect), 30, 31, 32


_cache = {}


def reference(kind, model, period, start="model"):
    """(tracks, truth, f64) of the accuracy batch of `kind` ("linear", "ct", "ais"), evaluated once and shared: per track the dict of the
    score in np.longdouble and in float64.  Callers leave them unchanged.  start: the linear batch under smooth_em_ref.start_values."""
    key = (kind, model.__name__, period, start)
    if key not in _cache:
        if kind == "linear":
            tracks = linear_batch(model, period)[0]
            A, C = model.Phi(period), model.C_RADAR
            def run(t, dtype):
                Q, R, P = er.start_values(model, period, t[1], start)
                return score(A, Q, C, R, t[0], P, t[2], dtype=dtype)
        elif kind == "ct":
            tracks = ct_batch(model, period)[0]
            mats = cr.model_matrices(model, period)
            run = lambda t, dtype: score_ct(*mats, *t, dtype=dtype)
        else:
            model, tracks = ar.accuracy_batch()
            run = lambda t, dtype: score_ais(model, period, *t, dtype=dtype)
        _cache[key] = (tracks, [run(t, np.longdouble) for t in tracks], [run(t, np.float64) for t in tracks])
    return _cache[key]


def trace_reference(model, period, start, n_iter=5):
    """(tracks, truth, f64) of smooth_em_ref.accuracy_batch under `start`: per track ll [n_iter + 1], once per key and shared."""
    key = ("trace", model.__name__, period, start, n_iter)
    if key not in _cache:
        tracks = er.accuracy_batch(model, period)[0]
        A, C = model.Phi(period), model.C_RADAR
        runs = []
        for dtype in (np.longdouble, np.float64):
            out = []
            for x0, P0, z in tracks:
                Q, R, P = er.start_values(model, period, P0, start)
                out.append(em_trace(A, Q, C, R, x0, P, z, n_iter, dtype=dtype))
            runs.append(out)
        _cache[key] = (tracks, runs[0], runs[1])
    return _cache[key]


def ratios(got, truth, f64, names=("ll", "nis")):
    """Per name: (e_dev, e_np, e_dev / max(e_np, eps64)) over a batch of per-track dicts; e = max |got - truth| / (1 + |truth|)."""
    eps = float(np.finfo(np.float64).eps)
    out = {}
    for name in names:
        e_dev = max(err(g[name], t[name]) for g, t in zip(got, truth))
        e_np = max(err(f[name], t[name]) for f, t in zip(f64, truth))
        out[name] = (e_dev, e_np, e_dev / max(e_np, eps))
    return out


def trace_ratios(got, truth, f64):
    """Per row i of the trace: (e_dev, e_np, ratio) over a batch of per-track ll [n_iter + 1]."""
    eps = float(np.finfo(np.float64).eps)
    out = []
    for i in range(len(truth[0])):
        e_dev = max(err(g[i], t[i]) for g, t in zip(got, truth))
        e_np = max(err(f[i], t[i]) for f, t in zip(f64, truth))
        out.append((e_dev, e_np, e_dev / max(e_np, eps)))
    return out
