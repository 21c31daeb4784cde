"""NumPy restatement of what `mht_trace_tracks`, `mht_trace_tracks_ct` and `mht_trace_tracks_ais` compute (include/mht_amd.h): the forward
recursions of tests/smooth_score_ref.py, expression for expression, with the terms that module adds up kept per node.  Parametrised by
dtype like its siblings: float64 is the yardstick, np.longdouble the truth.

A trace is a dict of arrays with a row per node, the keys of pymht_amd.smoothing.trace_tracks*: v [L, 2], S [L, 2, 2], nis [L], ll [L],
observed [L] (bool), and for the AIS model vAis [L, 4], SAis [L, 4, 4], nisAis [L], llAis [L], message [L] (bool).  Rows of a node
without a plot (without a message) are NaN; node 0 is the initial state and never observed.
"""
import numpy as np

import smooth_ais_ref as ar
import smooth_ct_ref as cr
import smooth_em_ref as er
import smooth_ref as sr
import smooth_score_ref as score_ref
from smooth_ref import detected, err, inv  # noqa: F401
from smooth_score_ref import _term

RADAR = ("v", "S", "nis", "ll")
AIS = ("vAis", "SAis", "nisAis", "llAis")


def _blank(L, dtype, ais=False):
    nan = lambda *shape: np.full(shape, np.nan, dtype=dtype)
    out = dict(v=nan(L, 2), S=nan(L, 2, 2), nis=nan(L), ll=nan(L), observed=np.zeros(L, dtype=bool))
    if ais:
        out.update(vAis=nan(L, 4), SAis=nan(L, 4, 4), nisAis=nan(L), llAis=nan(L), message=np.zeros(L, dtype=bool))
    return out


def _radar(out, k, C, R, x, P, zk, dtype):
    """smooth_score_ref._radar with the node's terms into row k of `out`."""
    S = C @ P @ C.T + R
    v = zk - C @ x
    q, ln = _term(v, S, dtype)
    out["v"][k], out["S"][k], out["nis"][k], out["ll"][k], out["observed"][k] = v, S, q, ln, True
    K = P @ C.T @ inv(S)
    return x + K @ (zk - C @ x), P - K @ C @ P


def trace(A, Q, C, R, x_init, P_init, z, dtype=np.float64):
    """The linear model.  z: entry 0 ignored, entry k >= 1 a 2-vector or None / NaN."""
    A, Q, C, R = [np.asarray(m, dtype=np.float64).astype(dtype) for m in (A, Q, C, R)]
    x = np.asarray(x_init, dtype=np.float64).astype(dtype)
    P = np.asarray(P_init, dtype=np.float64).astype(dtype)
    has = detected(z)
    out = _blank(len(z), dtype)
    for k in range(1, len(z)):
        x = A @ x
        P = A @ P @ A.T + Q
        if has[k]:
            x, P = _radar(out, k, C, R, x, P, np.asarray(z[k], dtype=np.float64).astype(dtype), dtype)
    return out


def trace_ct(T, Q, C, R, x_init, P_init, z, dtype=np.float64):
    """The constant-turn model: A_k = Phi(T, w) at the filtered turn rate of the node in front."""
    Q, C, R = [np.asarray(m, dtype=np.float64).astype(dtype) for m in (Q, C, R)]
    x = np.asarray(x_init, dtype=np.float64).astype(dtype)
    P = np.asarray(P_init, dtype=np.float64).astype(dtype)
    has = detected(z)
    out = _blank(len(z), dtype)
    for k in range(1, len(z)):
        A = cr.phi(T, x[4], dtype)
        x = A @ x
        P = A @ P @ A.T + Q
        if has[k]:
            x, P = _radar(out, k, C, R, x, P, np.asarray(z[k], dtype=np.float64).astype(dtype), dtype)
    return out


def trace_ais(model, period, x_init, P_init, z, ais, dtype=np.float64):
    """The AIS-aware model (smooth_score_ref.score_ais's recursion)."""
    cast = lambda m: np.asarray(m, dtype=np.float64).astype(dtype)
    A, Q, C, R = [cast(m) for m in sr.model_matrices(model, period)]
    x, P = cast(x_init), cast(P_init)
    has = detected(z)
    eye = np.eye(4, dtype=dtype)
    out = _blank(len(z), dtype, ais=True)
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
            v = cast(m) - xp
            q, ln = _term(v, S, dtype)
            out["vAis"][k], out["SAis"][k], out["nisAis"][k], out["llAis"][k], out["message"][k] = v, S, q, ln, True
            K = Pp @ inv(S)
            x = xp + K @ (cast(m) - xp)
            P = Pp - K @ Pp
            xp = A2 @ x
            P = A2 @ P @ A2.T + Q2
            x = xp
        if has[k]:
            x, P = _radar(out, k, C, R, x, P, cast(z[k]), dtype)
    return out


def resum(tr):
    """A trace added up in node order, llAis in front of ll at a node with both: the dict smooth_score_ref.score* gives, in the
    trace's dtype.  A Python loop, so that the order of the additions is the score walk's."""
    zero = tr["ll"].dtype.type(0)
    out = dict(ll=zero, nis=zero, nobs=0, nis_ais=zero, nais=0)
    for k in range(len(tr["ll"])):
        if "message" in tr and tr["message"][k]:
            out["ll"], out["nis_ais"], out["nais"] = out["ll"] + tr["llAis"][k], out["nis_ais"] + tr["nisAis"][k], out["nais"] + 1
        if tr["observed"][k]:
            out["ll"], out["nis"], out["nobs"] = out["ll"] + tr["ll"][k], out["nis"] + tr["nis"][k], out["nobs"] + 1
    return out


AIS_MAX_NODES = 60


def ais_batch():
    """smooth_ais_ref.accuracy_batch with every track cut to at most 60 nodes: (model, tracks)."""
    model, tracks = ar.accuracy_batch()
    return model, [(x0, P0, z[:AIS_MAX_NODES], ais[:AIS_MAX_NODES]) for x0, P0, z, ais in tracks]


_cache = {}


def reference(kind, model, period):
    """(tracks, truth, f64) of the accuracy batch of `kind` ("linear", "ct", "ais"), evaluated once and shared: per track the trace in
    np.longdouble and in float64.  Callers leave them unchanged."""
    key = (kind, model.__name__, period)
    if key not in _cache:
        if kind == "linear":
            tracks = er.accuracy_batch(model, period)[0]
            A, C = model.Phi(period), model.C_RADAR
            def run(t, dtype):
                Q, R, P = er.start_values(model, period, t[1], "model")
                return trace(A, Q, C, R, t[0], P, t[2], dtype=dtype)
        elif kind == "ct":
            tracks = score_ref.ct_batch(model, period)[0]
            mats = cr.model_matrices(model, period)
            run = lambda t, dtype: trace_ct(*mats, *t, dtype=dtype)
        else:
            model, tracks = ais_batch()
            run = lambda t, dtype: trace_ais(model, period, *t, dtype=dtype)
        _cache[key] = (tracks, [run(t, np.longdouble) for t in tracks], [run(t, np.float64) for t in tracks])
    return _cache[key]


def _family_err(got, truth, name):
    """max |got - truth| / (1 + |truth|) over the cells of a family that are not NaN in the truth, over a batch."""
    e = 0.0
    for g, t in zip(got, truth):
        there = ~np.isnan(t[name])
        if there.any():
            e = max(e, err(np.asarray(g[name])[there], t[name][there]))
    return e


def ratios(got, truth, f64, names=RADAR):
    """Per output family: (e_dev, e_np, e_dev / max(e_np, eps64)) over a batch of traces."""
    eps = float(np.finfo(np.float64).eps)
    out = {}
    for name in names:
        e_dev, e_np = _family_err(got, truth, name), _family_err(f64, truth, name)
        out[name] = (e_dev, e_np, e_dev / max(e_np, eps))
    return out


def same_nan(got, truth, names=RADAR):
    """The NaN cells of `got` are exactly the truth's, the flags are the truth's, shapes included."""
    for g, t in zip(got, truth):
        for name in names:
            a, b = np.asarray(g[name]), t[name]
            if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
                return False
        for flag in ("observed", "message"):
            if flag in t and not (flag in g and np.array_equal(np.asarray(g[flag], dtype=bool), t[flag])):
                return False
    return True


def simulate(model, period, n_tracks, length, seed, p_detect=0.9):
    """A batch whose filter is consistent by construction: the truth follows model's own Phi, Q, the plots its C_RADAR, R_RADAR(), and
    the initial ESTIMATE is the truth plus a draw of N(0, P0) -- what P_init = P0 claims.  List of (x_init, P_init, z), z [L, 2] float64
    with NaN rows for missed detections, row 0 NaN."""
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
            x = A @ x + w[k - 1]
            if seen[k - 1]:
                z[k] = C @ x + e[k - 1]
        tracks.append((x_init, P0, z))
    return tracks
