"""NumPy restatement of what `mht_filter_tracks`, `mht_filter_tracks_ct` and `mht_filter_tracks_ais` hand out (include/mht_amd.h): the
filtered state and covariance of every node, which the smoother references compute on their way forward -- the forward halves of
smooth_ref.rts, smooth_ct_ref.rts_ct and smooth_ais_ref.rts_ais, expression for expression and with their inverse and transition (their
xf and Pf bit for bit, which tests/test_filter_cpu.py asserts; the backward half is not run).  Parametrised by dtype like them: float64
is the yardstick, np.longdouble the truth.

A result is a dict xf [L, n], Pf [L, n, n] (full, symmetric up to rounding), a row per node; node 0 is (x_init, P_init).
"""
import numpy as np

import smooth_ais_ref as ar
import smooth_ct_ref as cr
import smooth_ref as sr
from smooth_trace_ref import ratios, same_nan  # noqa: F401  (the criterion's helpers, re-exported for the tests)

NAMES = ("xf", "Pf")
EDGE_LENGTHS = [1, 2, 60, 7, 33]      # cycled over a batch: the shortest tracks next to the longest in every wavefront


def _radar(C, R, x, P, zk):
    """The radar update of the smoother references, expression for expression"""
    S = C @ P @ C.T + R
    K = P @ C.T @ sr.inv(S)
    return x + K @ (zk - C @ x), P - K @ C @ P


def _out(xf, Pf, dtype):
    L, n = len(xf), xf[0].shape[0]
    return dict(xf=np.array(xf, dtype=dtype).reshape(L, n), Pf=np.array(Pf, dtype=dtype).reshape(L, n, n))


def filter_lin(A, Q, C, R, x_init, P_init, z, dtype=np.float64):
    """The linear model: smooth_ref.rts going forward.  z: entry 0 ignored, entry k >= 1 a 2-vector or None / NaN."""
    cast = lambda m: np.asarray(m, dtype=np.float64).astype(dtype)
    A, Q, C, R = [cast(m) for m in (A, Q, C, R)]
    has = sr.detected(z)
    xf, Pf = [cast(x_init)], [cast(P_init)]
    for k in range(1, len(z)):
        x = A @ xf[-1]
        P = A @ Pf[-1] @ A.T + Q
        if has[k]:
            x, P = _radar(C, R, x, P, cast(z[k]))
        xf.append(x)
        Pf.append(P)
    return _out(xf, Pf, dtype)


def filter_ct(T, Q, C, R, x_init, P_init, z, dtype=np.float64):
    """The constant-turn model: smooth_ct_ref.rts_ct going forward, A_k = Phi(T, w) at the filtered turn rate of the node in front."""
    cast = lambda m: np.asarray(m, dtype=np.float64).astype(dtype)
    Q, C, R = [cast(m) for m in (Q, C, R)]
    has = sr.detected(z)
    xf, Pf = [cast(x_init)], [cast(P_init)]
    for k in range(1, len(z)):
        A = cr.phi(T, xf[-1][4], dtype)
        x = A @ xf[-1]
        P = A @ Pf[-1] @ A.T + Q
        if has[k]:
            x, P = _radar(C, R, x, P, cast(z[k]))
        xf.append(x)
        Pf.append(P)
    return _out(xf, Pf, dtype)


def filter_ais(model, period, x_init, P_init, z, ais, dtype=np.float64):
    """The AIS-aware model: smooth_ais_ref.rts_ais going forward; the filtered states are those at the scans' times."""
    cast = lambda m: np.asarray(m, dtype=np.float64).astype(dtype)
    A, Q, C, R = [cast(m) for m in sr.model_matrices(model, period)]
    has = sr.detected(z)
    eye = np.eye(4, dtype=dtype)
    xf, Pf = [cast(x_init)], [cast(P_init)]
    for k in range(1, len(z)):
        x, P = xf[-1], Pf[-1]
        if ais[k] is None:
            x, P = A @ x, A @ P @ A.T + Q
        else:
            dT1, dT2, m, high = ais[k]
            A1, Q1, A2, Q2 = cast(model.Phi(dT1)), cast(model.Q(dT1)), cast(model.Phi(dT2)), cast(model.Q(dT2))
            xp = A1 @ x
            Pp = A1 @ P @ A1.T + Q1
            S = Pp + dtype(ar.SIGMA2[bool(high)]) * eye
            K = Pp @ sr.inv(S)
            x = xp + K @ (cast(m) - xp)
            P = Pp - K @ Pp
            x, P = A2 @ x, A2 @ P @ A2.T + Q2
        if has[k]:
            x, P = _radar(C, R, x, P, cast(z[k]))
        xf.append(x)
        Pf.append(P)
    return _out(xf, Pf, dtype)


def run(kind, model, period, track, dtype=np.float64):
    """One track of a batch of `kind` ("linear", "ct", "ais", "ais-none": AIS tracks whose messages are left out)."""
    if kind == "linear":
        return filter_lin(*sr.model_matrices(model, period), *track, dtype=dtype)
    if kind == "ct":
        return filter_ct(*cr.model_matrices(model, period), *track, dtype=dtype)
    return filter_ais(model, period, *track, dtype=dtype)


def edge_lengths(n):
    return [EDGE_LENGTHS[i % len(EDGE_LENGTHS)] for i in range(n)]


def edge_batch(kind, model, period, n, seed):
    """n tracks of lengths 1, 2, 60, 7, 33 in turn; every fourth is never detected.  "ais-none": the AIS batch without its messages."""
    make = {"linear": sr.make_batch, "ct": cr.make_batch, "ais": ar.make_batch, "ais-none": ar.make_batch}[kind]
    tracks = make(model, period, edge_lengths(n), seed=seed, p_detect=[0.0 if i % 4 == 3 else 0.8 for i in range(n)])
    if kind == "ais-none":
        tracks = [t[:3] + ([None] * len(t[2]),) for t in tracks]
    return tracks


_cache = {}


def reference(kind, model, period, n, seed):
    """(tracks, truth, f64) of edge_batch(kind, ..), evaluated once and shared: per track the filter in np.longdouble and in float64.
    Callers leave them unchanged."""
    key = (kind, model.__name__, period, n, seed)
    if key not in _cache:
        tracks = edge_batch(kind, model, period, n, seed)
        _cache[key] = (tracks, [run(kind, model, period, t, np.longdouble) for t in tracks], [run(kind, model, period, t, np.float64) for t in tracks])
    return _cache[key]


def full(Pp, n):
    """Packed upper triangles [.., n (n + 1) / 2] -> full symmetric matrices [.., n, n]."""
    iu = np.triu_indices(n)
    Pp = np.asarray(Pp)
    out = np.empty(Pp.shape[:-1] + (n, n), dtype=Pp.dtype)
    out[..., iu[0], iu[1]] = Pp
    out[..., iu[1], iu[0]] = Pp
    return out
