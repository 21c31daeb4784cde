"""NumPy restatement of what `mht_smooth_tracks_em` computes (include/mht_amd.h): expectation-maximisation over one track of the linear
smoother, then the smoother -- the reference's pykalman call (pyTarget.py:580-609: em(n_iter=5), then smooth) as an algorithm, not as
pykalman's bits.  Parametrised by dtype like tests/smooth_ref.py, whose conventions, inverse and batches it shares: float64 is the
yardstick, np.longdouble the truth.

A = Phi(T) and C stay fixed; theta = (Q, R, x0, P0).  One iteration, all four updated from the same E-step:
  E-step   the forward filter and the Rauch-Tung-Striebel backward pass of smooth_ref.rts under theta: xs_k, Ps_k, the gains
           G_k = Pf_k A' Pp_{k+1}^-1 and the lag-one covariances X_k = Ps_{k+1} G_k' = Cov(x_{k+1}, x_k | all z)
  M-step   Q <- 1/(L-1) sum_{k=0}^{L-2} [e e' + A Ps_k A' + Ps_{k+1} - X_k A' - A X_k'],  e = xs_{k+1} - A xs_k
           R <- 1/n_obs sum_{k: z_k present} [r r' + C Ps_k C'],  r = z_k - C xs_k   (n_obs == 0: R stays)
           x0 <- xs_0,  P0 <- Ps_0                                                    (L == 1: nothing is learned)
After n_iter iterations one more E-step under the learned theta gives xs and Ps; n_iter == 0 is smooth_ref.rts.
"""
import numpy as np

from smooth_ref import detected, err, inv, make_batch  # noqa: F401  (err and make_batch: for the tests that import this module)


def e_step(A, Q, C, R, x0, P0, z, has):
    """smooth_ref.rts in the dtype of its arguments, with the gains kept: xs [L], Ps [L], G [L-1] as lists."""
    L = len(z)
    xf, Pf, xp, Pp = [x0], [P0], [None], [None]
    for k in range(1, L):
        x = A @ xf[-1]
        P = A @ Pf[-1] @ A.T + Q
        xp.append(x)
        Pp.append(P)
        if has[k]:
            S = C @ P @ C.T + R
            K = P @ C.T @ inv(S)
            x = x + K @ (z[k] - C @ x)
            P = P - K @ C @ P
        xf.append(x)
        Pf.append(P)
    xs, Ps, G = [None] * L, [None] * L, [None] * (L - 1)
    xs[-1], Ps[-1] = xf[-1], Pf[-1]
    for k in range(L - 2, -1, -1):
        G[k] = Pf[k] @ A.T @ inv(Pp[k + 1])
        xs[k] = xf[k] + G[k] @ (xs[k + 1] - xp[k + 1])
        Ps[k] = Pf[k] + G[k] @ (Ps[k + 1] - Pp[k + 1]) @ G[k].T
    return xs, Ps, G


def em(A, Q, C, R, x_init, P_init, z, n_iter, dtype=np.float64):
    """z as for smooth_ref.rts (entry 0 ignored, None / NaN = missed).  Returns dict(xs [L, n], Ps [L, n, n], Q [n, n], R [2, 2]) in `dtype`."""
    A, Q, C, R = [np.asarray(m, dtype=np.float64).astype(dtype) for m in (A, Q, C, R)]
    x0 = np.asarray(x_init, dtype=np.float64).astype(dtype)
    P0 = np.asarray(P_init, dtype=np.float64).astype(dtype)
    L, n = len(z), x0.shape[0]
    has = detected(z)
    has[0] = False
    zz = [None if not has[k] else np.asarray(z[k], dtype=np.float64).astype(dtype) for k in range(L)]
    for _ in range(n_iter if L > 1 else 0):
        xs, Ps, G = e_step(A, Q, C, R, x0, P0, zz, has)
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
    xs, Ps, _ = e_step(A, Q, C, R, x0, P0, zz, has)
    return dict(xs=np.array(xs, dtype=dtype).reshape(L, n), Ps=np.array(Ps, dtype=dtype).reshape(L, n, n), Q=Q, R=R)


def start_values(model, period, P_init, start):
    """(Q, R, P0) a walk starts from: the tracker's own ("model", float32 matrices widened as the seam widens them), or identities ("reference")."""
    n = np.asarray(model.C_RADAR).shape[1]
    if start == "reference":
        return np.eye(n), np.eye(2), np.eye(n)
    widen = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64)
    return widen(model.Q(period)), widen(model.R_RADAR()), np.asarray(P_init, dtype=np.float64)


def accuracy_batch(model, period):
    """The batch of the accuracy tests (tests/test_smooth_em_cpu.py, test_smooth_em_gpu.py): short tracks, 24 of 8 .. 60 nodes detected
    with probability 0.8, then one track of one node, one never detected and one always detected.  Returns (tracks, index of the
    one-node track, of the never-detected one, of the always-detected one)."""
    lengths = [2, 3, 4, 5, 6, 8] + [int(v) for v in np.random.default_rng(3).integers(8, 61, 24)] + [1, 6, 20]
    p_detect = [0.8] * 30 + [0.8, 0.0, 1.0]
    return make_batch(model, period, lengths, seed=17, p_detect=p_detect), 30, 31, 32


_cache = {}


def accuracy_reference(model, period, start, n_iter=5):
    """(tracks, truth, f64) of accuracy_batch under `start`, evaluated once per (model, start) and shared: per track the dict of `em` in
    np.longdouble and in float64.  Callers leave them unchanged."""
    key = (model.__name__, period, start, n_iter)
    if key not in _cache:
        tracks = accuracy_batch(model, period)[0]
        A, C = model.Phi(period), model.C_RADAR
        runs = []
        for dtype in (np.longdouble, np.float64):
            out = []
            for x0, P0, z in tracks:
                Q, R, P = start_values(model, period, P0, start)
                out.append(em(A, Q, C, R, x0, P, z, n_iter, dtype=dtype))
            runs.append(out)
        _cache[key] = (tracks, runs[0], runs[1])
    return _cache[key]


def ratios(got, truth, f64):
    """Per output name: (e_dev, e_np, e_dev / max(e_np, eps64)) over a batch -- got, truth, f64: per track dicts with xs, Ps, Q, R
    (Ps None in `got` is skipped)."""
    eps = float(np.finfo(np.float64).eps)
    out = {}
    for name in ("xs", "Ps", "Q", "R"):
        if got[0][name] is None:
            continue
        e_dev = max(err(g[name], t[name]) for g, t in zip(got, truth))
        e_np = max(err(f[name], t[name]) for f, t in zip(f64, truth))
        out[name] = (e_dev, e_np, e_dev / max(e_np, eps))
    return out
