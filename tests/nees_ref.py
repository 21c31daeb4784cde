"""NumPy restatement of what `mht_nees_nodes` computes per cell (include/mht_amd.h, csrc/mht_nees.h): the estimation error e = x - truth
on the leading D components, the Cholesky factor P = U' U, the forward substitution U' y = e, and the prefix sums of y_j^2 -- nees2 over
the position, nees4 over position and velocity, nees over the full state.  The leading block of U is the factor of the leading block of
P, so each prefix sum is e_d' P_dd^-1 e_d under the marginal covariance (asserted against a plain solve in tests/test_nees_cpu.py).
Parametrised by dtype like its siblings: float64 is the yardstick, np.longdouble the truth.  The factorisation is written out, so
nothing falls back to a float64 LAPACK call behind a longdouble array.

A result is a dict with a row per node, the keys of pymht_amd.evaluation.nees_nodes: error [L, N] (NaN at components >= D), nees2 [L],
nees4 [L], nees [L].  A node without truth (a NaN row of `truth`), or whose x or P holds a NaN, is NaN throughout; a figure that needs
components beyond D is NaN; a pivot j that is not positive gives NaN in every figure that includes component j.
"""
import numpy as np

import smooth_ref as sr
from smooth_trace_ref import ratios, same_nan  # noqa: F401  (the criterion's helpers, re-exported for the tests)

NAMES = ("error", "nees2", "nees4", "nees")


def nees_eval(x, P, truth, D, dtype=np.float64):
    """x [.., N], P [.., N, N] (the upper triangle is read), truth [.., >= D], any leading shape: (error [.., N], nees2 [..], nees4 [..],
    neesN [..]) in `dtype`, the cells side by side -- the loops run over the matrix entries only."""
    x, P, truth = np.asarray(x).astype(dtype), np.asarray(P).astype(dtype), np.asarray(truth).astype(dtype)
    N, shape = x.shape[-1], x.shape[:-1]
    e = np.full(shape + (N,), np.nan, dtype=dtype)
    e[..., :D] = x[..., :D] - truth[..., :D]
    U, y = np.zeros(shape + (N, N), dtype=dtype), np.zeros(shape + (N,), dtype=dtype)
    q, ok = np.zeros(shape, dtype=dtype), np.ones(shape, dtype=bool)
    figures = {}
    with np.errstate(all="ignore"):
        for j in range(N):
            for i in range(j):      # column j of U above the diagonal
                U[..., i, j] = (P[..., i, j] - np.sum(U[..., :i, i] * U[..., :i, j], axis=-1)) / U[..., i, i]
            d = P[..., j, j] - np.sum(U[..., :j, j] * U[..., :j, j], axis=-1)
            ok = ok & (d > 0) & (j < D)      # (a pivot that is not positive: NaN from here on)
            U[..., j, j] = np.sqrt(np.where(ok, d, np.nan))
            y[..., j] = (e[..., j] - np.sum(U[..., :j, j] * y[..., :j], axis=-1)) / U[..., j, j]
            q = q + y[..., j] * y[..., j]
            figures[j] = np.where(ok, q, np.nan).astype(dtype)
    return e, figures[1], figures[3], figures[N - 1]


def _blank_absent(out, there):
    for k in NAMES:
        out[k][~there] = np.nan
    return out


def nees_nodes(x, P, truth, dtype=np.float64):
    """One track: x [L, N], P [L, N, N], truth [L, D] with NaN rows where the node has none."""
    x, P, truth = np.asarray(x), np.asarray(P), np.asarray(truth)
    N, D = x.shape[1], truth.shape[1]
    iu = np.triu_indices(N)
    there = ~(np.isnan(truth).any(axis=1) | np.isnan(x).any(axis=1) | np.isnan(P[:, iu[0], iu[1]]).any(axis=1))
    e, n2, n4, nn = nees_eval(x, P, np.where(there[:, None], truth, 0.0), D, dtype)
    return _blank_absent(dict(error=e, nees2=n2, nees4=n4, nees=nn), there)


def nees_batch(x, P, truth, present, D, dtype=np.float64):
    """A batch in the seam's layouts -- x [L_max, N, n], P [L_max, N (N + 1) / 2, n] packed, truth [L_max, N, n], present [L_max, n] --
    as ONE dict of arrays over the cells: error [L_max, n, N], nees2 / nees4 / nees [L_max, n]."""
    x, Pp, truth = np.moveaxis(np.asarray(x), 1, 2), np.moveaxis(np.asarray(P), 1, 2), np.moveaxis(np.asarray(truth), 1, 2)
    N = x.shape[-1]
    iu = np.triu_indices(N)
    Pm = np.zeros(x.shape + (N,))
    Pm[..., iu[0], iu[1]] = Pp
    there = (np.asarray(present) != 0) & ~np.isnan(x).any(axis=-1) & ~np.isnan(Pp).any(axis=-1)
    e, n2, n4, nn = nees_eval(x, Pm, truth, D, dtype)
    return _blank_absent(dict(error=e, nees2=n2, nees4=n4, nees=nn), there)


def seam_dict(out, N):
    """The seam's out [L_max, N + 3, n] as nees_batch's dict"""
    out = np.asarray(out)
    return dict(error=np.moveaxis(out[:, :N], 1, 2).copy(), nees2=out[:, N].copy(), nees4=out[:, N + 1].copy(), nees=out[:, N + 2].copy())


BAD_PIVOT, ABSENT, NAN_X, NAN_P = (0, 0), (1, 1), (2, 0), (3, 2)      # (node, track) of the cells cell_batch makes special


def cell_batch(N, n, L_max, seed):
    """Seeded cells in the seam's layouts: (x [L_max, N, n], P [L_max, NS, n] packed, truth [L_max, N, n], present [L_max, n] uint8).
    P = B' B + a diagonal with entries spread over six decades (positions in the thousands of square metres, rates far below one), so
    the conditioning varies from cell to cell; the errors are draws of N(0, P) scaled by 0.5 .. 2.  A fifth of the cells are absent; the
    last two rows of every third track are NaN in x and P (a track's end, as the seams write it).  Four cells are special: BAD_PIVOT
    has P[2][2] lowered until the pivot of component 2 is -1 (components 0, 1 stay fine); ABSENT is absent; NAN_X has a NaN in
    x[N - 1] and NAN_P one in the last entry of P, both present."""
    rng = np.random.default_rng(seed)
    NS = N * (N + 1) // 2
    iu = np.triu_indices(N)
    scale = np.array([30.0, 30.0, 2.0, 2.0, 0.02, 0.005][:N])
    B = rng.normal(size=(L_max, n, N, N)) * scale * rng.uniform(0.3, 3.0, size=(L_max, n, 1, 1))
    Pm = np.swapaxes(B, -1, -2) @ B + np.eye(N) * (scale * scale * 10.0 ** rng.uniform(-3, 0, size=(L_max, n, 1)))[..., None, :]
    Pm = 0.5 * (Pm + np.swapaxes(Pm, -1, -2))
    U = np.swapaxes(np.linalg.cholesky(Pm), -1, -2)
    Pm[BAD_PIVOT][2, 2] = U[BAD_PIVOT][0, 2] ** 2 + U[BAD_PIVOT][1, 2] ** 2 - 1.0
    truth = np.zeros((L_max, n, N))
    truth[..., :2] = rng.uniform(-15000, 15000, size=(L_max, n, 2))
    truth[..., 2:4] = rng.uniform(-12, 12, size=(L_max, n, 2))
    err = np.einsum("...ji,...j->...i", U, rng.normal(size=(L_max, n, N))) * rng.uniform(0.5, 2.0, size=(L_max, n, 1))
    x = truth + err
    present = (rng.random((L_max, n)) < 0.8).astype(np.uint8)
    Pp = Pm[..., iu[0], iu[1]]
    for t in range(0, n, 3):
        x[L_max - 2:, t], Pp[L_max - 2:, t] = np.nan, np.nan
    present[BAD_PIVOT], present[ABSENT], present[NAN_X], present[NAN_P] = 1, 0, 1, 1
    x[NAN_X][N - 1] = np.nan
    Pp[NAN_P][NS - 1] = np.nan
    mv = lambda a: np.ascontiguousarray(np.moveaxis(a, 1, 2))
    return mv(x), mv(Pp), mv(truth), present


def simulate(model, period, n_tracks, length, seed, p_detect=0.9):
    """smooth_trace_ref.simulate with the true states kept: a batch whose filter is consistent by construction -- the truth follows
    the model's own Phi, Q, the plots its C_RADAR, R_RADAR(), and the initial ESTIMATE is the truth plus a draw of N(0, P0).
    Returns (tracks [(x_init, P_init, z)], states: per track [L, n] float64)."""
    rng = np.random.default_rng(seed)
    A, Q, C, R = [np.asarray(m, dtype=np.float64) for m in sr.model_matrices(model, period)]
    P0 = np.asarray(model.P0, dtype=np.float64)
    n = A.shape[0]
    tracks, states = [], []
    for _ in range(n_tracks):
        x = np.zeros(n)
        x[:2] = rng.uniform(-15000, 15000, 2)
        x[2:4] = rng.uniform(-12, 12, 2)
        x_init = x + rng.multivariate_normal(np.zeros(n), P0)
        xs = [x.copy()]
        z = np.full((length, 2), np.nan)
        w = rng.multivariate_normal(np.zeros(n), Q, size=length - 1)
        e = rng.multivariate_normal(np.zeros(2), R, size=length - 1)
        seen = rng.random(length - 1) < p_detect
        for k in range(1, length):
            x = A @ x + w[k - 1]
            xs.append(x.copy())
            if seen[k - 1]:
                z[k] = C @ x + e[k - 1]
        tracks.append((x_init, P0, z))
        states.append(np.array(xs))
    return tracks, states
