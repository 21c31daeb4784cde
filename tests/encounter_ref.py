"""NumPy restatement of what `mht_encounters` computes (include/mht_amd.h, csrc/mht_encounter.h): the propagation of n entries over K
steps of a linear model, and per pair (i, j), i < j, the closest point of approach of the piecewise-linear path of the position
difference (tcpa, dcpa), the smallest Mahalanobis distance (md2) and the largest probability over the steps of being within a radius R
(pc, at time tpc), pc_k by THE RULE of the header: closed-form eigen-decomposition of Sigma_k, a clip at 8 sigma along the narrow axis
(beyond it an exact 0), a 64-node Gauss-Legendre rule in theta of exp and erfc.

Twice: in float64 (the yardstick; every sum in the order the header writes it, so that only exp, erfc, sin, cos and asin differ from
a host build of the header), and as the truth -- np.longdouble for the propagation, tcpa, dcpa and md2, and mpmath at 30 digits with the
same 64 nodes for the rule of pc.  The nodes are computed here (Newton on the Legendre polynomial, 40 digits), not copied from the
header.  `pc_exact_isotropic` is an independent exact pc for Sigma = s^2 I through scipy.stats.ncx2.

A result is a dict of [first, n] arrays: tcpa, dcpa, md2, pc, tpc, NaN where j <= i; `pck` ([K + 1, first, n], the pc_k behind pc) is
kept for the test of tpc, which is an arg max."""
import mpmath as mp
import numpy as np

from smooth_trace_ref import ratios, same_nan  # noqa: F401  (the criterion's helpers, re-exported for the tests)

NAMES = ("tcpa", "dcpa", "md2", "pc", "tpc")
CLIP = 8
_rule = {}


def gauss_legendre(n=64):
    """The positive nodes, ascending, and their weights of the n-node Gauss-Legendre rule (n even), as mpmath numbers good to 38 digits"""
    if n not in _rule:
        with mp.workdps(40):
            xs, ws = [], []
            for i in range(1, n // 2 + 1):
                x = mp.cos(mp.pi * (i - mp.mpf(1) / 4) / (n + mp.mpf(1) / 2))
                for _ in range(100):
                    p0, p1 = mp.mpf(1), x
                    for k in range(2, n + 1):
                        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
                    dp = n * (x * p1 - p0) / (x * x - 1)
                    dx = p1 / dp
                    x -= dx
                    if abs(dx) < mp.mpf(10) ** -38:
                        break
                xs.append(x)
                ws.append(2 / ((1 - x * x) * dp * dp))
            _rule[n] = sorted(zip(xs, ws))
    return [p[0] for p in _rule[n]], [p[1] for p in _rule[n]]


# ---- propagation -------------------------------------------------------------------------------------------------------------------
def propagate(x, P, Phi, Q, K, dtype=np.float64):
    """x [n, N], P [n, N, N] (the upper triangle is read), Phi, Q [N, N] (of Q the upper triangle): pos [K + 1, n, 2], S [K + 1, n, 3]
    in `dtype`.  An entry with a NaN in x or in the upper triangle of P is NaN throughout."""
    x, P = np.asarray(x).astype(dtype), np.asarray(P).astype(dtype)
    Phi, Q = np.asarray(Phi, dtype=np.float64).astype(dtype), np.asarray(Q, dtype=np.float64).astype(dtype)
    n, N = x.shape
    iu = np.triu_indices(N)
    bad = np.isnan(x).any(axis=1) | np.isnan(P[:, iu[0], iu[1]]).any(axis=1)
    xk = [x[:, i].copy() for i in range(N)]
    Pf = [[P[:, min(i, j), max(i, j)].copy() for j in range(N)] for i in range(N)]
    pos, S = np.zeros((K + 1, n, 2), dtype=dtype), np.zeros((K + 1, n, 3), dtype=dtype)
    with np.errstate(all="ignore"):
        for k in range(K + 1):
            if k > 0:
                xn = []
                for i in range(N):
                    acc = Phi[i, 0] * xk[0]
                    for l in range(1, N):
                        acc = acc + Phi[i, l] * xk[l]
                    xn.append(acc)
                xk = xn
                T = [[None] * N for _ in range(N)]
                for i in range(N):
                    for j in range(N):
                        acc = Phi[i, 0] * Pf[0][j]
                        for l in range(1, N):
                            acc = acc + Phi[i, l] * Pf[l][j]
                        T[i][j] = acc
                new = [[None] * N for _ in range(N)]
                for i in range(N):
                    for j in range(i, N):
                        acc = T[i][0] * Phi[j, 0]
                        for l in range(1, N):
                            acc = acc + T[i][l] * Phi[j, l]
                        new[i][j] = new[j][i] = acc + Q[i, j]
                Pf = new
            pos[k, :, 0], pos[k, :, 1] = xk[0], xk[1]
            S[k, :, 0], S[k, :, 1], S[k, :, 2] = Pf[0][0], Pf[0][1], Pf[1][1]
    pos[:, bad], S[:, bad] = np.nan, np.nan
    return pos, S


# ---- the rule of pc_k --------------------------------------------------------------------------------------------------------------
def pc_rule(dx, dy, a, b, c, R):
    """float64, any common shape: the header's encounter_pc, operation by operation.  Sigma = [[a, b], [b, c]] positive definite."""
    from scipy.special import erfc
    dx, dy, a, b, c, R = [np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(dx, dy, a, b, c, R)]
    xs, ws = gauss_legendre(64)
    xs, ws = [float(v) for v in xs], [float(v) for v in ws]
    inv_sqrt2, inv_sqrt_2pi = 0.70710678118654752440, 0.39894228040143267794
    with np.errstate(all="ignore"):
        det = a * c - b * b
        h, g = 0.5 * (a + c), 0.5 * (a - c)
        r = np.sqrt(g * g + b * b)
        l2 = h + r
        l1 = det / l2
        ux, uy = np.where(g >= 0.0, g + r, b), np.where(g >= 0.0, b, r - g)
        nrm = np.sqrt(ux * ux + uy * uy)
        ok = nrm > 0.0
        ux, uy = np.where(ok, ux / nrm, 1.0), np.where(ok, uy / nrm, 0.0)
        m2, m1 = -np.abs(dx * ux + dy * uy), np.abs(dy * ux - dx * uy)
        s1, s2 = np.sqrt(l1), np.sqrt(l2)
        lo, hi = np.fmax(-R, m1 - 8.0 * s1), np.fmin(R, m1 + 8.0 * s1)
        live = hi > lo
        tl, th = np.arcsin(lo / R), np.arcsin(hi / R)
        mid, half = 0.5 * (th + tl), 0.5 * (th - tl)

        def f(theta):
            sn, cs = np.sin(theta), np.cos(theta)
            z = (R * sn - m1) / s1
            e = np.exp(-0.5 * z * z)
            rc = R * cs
            u1, u2 = (-rc - m2) / s2, (rc - m2) / s2
            br = 0.5 * (erfc(u1 * inv_sqrt2) - erfc(u2 * inv_sqrt2))
            return e / s1 * br * rc

        total = np.zeros(dx.shape)
        for q in range(32):
            t = half * xs[q]
            total = total + ws[q] * (f(mid - t) + f(mid + t))
        return np.where(live, half * total * inv_sqrt_2pi, 0.0)


def _mpf(v):
    """A np.longdouble (or float) as an mpmath number, exactly"""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))


def _longdouble(v):
    hi = float(v)
    return np.longdouble(hi) + np.longdouble(float(v - mp.mpf(hi)))


def pc_rule_mp(dx, dy, a, b, c, R, nodes=64, clip=CLIP, dps=30):
    """One case of the rule in mpmath at `dps` digits (inputs: mpmath numbers, Sigma positive definite): an mpmath number, mpf(0) where
    the rule says 0 exactly.  nodes and clip are the rule's (64 and 8); 400 and 12 give the converged figure."""
    xs, ws = gauss_legendre(nodes)
    with mp.workdps(dps):
        det = a * c - b * b
        h, g = (a + c) / 2, (a - c) / 2
        r = mp.sqrt(g * g + b * b)
        l2 = h + r
        l1 = det / l2
        ux, uy = (g + r, b) if g >= 0 else (b, r - g)
        nrm = mp.sqrt(ux * ux + uy * uy)
        ux, uy = (ux / nrm, uy / nrm) if nrm > 0 else (mp.mpf(1), mp.mpf(0))
        m2, m1 = -abs(dx * ux + dy * uy), abs(dy * ux - dx * uy)
        s1, s2 = mp.sqrt(l1), mp.sqrt(l2)
        lo, hi = max(-R, m1 - clip * s1), min(R, m1 + clip * s1)
        if not hi > lo:
            return mp.mpf(0)
        tl, th = mp.asin(lo / R), mp.asin(hi / R)
        mid, half = (th + tl) / 2, (th - tl) / 2
        rt2 = mp.sqrt(2)

        def f(theta):
            sn, cs = mp.sin(theta), mp.cos(theta)
            z = (R * sn - m1) / s1
            rc = R * cs
            return mp.exp(-z * z / 2) / s1 * (mp.erfc((-rc - m2) / s2 / rt2) - mp.erfc((rc - m2) / s2 / rt2)) / 2 * rc

        total = mp.mpf(0)
        for x, w in zip(xs, ws):
            t = half * x
            total += w * (f(mid - t) + f(mid + t))
        return half * total / mp.sqrt(2 * mp.pi)


def pc_exact_isotropic(dist, s, R):
    """The exact mass of N(d, s^2 I), |d| = dist, inside the disc of radius R: a non-central chi-square with 2 degrees of freedom"""
    from scipy.stats import ncx2
    dist, s, R = [np.asarray(v, dtype=np.float64) for v in (dist, s, R)]
    return ncx2.cdf((R / s) ** 2, 2, (dist / s) ** 2)


def isotropic_grid(n=800, seed=11):
    """The fixed-seed cases the rule is held to the exact pc on: R log-uniform over 1 .. 1000, s / R over 10^-2.5 .. 10^1.5, the offset
    uniform over 0 .. R + 6 s in a random direction: (dx, dy, s, R)"""
    rng = np.random.default_rng(seed)
    R = 10.0 ** rng.uniform(0, 3, n)
    s = R * 10.0 ** rng.uniform(-2.5, 1.5, n)
    dist = rng.uniform(0, 1, n) * (R + 6 * s)
    phi = rng.uniform(0, 2 * np.pi, n)
    return dist * np.cos(phi), dist * np.sin(phi), s, R


# ---- pairs -------------------------------------------------------------------------------------------------------------------------
def encounters(x, P, Phi, Q, K, dt, R, first=None, truth=False, pc_mp=True):
    """The seam's figures over the [first, n] table: float64, or with truth=True np.longdouble with pc from mpmath (pc_mp=False, for
    tables too large for mpmath: pc, tpc and pck are then the float64 rule's on the longdouble d_k and Sigma_k, rounded)."""
    dtype = np.longdouble if truth else np.float64
    n = len(x)
    first = n if first is None else first
    pos, S = propagate(x, P, Phi, Q, K, dtype)
    dt_, R_ = dtype(dt), dtype(R)
    d = pos[:, :first, None, :] - pos[:, None, :, :]      # [K + 1, first, n, 2]
    Sg = S[:, :first, None, :] + S[:, None, :, :]
    dx, dy, a, b, c = d[..., 0], d[..., 1], Sg[..., 0], Sg[..., 1], Sg[..., 2]
    shape = (first, n)
    there = ~(np.isnan(dx) | np.isnan(dy)).any(axis=0)
    upper = np.arange(n)[None, :] > np.arange(first)[:, None]
    with np.errstate(all="ignore"):
        best, tcpa = np.full(shape, np.inf, dtype=dtype), np.zeros(shape, dtype=dtype)
        for k in range(1, K + 1):
            px, py = dx[k - 1], dy[k - 1]
            ex, ey = dx[k] - px, dy[k] - py
            ee = ex * ex + ey * ey
            sp = np.where(ee > 0, np.fmin(np.fmax(-(px * ex + py * ey) / ee, 0), 1), 0).astype(dtype)
            cx, cy = px + sp * ex, py + sp * ey
            dist2 = cx * cx + cy * cy
            better = dist2 < best
            best = np.where(better, dist2, best)
            tcpa = np.where(better, (dtype(1) * (k - 1) + sp) * dt_, tcpa)
        det = a * c - b * b
        pd_k = (a > 0) & (det > 0)
        pd = pd_k.all(axis=0)
        q = (c * dx * dx - 2.0 * b * dx * dy + a * dy * dy) / det
        md2 = np.min(np.where(pd_k, q, np.inf), axis=0)
        run = pd & there & upper
        pck = np.zeros((K + 1,) + shape, dtype=dtype)
        if truth and pc_mp:
            for i, j in zip(*np.nonzero(run)):
                for k in range(K + 1):
                    v = pc_rule_mp(*[_mpf(u[k, i, j]) for u in (dx, dy, a, b, c)], _mpf(R_))
                    pck[k, i, j] = _longdouble(v)
        else:
            sel = np.broadcast_to(run, pck.shape)
            pck[sel] = pc_rule(*[u[sel].astype(np.float64) for u in (dx, dy, a, b, c)], R)
        pc, tpc = np.full(shape, -1.0, dtype=dtype), np.zeros(shape, dtype=dtype)
        for k in range(K + 1):
            better = pck[k] > pc
            pc = np.where(better, pck[k], pc)
            tpc = np.where(better, dtype(k) * dt_, tpc)
    out = dict(tcpa=tcpa, dcpa=np.sqrt(best), md2=md2, pc=pc, tpc=tpc)
    for name in ("md2", "pc", "tpc"):
        out[name] = np.where(pd, out[name], np.nan)
    for name in NAMES:
        out[name] = np.where(there & upper, out[name], np.nan).astype(dtype)
    out["pck"] = np.where(run, pck, np.nan)
    return out


def seam_dict(out):
    """The seam's out [5, first, n] as the dict above (without pck)"""
    out = np.asarray(out)
    return {name: out[f].copy() for f, name in enumerate(NAMES)}


def pack(x, P):
    """x [n, N], P [n, N, N] in the seam's layouts: x [N, n], P [N (N + 1) / 2, n], contiguous"""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    iu = np.triu_indices(x.shape[1])
    return np.ascontiguousarray(x.T), np.ascontiguousarray(P[:, iu[0], iu[1]].T)


def model_matrices(model, dt):
    """Phi(dt) and Q(dt) as the model module returns them (float32), in float64"""
    N = int(np.asarray(model.C_RADAR).shape[1])
    widen = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64).reshape(N, N)
    return widen(model.Phi(dt)), widen(model.Q(dt))


# ---- the batch ---------------------------------------------------------------------------------------------------------------------
NAN_X, NAN_P = 5, 9                  # entries with a NaN in x (last component) and in P (an entry off the position block)
TWINS = (12, 13)                     # identical states: d = 0 at every step
ZERO_P = (20, 21)                    # P = 0 both: Sigma_0 is not positive definite
STATIONARY = (30, 31)                # no velocity, no acceleration: every segment has length zero
BEYOND = (40, 41)                    # closing at 2 m/s from 1400 m: the CPA lies beyond any horizon below 700 s
AT_ZERO = (50, 51)                   # opening: the CPA is at t = 0
SPECIAL_ENTRIES = (NAN_X, NAN_P) + TWINS + ZERO_P + STATIONARY + BEYOND + AT_ZERO


def make_batch(model, n, seed, spread=1000.0):
    """n >= 52 seeded entries (x [n, N], P [n, N, N]) of a model module: positions uniform over +-spread metres, speeds 0 .. 15 m/s
    on any heading (a six-state entry: accelerations within 0.02 m/s^2), P the model's P0 with the x and the y axis scaled by
    0.1 .. 30 each and the plane turned by a random angle (so that Sigma has an off-diagonal), and the special entries above."""
    rng = np.random.default_rng(seed)
    P0 = np.asarray(model.P0, dtype=np.float64)
    N = P0.shape[0]
    x = np.zeros((n, N))
    x[:, :2] = rng.uniform(-spread, spread, (n, 2))
    speed, head = rng.uniform(0, 15, n), rng.uniform(0, 2 * np.pi, n)
    x[:, 2], x[:, 3] = speed * np.cos(head), speed * np.sin(head)
    if N == 6:
        x[:, 4:] = rng.uniform(-0.02, 0.02, (n, 2))
    P = np.zeros((n, N, N))
    for t in range(n):
        sx, sy = np.sqrt(rng.uniform(0.1, 30, 2))
        D = np.diag(np.tile([sx, sy], N // 2))
        phi = rng.uniform(0, 2 * np.pi)
        G = np.kron(np.eye(N // 2), np.array([[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]]))
        M = G @ D @ P0 @ D @ G.T
        P[t] = 0.5 * (M + M.T)
    x[NAN_X, N - 1] = np.nan
    P[NAN_P, 1, 2] = P[NAN_P, 2, 1] = np.nan
    x[TWINS[1]] = x[TWINS[0]]
    P[ZERO_P[0]] = P[ZERO_P[1]] = 0.0
    x[STATIONARY[0], 2:] = x[STATIONARY[1], 2:] = 0.0
    x[BEYOND[0]], x[BEYOND[1]] = 0.0, 0.0
    x[BEYOND[0], :4], x[BEYOND[1], :4] = [-700.0, 300.0, 1.0, 0.0], [700.0, 300.0, -1.0, 0.0]
    x[AT_ZERO[0]], x[AT_ZERO[1]] = 0.0, 0.0
    x[AT_ZERO[0], :4], x[AT_ZERO[1], :4] = [100.0, 100.0, -3.0, -3.0], [200.0, 200.0, 3.0, 3.0]
    return x, P


def check_special_cells(got, K, dt):
    """What the special pairs of make_batch must look like in any evaluation of all pairs"""
    for e in (NAN_X, NAN_P):
        for name in NAMES:
            assert np.isnan(got[name][e, e + 1:]).all() and np.isnan(got[name][:e, e]).all(), (name, e)
    i, j = TWINS
    assert got["dcpa"][i, j] == 0 and got["tcpa"][i, j] == 0 and got["md2"][i, j] == 0 and got["pc"][i, j] > 0 and got["tpc"][i, j] >= 0
    i, j = ZERO_P
    assert np.isnan(got["pc"][i, j]) and np.isnan(got["md2"][i, j]) and np.isnan(got["tpc"][i, j])
    assert np.isfinite(got["dcpa"][i, j]) and np.isfinite(got["tcpa"][i, j])
    i, j = STATIONARY
    assert got["tcpa"][i, j] == 0 and got["dcpa"][i, j] > 0
    i, j = BEYOND
    assert got["tcpa"][i, j] == K * dt and abs(got["dcpa"][i, j] - (1400.0 - 2.0 * K * dt)) < 1e-6
    i, j = AT_ZERO
    assert got["tcpa"][i, j] == 0 and abs(got["dcpa"][i, j] - np.sqrt(20000.0)) < 1e-9
    lower = np.tril(np.ones(got["pc"].shape, dtype=bool))
    assert all(np.isnan(got[name][lower]).all() for name in NAMES)


def hold_tpc(got, truth, dt, factor, e_np):
    """tpc is an arg max, which no accuracy criterion can hold where two steps tie (pc_k = 1 to the last bit at several steps, or below
    the smallest float64 at all of them): it must be a multiple k dt of the step, and the TRUTH's pc_k at that k within
    factor max(e_np, eps64) (1 + pc) of the truth's maximum.  Where the truth's maximum is separated from every other step by more
    than that, this is equality with the truth's tpc.  Returns the number of cells held."""
    eps = float(np.finfo(np.float64).eps)
    pck, pc = truth["pck"], truth["pc"]
    cells = np.argwhere(~np.isnan(pc))
    for i, j in cells:
        k = got["tpc"][i, j] / dt
        assert k == np.round(k) and 0 <= k < len(pck), (i, j, got["tpc"][i, j])
        k = int(k)
        assert got["tpc"][i, j] == k * dt
        tol = factor * max(e_np, eps) * (1 + pc[i, j])
        assert pck[k, i, j] >= pc[i, j] - tol, (i, j, k, pck[:, i, j], pc[i, j])
    return len(cells)
