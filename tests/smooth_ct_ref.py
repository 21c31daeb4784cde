"""NumPy restatement of the constant-turn Rauch-Tung-Striebel smoother `mht_smooth_tracks_ct` computes (include/mht_amd.h), parametrised by
dtype like smooth_ref.rts: float64 is the yardstick of what the number format can do, np.longdouble the truth both are measured against.

The model is pymht_amd/models/ct.py, state [x, y, vx, vy, w, a].  The recursion is smooth_ref's with a transition per step,
  A_k = Phi(T, w) at the FILTERED turn rate w = xf_k[4] of the node predicted from, no Jacobian with respect to w (the forest's own filter),
built in `dtype` from np.sin / np.cos of the dtype's own values (longdouble trigonometry for the truth), with models/ct.Phi's straight-line
limits for |w| < 1e-9 and NOT rounded to float32 (models/ct.Phi returns float32; see pymht_amd/csrc/mht_smooth_ct_math.h for why the
smoother does not).  Inverses are smooth_ref.inv."""
import numpy as np

from smooth_ref import detected, err, inv      # noqa: F401  (err is re-exported for the tests)


def phi(T, w, dtype):
    """Phi(T, w) in `dtype`; T and w are taken as they are in that dtype."""
    T, w = dtype(T), dtype(w)
    s, c = np.sin(w * T), np.cos(w * T)
    if abs(w) < 1e-9:
        sw, cw = T, dtype(0)
    else:
        sw, cw = s / w, (dtype(1) - c) / w
    a = np.identity(6, dtype=dtype)
    a[0, 2], a[0, 3] = sw, -cw
    a[1, 2], a[1, 3] = cw, sw
    a[2, 2], a[2, 3] = c, -s
    a[3, 2], a[3, 3] = s, c
    a[4, 5] = T
    return a


def model_matrices(model, period):
    """(T, Q, C, R): what the seam reads of a constant-turn model."""
    return float(period), model.Q(period), model.C_RADAR, model.R_RADAR()


def rts_ct(T, Q, C, R, x_init, P_init, z, dtype=np.float64):
    """z as in smooth_ref.rts.  Returns dict(xs [L, 6], Ps [L, 6, 6], xf, Pf, w [L]: the filtered turn rate A_k was built from) in `dtype`."""
    Q, C, R = [np.asarray(m, dtype=np.float64).astype(dtype) for m in (Q, C, R)]
    x0 = np.asarray(x_init, dtype=np.float64).astype(dtype)
    P0 = np.asarray(P_init, dtype=np.float64).astype(dtype)
    L, n = len(z), 6
    has = detected(z)
    xf, Pf, xp, Pp, As = [x0], [P0], [None], [None], []
    for k in range(1, L):
        A = phi(T, xf[-1][4], dtype)
        As.append(A)
        x = A @ xf[-1]
        P = A @ Pf[-1] @ A.T + Q
        xp.append(x)
        Pp.append(P)
        if has[k]:
            zk = np.asarray(z[k], dtype=np.float64).astype(dtype)
            S = C @ P @ C.T + R
            K = P @ C.T @ inv(S)
            x = x + K @ (zk - C @ x)
            P = P - K @ C @ P
        xf.append(x)
        Pf.append(P)
    xs, Ps = [None] * L, [None] * L
    xs[-1], Ps[-1] = xf[-1], Pf[-1]
    for k in range(L - 2, -1, -1):
        G = Pf[k] @ As[k].T @ inv(Pp[k + 1])
        xs[k] = xf[k] + G @ (xs[k + 1] - xp[k + 1])
        Ps[k] = Pf[k] + G @ (Ps[k + 1] - Pp[k + 1]) @ G.T
    out = dict(xs=np.array(xs, dtype=dtype).reshape(L, n), Ps=np.array(Ps, dtype=dtype).reshape(L, n, n),
               xf=np.array(xf, dtype=dtype).reshape(L, n), Pf=np.array(Pf, dtype=dtype).reshape(L, n, n))
    out["w"] = out["xf"][:, 4]
    return out


def coupled_P0(model):
    """models/ct.P0 with a velocity / turn-rate cross-covariance (correlation 0.5 with vx, -0.5 with vy): symmetric positive definite
    (asserted).  With the diagonal P0 the no-Jacobian transition keeps the turn block uncoupled from the measured block and the filtered
    turn rate follows w_0 + k T a_0 whatever the data say; with this one every measurement moves it."""
    P = np.asarray(model.P0, dtype=np.float64).copy()
    for i, rho in ((2, 0.5), (3, -0.5)):
        P[i, 4] = P[4, i] = rho * np.sqrt(P[i, i] * P[4, 4])
    assert np.array_equal(P, P.T) and np.linalg.eigvalsh(P).min() > 0
    return P


# per track, cycling: the turn rate at node 0 -- exactly 0, inside the straight-line limit, gentle, moderate, up to the fuzz campaign's 0.6 rad/s
TURN_KINDS = ("zero", "tiny", "gentle", "moderate", "hard")


def make_batch(model, period, lengths, seed, p_detect=0.8):
    """Seeded tracks of true constant-turn motion (the unrounded Phi at the true turn rate w_0 + k T a_0, which stays within the fuzz
    campaign's range; white-noise acceleration of model.Q's size on the velocity, none on the turn rate): list of
    (x_init, P_init, z) like smooth_ref.make_batch -- z [L, 2] float64 holding float32 values, NaN rows for misses, row 0 NaN.
    Track i: turn kind TURN_KINDS[i % 5]; a non-zero turn-rate rate a_0 where i % 3 == 1 (never on the zero / tiny kinds of even i, so
    that some tracks stay exactly straight); P_init = coupled_P0 for odd i, model.P0 for even i."""
    rng = np.random.default_rng(seed)
    T = float(period)
    Q, C, R = [np.asarray(m, dtype=np.float64) for m in (model.Q(T), model.C_RADAR, model.R_RADAR())]
    q_acc = np.sqrt(Q[2, 2]) / T      # Q = G G' scaled, G = [T^2 / 2, T] per axis
    g = np.array([T * T / 2.0, T])
    pds = np.broadcast_to(np.asarray(p_detect, dtype=np.float64), (len(lengths),))
    P_diag, P_coupled = np.asarray(model.P0, dtype=np.float64), coupled_P0(model)
    tracks = []
    for i, (L, pdet) in enumerate(zip(lengths, pds)):
        kind = TURN_KINDS[i % 5]
        sign = 1.0 if rng.random() < 0.5 else -1.0
        w0 = {"zero": 0.0, "tiny": sign * rng.uniform(1e-12, 9e-10), "gentle": sign * rng.uniform(1e-4, 0.02),
              "moderate": sign * rng.uniform(0.02, 0.1), "hard": sign * rng.uniform(0.1, 0.6)}[kind]
        a0 = 0.0
        if i % 3 == 1 and not (kind in ("zero", "tiny") and i % 2 == 0):
            a0 = rng.uniform(-1.0, 1.0) * 0.2 / (T * max(L, 2))      # (the turn rate drifts by at most 0.2 rad/s over the track)
        x = np.zeros(6)
        x[:2] = rng.uniform(-15000, 15000, 2)
        x[2:4] = rng.uniform(-12, 12, 2)
        x[4], x[5] = w0, a0
        x_init = x.copy()
        z = np.full((L, 2), np.nan)
        if L > 1:
            acc = rng.normal(0.0, q_acc, (L - 1, 2))
            v = rng.normal(0.0, np.sqrt(R[0, 0]), (L - 1, 2))
            seen = rng.random(L - 1) < pdet
            for k in range(1, L):
                x = phi(T, x[4], np.float64) @ x
                x[[0, 2]] += g * acc[k - 1, 0]
                x[[1, 3]] += g * acc[k - 1, 1]
                if seen[k - 1]:
                    z[k] = (C @ x + v[k - 1]).astype(np.float32)
        tracks.append((x_init, P_coupled if i % 2 else P_diag, z))
    return tracks
