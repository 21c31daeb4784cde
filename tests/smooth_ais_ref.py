"""NumPy restatement of the AIS-aware fixed-interval Rauch-Tung-Striebel smoother `mht_smooth_tracks_ais` computes (include/mht_amd.h),
parametrised by dtype like tests/smooth_ref.py, whose `inv` (hand-written Gauss-Jordan: nothing falls back to a float64 LAPACK call
behind a longdouble array) and `err` it uses.

One track: nodes k = 0 .. L-1; node 0 is (x_init, P_init); node k >= 1 carries a radar plot z[k] or None / NaN, and ais[k] = None or
(dT1, dT2, state [4], highAccuracy).  Every node is a sequence of prediction steps (A, Q) with updates between and behind them:
  without a message  one step with A = Phi(T), Q = Q(T); then the radar update if there is a plot -- tests/smooth_ref.py's node,
                     expression for expression (no AIS node at all: the same bits)
  with a message     step 1 with Phi(dT1), Q(dT1); the AIS update S = P + r I, K = P S^-1, x += K (m - x), P -= K P with r = 1 (high
                     accuracy) or 9; step 2 with Phi(dT2), Q(dT2); then the radar update if there is a plot
  backward           one Rauch-Tung-Striebel step per prediction step, last first: G = Pf A' Pp^-1, xs = xf + G (xs+ - xp),
                     Ps = Pf + G (Ps+ - Pp) G', (xf, Pf) the filtered state the step predicted from -- for step 2 the state behind
                     the AIS update.  The smoothed state at the message's time is an intermediate.
Phi(dT) and Q(dT) are taken as the model returns them (float32: the matrices the forest filters with), widened."""
import numpy as np

import smooth_ref as sr

SIGMA2 = {True: 1.0, False: 9.0}      # models/ais.py: sigma 1 for a high-accuracy message, 3 otherwise


def kinds(z, ais):
    """Per node 0 plain / 1 plain + radar / 2 AIS legs / 3 AIS legs + radar (node 0: 0)."""
    has = sr.detected(z)
    k = np.array([(2 if a is not None else 0) + int(h) for a, h in zip(ais, has)], dtype=np.uint8)
    k[0] = 0
    return k


def rts_ais(model, period, x_init, P_init, z, ais, dtype=np.float64):
    """Returns dict(xs [L, 4], Ps [L, 4, 4], xf, Pf) in `dtype`; xf, Pf are the filtered states at the scan times."""
    cast = lambda m: np.asarray(m, dtype=np.float64).astype(dtype)
    A, Q, C, R = [cast(m) for m in sr.model_matrices(model, period)]
    x0, P0 = cast(x_init), cast(P_init)
    L, n = len(z), x0.shape[0]
    assert len(ais) == L and n == 4
    has = sr.detected(z)
    eye = np.eye(n, dtype=dtype)
    xf, Pf, steps = [x0], [P0], [None]      # steps[k]: [(A, xf, Pf, xp, Pp)] of the prediction steps that lead to node k
    for k in range(1, L):
        x, P, st = xf[-1], Pf[-1], []
        if ais[k] is None:
            xp = A @ x
            Pp = A @ P @ A.T + Q
            st.append((A, x, P, xp, Pp))
            x, P = xp, Pp
        else:
            dT1, dT2, m, high = ais[k]
            A1, Q1, A2, Q2 = cast(model.Phi(dT1)), cast(model.Q(dT1)), cast(model.Phi(dT2)), cast(model.Q(dT2))
            xp = A1 @ x
            Pp = A1 @ P @ A1.T + Q1
            st.append((A1, x, P, xp, Pp))
            S = Pp + dtype(SIGMA2[bool(high)]) * eye
            K = Pp @ sr.inv(S)
            x = xp + K @ (cast(m) - xp)
            P = Pp - K @ Pp
            xp = A2 @ x
            Pp = A2 @ P @ A2.T + Q2
            st.append((A2, x, P, xp, Pp))
            x, P = xp, Pp
        if has[k]:
            zk = cast(z[k])
            S = C @ P @ C.T + R
            K = P @ C.T @ sr.inv(S)
            x = x + K @ (zk - C @ x)
            P = P - K @ C @ P
        steps.append(st)
        xf.append(x)
        Pf.append(P)
    xs, Ps = [None] * L, [None] * L
    xs[-1], Ps[-1] = xf[-1], Pf[-1]
    for k in range(L - 2, -1, -1):
        x, P = xs[k + 1], Ps[k + 1]
        for A_, xf_, Pf_, xp_, Pp_ in reversed(steps[k + 1]):
            G = Pf_ @ A_.T @ sr.inv(Pp_)
            x = xf_ + G @ (x - xp_)
            P = Pf_ + G @ (P - Pp_) @ G.T
        xs[k], Ps[k] = x, P
    return dict(xs=np.array(xs, dtype=dtype).reshape(L, n), Ps=np.array(Ps, dtype=dtype).reshape(L, n, n),
                xf=np.array(xf, dtype=dtype).reshape(L, n), Pf=np.array(Pf, dtype=dtype).reshape(L, n, n))


def make_batch(model, period, lengths, seed, p_detect=0.8, p_ais=0.3, offsets=(0.25, 0.5, 0.75)):
    """Seeded tracks for the four-state `model`: list of (x_init, P_init, z, ais) along a simulated truth.  z [L, 2] float64 holding
    float32 values, NaN rows for missed detections, row 0 NaN.  ais: list of L entries, None or (dT1, dT2, state [4] float64 holding
    float32 values, highAccuracy): with probability p_ais a node has a message, made at one of `offsets` (a share of the period) behind
    the node in front, the truth there plus noise of the accuracy class it claims, either class equally likely.  Radar detections and
    messages are drawn independently, so both "message only" and "message, then plot" occur.  p_detect and p_ais may be one number or
    one per track."""
    rng = np.random.default_rng(seed)
    A, Q, C, R = [np.asarray(m, dtype=np.float64) for m in sr.model_matrices(model, period)]
    n = A.shape[0]
    pds = np.broadcast_to(np.asarray(p_detect, dtype=np.float64), (len(lengths),))
    pas = np.broadcast_to(np.asarray(p_ais, dtype=np.float64), (len(lengths),))
    legs = {}
    for off in offsets:
        dT1 = float(off) * float(period)
        dT2 = float(period) - dT1
        legs[off] = (dT1, dT2) + tuple(np.asarray(m, dtype=np.float64) for m in (model.Phi(dT1), model.Q(dT1), model.Phi(dT2), model.Q(dT2)))
    tracks = []
    for L, pdet, pais in zip(lengths, pds, pas):
        x = np.zeros(n)
        x[:2] = rng.uniform(-15000, 15000, 2)
        x[2:4] = rng.uniform(-12, 12, 2)
        x_init = x.copy()
        z = np.full((L, 2), np.nan)
        ais = [None] * L
        for k in range(1, L):
            if rng.random() < pais:
                dT1, dT2, A1, Q1, A2, Q2 = legs[offsets[int(rng.integers(0, len(offsets)))]]
                x = A1 @ x + rng.multivariate_normal(np.zeros(n), Q1)
                high = bool(rng.random() < 0.5)
                msg = (x + rng.normal(0.0, np.sqrt(SIGMA2[high]), n)).astype(np.float32).astype(np.float64)
                ais[k] = (dT1, dT2, msg, high)
                x = A2 @ x + rng.multivariate_normal(np.zeros(n), Q2)
            else:
                x = A @ x + rng.multivariate_normal(np.zeros(n), Q)
            if rng.random() < pdet:
                z[k] = (C @ x + rng.normal(0.0, np.sqrt(R[0, 0]), 2)).astype(np.float32)
        tracks.append((x_init, np.asarray(model.P0, dtype=np.float64), z, ais))
    return tracks


ACCURACY_PERIOD = 2.5


def accuracy_batch():
    """The batch both accuracy tests run (tests/test_smooth_ais_cpu.py on the host build of the arithmetic, tests/test_smooth_ais_gpu.py
    on the device): models/pv, T = 2.5, 40 tracks of 2 .. 400 nodes, 80 % detections, 30 % of the nodes with a message."""
    from pymht_amd.models import pv
    rng = np.random.default_rng(20241)
    lengths = [int(v) for v in rng.integers(2, 401, 40)]
    return pv, make_batch(pv, ACCURACY_PERIOD, lengths, seed=29, p_detect=0.8, p_ais=0.3)


def references(model, period, tracks):
    """(longdouble truth, float64 evaluation) per track."""
    truth = [rts_ais(model, period, *t, dtype=np.longdouble) for t in tracks]
    f64 = [rts_ais(model, period, *t, dtype=np.float64) for t in tracks]
    return truth, f64
