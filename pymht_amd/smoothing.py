"""Fixed-interval Rauch-Tung-Striebel smoothing of track histories on the device (`mht_smooth_tracks`, include/mht_amd.h seam (v)).

The reference smooths one track at a time with pykalman (`Target.getSmoothTrack`, pyTarget.py:580-609: five EM iterations that
re-estimate the noise covariances, then a smoother).  pykalman's EM step is not reproducible and nothing here depends on pykalman:
the smoother below runs with the tracker's OWN model -- A = Phi(T), Q = Q(T), C_RADAR, R_RADAR(), float64 -- which is a documented
difference from the reference.  The inputs are the reference's: the initial state of the chain and
`backtrackMeasurement()` with None for a missed detection.

All tracks of a call go to the device in ONE launch, one track per lane; there is no host fallback.

Constant-turn models (models/ct.py) are smoothed only on request: `smooth_tracks_ct`, or `constantTurn=True` further up.  Their transition
Phi(T, w) is taken at each node's FILTERED turn rate, without a Jacobian with respect to w -- the model the forest itself filters with --
which makes a track a linear model with a known A_k per step (`mht_smooth_tracks_ct`); `smooth_tracks` keeps refusing such a model.

AIS-aided tracks are smoothed with their AIS updates only on request as well: `smooth_tracks_ais`, or `ais=True` further up.  A node that
took a message went through two legs -- predict by dT1 to the message's time, update with the message (C = I4, R = sigma^2 I4), predict by
dT2 to the scan's time -- before its radar update (Tracker.__fuseRadarAndAis, csrc/mht_ais_math.h), and `mht_smooth_tracks_ais` walks
that model forward and back.  Without the request such a track is smoothed from its radar plots alone, as before.

The reference's EM step is available on request too: `smooth_tracks_em`, or `em=5` further up (linear models).  Per track, Q, R and the
initial state are re-estimated from the track itself by `n_iter` expectation-maximisation iterations before the smoothing walk
(`mht_smooth_tracks_em`); with emStart="reference" the covariances start at the identity, pykalman's documented default for what the
reference does not hand it, and em=5 is then the reference's procedure -- restated (tests/smooth_em_ref.py), not pykalman's bits.

The same histories are SCORED here too: `score_tracks`, `score_tracks_ct`, `score_tracks_ais` (and `score_nodes`, `Tracker.getTrackLikelihoods`)
run the forward half of the smoother of that model and return per track the log-likelihood of its plots, their normalised innovation
squared summed (NIS) and their number (`mht_score_tracks*`, one forward-only launch, nothing stored per node); node 0 is the initial state
and not an observation, so the figures are not pykalman's loglikelihood(), which counts one at time 0.  `smooth_tracks_em(likelihoods=True)`
hands out the log-likelihood under every EM iterate (`mht_smooth_tracks_em_ll`).

To TUNE the noise by those figures the histories are scored under many candidate (Q, R) at once: `score_tracks_grid`,
`score_tracks_ct_grid` (and `score_nodes_grid`, `Tracker.getLikelihoodSurface`) pack and upload a batch once and score every
(track, candidate) in one launch (`mht_score_tracks_grid`); `noise_grid` makes the candidates of a grid of scalings of the model's own
matrices, `best_cell` picks the cell of the largest likelihood -- the pooled maximum-likelihood pair over the grid.

The sums say whether a model fits a track; WHERE it stops fitting is in the sequence they add up: `trace_tracks`, `trace_tracks_ct`,
`trace_tracks_ais` (and `trace_nodes`, `Tracker.getTrackInnovations`) run the score's walk and hand out per node the innovation, its
covariance, the node's NIS and log-likelihood term (`mht_trace_tracks*`, one launch, 7 doubles per node and track, 16 more per AIS
message); `consistency` runs the filter-consistency tests of the tracking literature on them, on the host.

The filtered state and covariance themselves, per node, are handed out by `filter_tracks`, `filter_tracks_ct`, `filter_tracks_ais` (and
`filter_nodes`, `Tracker.getFilteredTracks`): the forward half of the smoother with its (xf, Pf) stored (`mht_filter_tracks*`, one
launch) -- what `pymht_amd.evaluation.nees_nodes` holds against ground truth.

One noise level rarely fits a whole track: a ship steams straight, turns for a few scans and steams on.  `imm_tracks`, `imm_tracks_ct`
(and `imm_nodes`, `Tracker.getModeProbabilities`) run an interacting-multiple-model filter over the histories -- the same state under up
to four (Q, R), mixed through a Markov chain over the modes (`mht_imm_tracks*`, one launch, one (track, mode) per lane) -- and hand out
per node the probability of every mode and one combined state and covariance in `filter_tracks`' layout, per track the log-likelihood
under the mixture, comparable with `score_tracks`'; `imm_modes` makes the modes of scalings of the model's own noise.
`imm_smooth_tracks`, `imm_smooth_tracks_ct` (and `imm_smooth_nodes`, `Tracker.getSmoothModeProbabilities`, `getSmoothTracks(imm=..)`)
walk the same filter forward and a mode-matched RTS pass backward (`mht_imm_smooth_tracks*`): the mode probabilities in hindsight and
one smoothed state and covariance that needs no choice of a single noise level."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .device import Context


# (family, model kind) -> the seam, its workspace sizer, whether the sizer takes nx in front of (n_tracks, L_max), whether it takes the
# number of modes / candidates behind them.  Every seam takes (ctx, model, n, L_max, len, x_init, P_init, z, has_z) first and
# (work, work_bytes) behind its outputs; an AIS seam takes its per-node arrays and the leg table behind has_z (`_launch`).
_SEAMS = {("smooth", "linear"): ("mht_smooth_tracks", "mht_smooth_work_bytes", True, False),
          ("smooth", "ct"): ("mht_smooth_tracks_ct", "mht_smooth_ct_work_bytes", False, False),
          ("smooth", "ais"): ("mht_smooth_tracks_ais", "mht_smooth_ais_work_bytes", False, False),
          ("em", "linear"): ("mht_smooth_tracks_em", "mht_smooth_em_work_bytes", True, False),
          ("em_ll", "linear"): ("mht_smooth_tracks_em_ll", "mht_smooth_em_work_bytes", True, False),
          ("score", "linear"): ("mht_score_tracks", "mht_score_work_bytes", True, False),
          ("score", "ct"): ("mht_score_tracks_ct", "mht_score_work_bytes", True, False),
          ("score", "ais"): ("mht_score_tracks_ais", "mht_score_work_bytes", True, False),
          ("score_grid", "linear"): ("mht_score_tracks_grid", "mht_score_grid_work_bytes", True, True),
          ("score_grid", "ct"): ("mht_score_tracks_ct_grid", "mht_score_grid_work_bytes", True, True),
          ("trace", "linear"): ("mht_trace_tracks", "mht_trace_work_bytes", True, False),
          ("trace", "ct"): ("mht_trace_tracks_ct", "mht_trace_work_bytes", True, False),
          ("trace", "ais"): ("mht_trace_tracks_ais", "mht_trace_work_bytes", True, False),
          ("filter", "linear"): ("mht_filter_tracks", "mht_filter_work_bytes", True, False),
          ("filter", "ct"): ("mht_filter_tracks_ct", "mht_filter_work_bytes", True, False),
          ("filter", "ais"): ("mht_filter_tracks_ais", "mht_filter_work_bytes", True, False),
          ("imm", "linear"): ("mht_imm_tracks", "mht_imm_work_bytes", True, True),
          ("imm", "ct"): ("mht_imm_tracks_ct", "mht_imm_work_bytes", True, True),
          ("imm_smooth", "linear"): ("mht_imm_smooth_tracks", "mht_imm_smooth_work_bytes", True, True),
          ("imm_smooth", "ct"): ("mht_imm_smooth_tracks_ct", "mht_imm_smooth_work_bytes", True, True)}
EM_MAX_ITER = 64      # (SMOOTH_EM_MAX_ITER of csrc/mht_smooth_em.h)


def _check_model(model):
    if getattr(model, "transition", None) == "ct":
        raise NotImplementedError("smoothing: the transition of model %r depends on the state (Phi(T, w) per hypothesis, models/ct.py); the "
                                  "linear Rauch-Tung-Striebel recursion does not apply and it is not run with Phi(T, 0) in its place"
                                  % getattr(model, "__name__", model))
    nx = int(np.asarray(model.C_RADAR).shape[1])
    if nx not in (4, 6):
        raise ValueError("smoothing: 4- or 6-state models (got %d states)" % nx)
    return nx


def _measurement_array(measurements):
    """[L, 2] float64, NaN rows where the node has no measurement (None, or NaN already)."""
    if isinstance(measurements, np.ndarray) and measurements.dtype != object:
        return np.asarray(measurements, dtype=np.float64).reshape(-1, 2)
    z = np.full((len(measurements), 2), np.nan)
    for k, m in enumerate(measurements):
        if m is not None:
            z[k] = np.asarray(m, dtype=np.float64).reshape(2)
    return z


def _check_ct_model(model):
    if getattr(model, "transition", None) != "ct":
        raise ValueError("smoothing: constant-turn smoothing needs a model whose transition is \"ct\" (models/ct.py); model %r has no turn "
                         "rate to read" % getattr(model, "__name__", model))
    if np.asarray(model.C_RADAR).shape[1] != 6:
        raise ValueError("smoothing: the constant-turn model has 6 states (got %d)" % np.asarray(model.C_RADAR).shape[1])
    return 6


def _check_ais_model(model):
    if getattr(model, "transition", None) == "ct" or np.asarray(model.C_RADAR).shape[1] != 4:
        raise ValueError("smoothing: AIS messages report four states [x, y, vx, vy]: AIS-aware smoothing needs a 4-state linear model "
                         "(model %r is not one)" % getattr(model, "__name__", model))
    return 4


def _ais_inputs(model, tracks):
    """Host side of `smooth_tracks_ais`, checked before any device is needed: per track (has_message [L] bool, message [L, 4],
    r [L], leg [L] int32), and the leg table [n_legs, 52] -- per distinct (dT1, dT2): Phi(dT1) [16], the upper triangle of Q(dT1) [10],
    Phi(dT2), Q(dT2), as the model returns them (float32: the matrices the forest filtered with, ais.py::group_messages), widened."""
    from .ais import SIGMA_HIGH, SIGMA_LOW
    iu = np.triu_indices(4)
    widen = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64).reshape(4, 4)
    index, table, per_track = {}, [], []
    for t, track in enumerate(tracks):
        if len(track) != 4:
            raise ValueError("smoothing: an AIS-aware track is (x_init, P_init, measurements, ais) (track %d has %d entries)" % (t, len(track)))
        L, ais = len(track[2]), track[3]
        if len(ais) != L:
            raise ValueError("smoothing: track %d has %d nodes and %d AIS entries" % (t, L, len(ais)))
        has, msg, r, leg = np.zeros(L, dtype=bool), np.zeros((L, 4)), np.ones(L), np.zeros(L, dtype=np.int32)
        for k in range(1, L):      # (entry 0 belongs to the node x_init is the state of and is not used)
            if ais[k] is None:
                continue
            dT1, dT2, state, high = ais[k]
            dT1, dT2 = float(dT1), float(dT2)
            if not (dT1 > 0.0 and dT2 > 0.0):
                raise ValueError("smoothing: track %d node %d: an AIS message lies strictly inside the step to its node "
                                 "(dT1 = %r, dT2 = %r must be positive)" % (t, k, dT1, dT2))
            if (dT1, dT2) not in index:
                index[(dT1, dT2)] = len(table)
                A1, Q1, A2, Q2 = widen(model.Phi(dT1)), widen(model.Q(dT1)), widen(model.Phi(dT2)), widen(model.Q(dT2))
                table.append(np.concatenate([A1.ravel(), Q1[iu], A2.ravel(), Q2[iu]]))
            has[k], leg[k] = True, index[(dT1, dT2)]
            msg[k] = np.asarray(state, dtype=np.float64).reshape(4)
            r[k] = float(np.power(SIGMA_HIGH if high else SIGMA_LOW, 2))
        per_track.append((has, msg, r, leg))
    return per_track, np.array(table, dtype=np.float64).reshape(len(table), 52)


def smooth_tracks(model, radarPeriod, tracks, device=0, ctx=None, covariances=True):
    """Smooth a batch of track histories.

    model        a model module (pymht_amd.models.pv / .ca: Phi, Q, C_RADAR, R_RADAR); `transition == "ct"` raises NotImplementedError
    tracks       list of (x_init [nx], P_init [nx, nx], measurements): one entry of `measurements` per node of the track -- a 2-vector, or
                 None / a NaN row for a node without a radar measurement.  Entry 0 belongs to the node x_init is the state of and is
                 not used (what `Target.backtrackMeasurement()` returns can be handed in as it is).
    device, ctx  the GPU ordinal, or an existing pymht_amd.device.Context (a Tracker's) to run on
    Returns per track (xs [L, nx], Ps [L, nx, nx]) float64, Ps None with covariances=False (means only: the cheaper kernel)."""
    return _run(_smooth, [], ctx, device, model, radarPeriod, tracks, _check_model(model), "linear", covariances)


def smooth_tracks_ct(model, radarPeriod, tracks, device=0, ctx=None, covariances=True):
    """`smooth_tracks` for a constant-turn model (`model.transition == "ct"`: pymht_amd.models.ct; anything else raises ValueError): same
    arguments, same outputs with nx = 6.  A_k = Phi(T, w) at the filtered turn rate of node k, in float64 and not rounded to float32 as
    `model.Phi` returns it, no Jacobian with respect to w."""
    return _run(_smooth, [], ctx, device, model, radarPeriod, tracks, _check_ct_model(model), "ct", covariances)


def smooth_tracks_ais(model, radarPeriod, tracks, device=0, ctx=None, covariances=True):
    """`smooth_tracks` for the histories of an AIS-aided tracker, with the AIS updates the forest applied (4-state linear models;
    anything else raises ValueError).  tracks: list of (x_init, P_init, measurements, ais) -- the first three as for `smooth_tracks`, and
    ais[k] None or (dT1, dT2, state [4], highAccuracy) for a node that took a message: made dT1 behind the node in front and dT2 in
    front of the node itself (both positive, else ValueError), reporting [x, y, vx, vy] with sigma 1 (highAccuracy) or 3.  Entry 0 is
    not used.  Same outputs as `smooth_tracks`; a batch without any message gives its numbers bit for bit."""
    return _run(_smooth, [], ctx, device, model, radarPeriod, tracks, _check_ais_model(model), "ais", covariances)


def _check_em(n_iter, start):
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or not 0 <= n_iter <= EM_MAX_ITER:
        raise ValueError("smoothing: n_iter is an int in 0 .. %d (got %r)" % (EM_MAX_ITER, n_iter))
    if start not in ("model", "reference"):
        raise ValueError("smoothing: start is \"model\" (the tracker's Q(T), R_RADAR() and each track's P_init) or \"reference\" "
                         "(identity Q, R and P0: pykalman's defaults); got %r" % (start,))
    return int(n_iter), start


def smooth_tracks_em(model, radarPeriod, tracks, n_iter=5, start="model", device=0, ctx=None, covariances=True, likelihoods=False):
    """`smooth_tracks` with Q, R and the initial state learned per track by `n_iter` EM iterations first (linear models; a constant-turn
    model raises NotImplementedError).  start="model": theta begins at the tracker's Q(T), R_RADAR() and each track's P_init;
    start="reference": at identity Q, R and P0 (the reference gives pykalman the transition matrix, the observation matrix and the
    initial mean, and pykalman's default for the rest is the identity), so that n_iter=5 is the reference's procedure.  n_iter: an int
    in 0 .. 64 (0: `smooth_tracks` under the start values), anything else and any other `start` raise ValueError.
    Returns per track (xs [L, nx], Ps [L, nx, nx] or None, Q [nx, nx], R [2, 2]).  A track whose re-estimated covariances stop being
    positive definite comes back NaN, that track only.
    likelihoods=True (a bool, else TypeError): each track's tuple gains a last element ll [n_iter + 1], its log-likelihood
    (`score_tracks`' definition) under theta_0 -- the start values: ll[0] is `score_tracks`' figure under them, bit for bit -- theta_1, ..
    and theta_n_iter, what the output was smoothed under.  EM never decreases it: the trace says whether the iterations improved the
    fit and whether they were still moving.  The other outputs are the same bits; it costs n_iter + 1 forward-only launches
    (`mht_smooth_tracks_em_ll`)."""
    nx = _check_model(model)
    if not isinstance(likelihoods, (bool, np.bool_)):
        raise TypeError("smoothing: likelihoods is a bool (got %r)" % (likelihoods,))
    return _run(_smooth, [], ctx, device, model, radarPeriod, tracks, nx, "linear", covariances, em=_check_em(n_iter, start), likelihoods=bool(likelihoods))


_MODEL_CHECKS = {"linear": _check_model, "ct": _check_ct_model, "ais": _check_ais_model}      # each returns nx


def _run(family, empty, ctx, device, model, radarPeriod, tracks, nx, kind, *args, **kwargs):
    """family(ctx, model, period, tracks, nx, *args, constant_turn, ais, **kwargs) on the caller's context, or on one of this call's own
    that is closed behind it.  The callers have checked the model (nx) and their own arguments; the AIS inputs are checked here, before a
    device is needed; an empty batch gives `empty` without one."""
    ais = None
    if kind == "ais":
        ais, tracks = _ais_inputs(model, tracks), [t[:3] for t in tracks]
    if len(tracks) == 0:
        return empty
    own = ctx is None
    if own:
        ctx = Context(device, nx=nx)
    try:
        return family(ctx, model, float(radarPeriod), tracks, nx, *args, kind == "ct", ais, **kwargs)
    finally:
        if own:
            ctx.close()


def _pack(ctx, tracks, nx, identity_start=False):
    """The batch on the device, track-minor ([node][element][track]), tracks of similar length side by side: a wavefront runs as long as
    the longest of its 64 tracks (stable: equal lengths keep their order).  Returns (lens, order, L_max, hp, (x_d, P_d, z_d, h_d))."""
    n = len(tracks)
    zs = [_measurement_array(t[2]) for t in tracks]
    lens = np.array([len(z) for z in zs], dtype=np.int32)
    if lens.min() < 1:
        raise ValueError("smoothing: a track without nodes")
    order = np.argsort(-lens, kind="stable")
    L_max = int(lens.max())
    zp = np.zeros((n, L_max, 2))
    hp = np.zeros((n, L_max), dtype=np.uint8)
    x0 = np.empty((n, nx))
    P0 = np.empty((n, nx * nx))
    for j, t in enumerate(order):
        z = zs[t]
        has = ~np.isnan(z).any(axis=1)
        has[0] = False
        zp[j, :len(z)] = np.where(has[:, None], z, 0.0)
        hp[j, :len(z)] = has
        x0[j] = np.asarray(tracks[t][0], dtype=np.float64).reshape(nx)
        P0[j] = np.asarray(tracks[t][1], dtype=np.float64).reshape(nx * nx)
    if identity_start:
        P0[:] = np.eye(nx).reshape(nx * nx)
    up = lambda a: torch.from_numpy(a).to(ctx.device)
    z_d = up(zp).permute(1, 2, 0).contiguous()
    h_d = up(hp).permute(1, 0).contiguous()
    x_d = up(x0).permute(1, 0).contiguous()
    P_d = up(P0).permute(1, 0).contiguous()
    return lens, order, L_max, hp, (x_d, P_d, z_d, h_d)


def _pack_ais(ctx, ais, order, hp, L_max):
    """The per-node AIS inputs next to z / has_z, and the leg table: (the seam's arguments between has_z and its outputs, the device
    arrays behind them -- kept by the caller until the seam has returned)."""
    per_track, legs = ais
    n = len(order)
    up = lambda a: torch.from_numpy(a).to(ctx.device)
    kp = hp.copy()
    mp, rp, lp = np.zeros((n, L_max, 4)), np.ones((n, L_max)), np.zeros((n, L_max), dtype=np.int32)
    for j, t in enumerate(order):
        has_m, msg, r, leg = per_track[t]
        kp[j, :len(has_m)] += 2 * has_m.astype(np.uint8)
        mp[j, :len(has_m)], rp[j, :len(has_m)], lp[j, :len(has_m)] = msg, r, leg
    # the seam cannot see these device arrays: its contract is checked here, before the upload
    fused = kp >= 2
    if not np.array_equal(kp & 1, hp) or (fused.any() and (lp[fused].min() < 0 or lp[fused].max() >= len(legs))) or not (rp > 0).all():
        raise ValueError("smoothing: inconsistent AIS inputs (a leg index outside the table of %d entries, or a variance that is not positive)" % len(legs))
    k_d = up(kp).permute(1, 0).contiguous()
    m_d = up(mp).permute(1, 2, 0).contiguous()
    r_d = up(rp).permute(1, 0).contiguous()
    l_d = up(lp).permute(1, 0).contiguous()
    legs_d = up(legs) if len(legs) else None
    return (k_d.data_ptr(), m_d.data_ptr(), r_d.data_ptr(), l_d.data_ptr(), legs_d.data_ptr() if len(legs) else None, len(legs)), (k_d, m_d, r_d, l_d, legs_d)


def _model_x(model, period, nx, constant_turn, identity_start=False):
    """(the seam's mht_model_x, the float32 arrays it points into).  The constant-turn seams build their own transition per node:
    Phi(T, 0) stands in the struct and is not read."""
    mats = (model.Phi(period), np.eye(nx) if identity_start else model.Q(period), model.C_RADAR, np.eye(2) if identity_start else model.R_RADAR())
    keep = [np.ascontiguousarray(np.asarray(m, dtype=np.float32).ravel()) for m in mats]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    return _lib.MhtModelX(nx, fp(keep[0]), fp(keep[1]), fp(keep[2]), fp(keep[3]), 0.0, 0.0, 1 if constant_turn else 0, period), keep


def _launch(ctx, model, period, tracks, nx, constant_turn, family, ais, middle, make_outs, trailing=0, identity_start=False):
    """One seam call over a batch: the batch packed and uploaded (`_pack`, `_pack_ais`), the workspace the seam's sizer asks for, the
    model, and the call through `_lib.check`.  middle: the seam's arguments between the batch and its outputs (ints as they are, NumPy
    arrays as host pointers; the first is the count of modes / candidates where the sizer takes one); make_outs(L_max): its output
    tensors in the seam's order (None for one left out), the last `trailing` of them behind the workspace.  Everything the seam reads
    lives here until it has returned (it synchronises).  Returns (lens, order, L_max, hp, outs)."""
    n, dev, lib = len(tracks), ctx.device, ctx.lib
    lens, order, L_max, hp, batch = _pack(ctx, tracks, nx, identity_start)
    extra, ais_keep = _pack_ais(ctx, ais, order, hp, L_max) if ais is not None else ((), None)
    outs = list(make_outs(L_max))
    seam, sizer, takes_nx, takes_count = _SEAMS[family, "ais" if ais is not None else "ct" if constant_turn else "linear"]
    need = int(getattr(lib, sizer)(*((nx,) if takes_nx else ()), n, L_max, *((middle[0],) if takes_count else ())))
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    mx, keep = _model_x(model, period, nx, constant_turn, identity_start)
    lens_sorted = np.ascontiguousarray(lens[order])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a.data_ptr() if isinstance(a, torch.Tensor) else a
    outs_p = [ptr(o) for o in outs]
    torch.cuda.current_stream(dev).synchronize()      # (the packing above ran on torch's stream)
    _lib.check(getattr(lib, seam)(ctx.handle, C.byref(mx), n, L_max, ptr(lens_sorted), *(ptr(b) for b in batch), *extra, *(ptr(m) for m in middle),
                                  *outs_p[:len(outs) - trailing], work.data_ptr(), need, *outs_p[len(outs) - trailing:]), lib)
    return lens, order, L_max, hp, outs


def _unpack_index(nx, dev):
    """Per entry (i, j) of a full nx x nx matrix, row-major, its place in the packed upper triangle (sym_idx, csrc/mht_smooth_math.h)"""
    return torch.tensor([min(i, j) * nx - min(i, j) * (min(i, j) - 1) // 2 + abs(i - j) for i in range(nx) for j in range(nx)], device=dev)


def _per_track(rows_d, nx=None):
    """A per-node device array [L_max, elements, n] on the host as [track][node][element]; with nx the elements are a packed upper
    triangle, unpacked on the device to [track][node][nx, nx]"""
    if nx is None:
        return rows_d.permute(2, 0, 1).contiguous().cpu().numpy()
    full = rows_d.index_select(1, _unpack_index(nx, rows_d.device)).permute(2, 0, 1).contiguous().cpu().numpy()
    return full.reshape(full.shape[0], full.shape[1], nx, nx)


def _full(packed, nx):
    """Host: symmetric [.., nx, nx] from a packed upper triangle [.., nx (nx + 1) / 2], row by row"""
    iu = np.triu_indices(nx)
    full = np.empty(packed.shape[:-1] + (nx, nx))
    full[..., iu[0], iu[1]] = packed
    full[..., iu[1], iu[0]] = packed
    return full


def _back(order):
    """back[t]: the packed column the callers' track t sits in"""
    back = np.empty(len(order), dtype=np.int64)
    back[order] = np.arange(len(order))
    return back


def _smooth(ctx, model, period, tracks, nx, covariances, constant_turn, ais=None, em=None, likelihoods=False, on_device=False):
    """on_device=True (internal: Tracker.getNees): nothing is downloaded -- (xs_d [L_max, nx, n], Ps_d [L_max, ns, n], lens, order, L_max),
    the seam's outputs where they lie, packed column j holding track order[j]."""
    n, ns, dev = len(tracks), nx * (nx + 1) // 2, ctx.device
    # (the smoothers leave the rows behind a track's end as they were, the filters write NaN there: handed on as they lie, the arrays
    # start as NaN, so that both read the same and nothing of an earlier allocation shows through)
    rows = (lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)) if on_device else (lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev))

    def make_outs(L_max):      # xs, Ps; EM: the learned Q (packed) and R behind them, and the trace of log-likelihoods behind the workspace
        outs = [rows(L_max, nx, n), rows(L_max, ns, n) if covariances else None]
        if em is not None:
            outs += [torch.empty((ns, n), dtype=torch.float64, device=dev), torch.empty((3, n), dtype=torch.float64, device=dev)]
        return outs + ([torch.empty((em[0] + 1, n), dtype=torch.float64, device=dev)] if likelihoods else [])
    family = "smooth" if em is None else "em_ll" if likelihoods else "em"
    lens, order, L_max, hp, outs = _launch(ctx, model, period, tracks, nx, constant_turn, family, ais, () if em is None else (em[0],), make_outs,
                                           trailing=1 if likelihoods else 0, identity_start=em is not None and em[1] == "reference")
    if on_device:
        return outs[0], outs[1], lens, order, L_max
    xs = _per_track(outs[0])
    Ps = _per_track(outs[1], nx) if covariances else None
    if em is not None:
        Q = _full(outs[2].permute(1, 0).contiguous().cpu().numpy(), nx)
        R = outs[3].permute(1, 0).contiguous().cpu().numpy()[:, [0, 1, 1, 2]].reshape(n, 2, 2)
    if likelihoods:
        ll = outs[4].permute(1, 0).contiguous().cpu().numpy()      # [track][n_iter + 1]
    out = [None] * n
    for j, t in enumerate(order):
        L = int(lens[t])
        learned = () if em is None else (Q[j], R[j]) + ((ll[j],) if likelihoods else ())
        out[t] = (xs[j, :L], Ps[j, :L] if covariances else None) + learned
    return out


def score_tracks(model, radarPeriod, tracks, device=0, ctx=None):
    """How well `model` explains each of a batch of track histories: per track (logLikelihood, nis, nObs).  `model` and `tracks` as for
    `smooth_tracks` (the same checks and refusals; an empty list gives an empty list).  Over every node k >= 1 with a radar plot, with
    v = z_k - C xp_k and S = C Pp_k C' + R from the filter `smooth_tracks` runs forward (the same filtered states, bit for bit):
        nis = sum v' S^-1 v                                  chi-square with 2 nObs degrees of freedom over a consistent filter
        logLikelihood = -1/2 sum (ln det S + v' S^-1 v + 2 ln 2 pi)
    Node 0 is the initial state and is not an observation -- pykalman's loglikelihood() counts one at time 0, so these are not its
    figures.  A track of one node, or one never detected, gives (0.0, 0.0, 0).  One forward-only device launch (`mht_score_tracks`)."""
    return _run(_score, [], ctx, device, model, radarPeriod, tracks, _check_model(model), "linear")


def score_tracks_ct(model, radarPeriod, tracks, device=0, ctx=None):
    """`score_tracks` under the constant-turn model `smooth_tracks_ct` smooths with (anything else raises ValueError)."""
    return _run(_score, [], ctx, device, model, radarPeriod, tracks, _check_ct_model(model), "ct")


def score_tracks_ais(model, radarPeriod, tracks, device=0, ctx=None):
    """`score_tracks` under the AIS-aware model of `smooth_tracks_ais`, same `tracks` and refusals: per track
    (logLikelihood, nis, nObs, nisAis, nAis).  A node that took a message is scored at the message's time as well, v = m - xp,
    S = Pp + sigma^2 I4: its ln N(m; xp, S) goes into logLikelihood, v' S^-1 v into nisAis (chi-square with 4 nAis degrees of freedom);
    nis and nObs stay radar-only.  A batch without any message gives `score_tracks`' numbers bit for bit."""
    return _run(_score, [], ctx, device, model, radarPeriod, tracks, _check_ais_model(model), "ais")


def _score(ctx, model, period, tracks, nx, constant_turn, ais=None):
    n, dev = len(tracks), ctx.device
    dtypes = (torch.float64, torch.float64, torch.int32) + ((torch.float64, torch.int32) if ais is not None else ())
    lens, order, L_max, hp, outs = _launch(ctx, model, period, tracks, nx, constant_turn, "score", ais, (),
                                           lambda L_max: [torch.empty(n, dtype=dt, device=dev) for dt in dtypes])
    cols = [o.cpu().numpy() for o in outs]
    out = [None] * n
    for j, t in enumerate(order):
        out[t] = tuple(float(c[j]) if c.dtype == np.float64 else int(c[j]) for c in cols)
    return out


TRACE_RADAR_DOUBLES, TRACE_AIS_DOUBLES = 7, 16      # (csrc/mht_smooth_trace.h)


def trace_tracks(model, radarPeriod, tracks, device=0, ctx=None):
    """The innovation sequence behind `score_tracks`: per track a dict of NumPy arrays with a row per node,
        v [L, 2]       z_k - C xp_k                      S [L, 2, 2]    C Pp_k C' + R
        nis [L]        v' S^-1 v                         ll [L]         -1/2 (ln det S + nis + 2 ln 2 pi) = ln N(z_k; C xp_k, S)
        observed [L]   bool: the node has a radar plot (never node 0, the initial state)
    NaN in every row that is not observed.  `model` and `tracks` as for `score_tracks` (the same checks and refusals; an empty list
    gives an empty list).  The filter is `score_tracks`' own, bit for bit: a track's ll and nis added up in node order are its
    logLikelihood and nis there, and observed.sum() its nObs -- the sums say whether a model fits a track, the sequence says where it
    stops (a manoeuvre, a misassociated plot, a run of correlated innovations from a Q too small: `consistency`).  An observed node
    whose det S is not positive keeps v and S and has NaN in nis and ll.  One device launch (`mht_trace_tracks`)."""
    return _run(_trace, [], ctx, device, model, radarPeriod, tracks, _check_model(model), "linear")


def trace_tracks_ct(model, radarPeriod, tracks, device=0, ctx=None):
    """`trace_tracks` under the constant-turn model `score_tracks_ct` scores with (anything else raises ValueError)."""
    return _run(_trace, [], ctx, device, model, radarPeriod, tracks, _check_ct_model(model), "ct")


def trace_tracks_ais(model, radarPeriod, tracks, device=0, ctx=None):
    """`trace_tracks` under the AIS-aware model of `score_tracks_ais`, same `tracks` and refusals.  Each dict also holds, at the
    message's time of a node that took one (v = m - xp, S = Pp + sigma^2 I4; NaN rows elsewhere):
        vAis [L, 4]    SAis [L, 4, 4]    nisAis [L]    llAis [L] = -1/2 (ln det S + nisAis + 4 ln 2 pi)    message [L] bool
    `score_tracks_ais`' logLikelihood is llAis and ll added up in node order, llAis in front of ll at a node with both; nisAis adds
    up to its nisAis.  A batch without any message gives `trace_tracks`' radar arrays bit for bit."""
    return _run(_trace, [], ctx, device, model, radarPeriod, tracks, _check_ais_model(model), "ais")


def _trace_dict(radar, observed, ais=None, message=None):
    """One track's dict from its rows radar [L, 7] (and ais [L, 16]) as the seam lays them out."""
    L = len(radar)
    out = {"v": radar[:, 0:2].copy(), "S": radar[:, [2, 3, 3, 4]].reshape(L, 2, 2), "nis": radar[:, 5].copy(), "ll": radar[:, 6].copy(),
           "observed": np.asarray(observed, dtype=bool).copy()}
    if ais is not None:
        out.update({"vAis": ais[:, 0:4].copy(), "SAis": _full(ais[:, 4:14], 4), "nisAis": ais[:, 14].copy(), "llAis": ais[:, 15].copy(),
                    "message": np.asarray(message, dtype=bool).copy()})
    return out


def _blank_trace(L, ais=False):
    """The trace of a chain nothing was filtered over: L rows, none observed."""
    return _trace_dict(np.full((L, TRACE_RADAR_DOUBLES), np.nan), np.zeros(L, dtype=bool),
                       np.full((L, TRACE_AIS_DOUBLES), np.nan) if ais else None, np.zeros(L, dtype=bool))


def _trace(ctx, model, period, tracks, nx, constant_turn, ais=None):
    n, dev = len(tracks), ctx.device
    widths = (TRACE_RADAR_DOUBLES,) + ((TRACE_AIS_DOUBLES,) if ais is not None else ())
    lens, order, L_max, hp, outs = _launch(ctx, model, period, tracks, nx, constant_turn, "trace", ais, (),
                                           lambda L_max: [torch.empty((L_max, w, n), dtype=torch.float64, device=dev) for w in widths])
    rows = [_per_track(o) for o in outs]
    out = [None] * n
    for j, t in enumerate(order):
        L = int(lens[t])
        out[t] = _trace_dict(rows[0][j, :L], hp[j, :L], rows[1][j, :L] if ais is not None else None,
                             ais[0][t][0] if ais is not None else None)
    return out


def trace_nodes(model, radarPeriod, nodes, device=0, ctx=None, constantTurn=False, ais=None):
    """`trace_tracks` for many track nodes in one device call, built on `chain_inputs` / `chain_ais` like `score_nodes` (the same
    switches and refusals): per node the dict of its chain, with ais also the message arrays.  A chain of fewer than two nodes has
    nothing to explain: its rows are NaN and not observed."""
    kind = _kind(constantTurn, ais, "tracing")
    nx = _MODEL_CHECKS[kind](model)
    out, where, batch = _chains(model, nodes, lambda chain, inputs: _blank_trace(len(chain), ais is not None), ais)
    return _fill(out, where, _run(_trace, [], ctx, device, model, radarPeriod, batch, nx, kind))


def filter_tracks(model, radarPeriod, tracks, device=0, ctx=None):
    """The filtered state and covariance of every node of a batch of track histories: per track (xf [L, nx], Pf [L, nx, nx]) float64.
    `model` and `tracks` as for `smooth_tracks` (the same checks and refusals; an empty list gives an empty list).  Node 0 is
    (x_init, P_init); node k >= 1 is predicted from node k - 1 and, with a plot, updated with it.

    WHAT THESE COVARIANCES ARE: those of the float64 filter the smoothers and the scores run -- the tracker's model, A = Phi(T),
    Q = Q(T), C_RADAR, R_RADAR(), over the history from the chain's initial state.  They are the forward half of `smooth_tracks` bit
    for bit (a track's last row is the last row of its xs and Ps) and the states behind `score_tracks` and `trace_tracks`.  They are NOT
    the forest's own chains bit for bit: the forest filters in float32 (float64 for AIS-fused covariances) with tabulated gains.
    One device launch (`mht_filter_tracks`), no host fallback."""
    return _run(_filter, [], ctx, device, model, radarPeriod, tracks, _check_model(model), "linear")


def filter_tracks_ct(model, radarPeriod, tracks, device=0, ctx=None):
    """`filter_tracks` under the constant-turn model `smooth_tracks_ct` smooths with (anything else raises ValueError): nx = 6,
    A_k = Phi(T, w) at the filtered turn rate of the node in front, no Jacobian."""
    return _run(_filter, [], ctx, device, model, radarPeriod, tracks, _check_ct_model(model), "ct")


def filter_tracks_ais(model, radarPeriod, tracks, device=0, ctx=None):
    """`filter_tracks` under the AIS-aware model of `smooth_tracks_ais`, same `tracks` and refusals.  The state handed out for a node
    that took a message is the one at the SCAN's time, behind both legs and the radar update; the state at the message's time is an
    intermediate.  A batch without any message gives `filter_tracks`' numbers bit for bit."""
    return _run(_filter, [], ctx, device, model, radarPeriod, tracks, _check_ais_model(model), "ais")


def _filter(ctx, model, period, tracks, nx, constant_turn, ais=None, on_device=False):
    """on_device=True (internal: Tracker.getNees): nothing is downloaded -- (xf_d [L_max, nx, n], Pf_d [L_max, ns, n], lens, order, L_max),
    the seam's outputs where they lie, packed column j holding track order[j]."""
    n, dev = len(tracks), ctx.device
    lens, order, L_max, hp, (xf_d, Pf_d) = _launch(ctx, model, period, tracks, nx, constant_turn, "filter", ais, (), lambda L_max: [
        torch.empty((L_max, w, n), dtype=torch.float64, device=dev) for w in (nx, nx * (nx + 1) // 2)])
    if on_device:
        return xf_d, Pf_d, lens, order, L_max
    xf, Pf = _per_track(xf_d), _per_track(Pf_d, nx)
    return [(xf[j, :lens[t]], Pf[j, :lens[t]]) for t, j in enumerate(_back(order))]


def filter_nodes(model, radarPeriod, nodes, device=0, ctx=None, constantTurn=False, ais=None):
    """`filter_tracks` for many track nodes in one device call, built on `chain_inputs` / `chain_ais` like `trace_nodes` (the same
    switches and refusals): per node (xf [L, nx], Pf [L, nx, nx]) of its chain -- the float64 filter of the smoothers and scores, run
    over the history with `model` from the chain's initial state, not the forest's float32 / float64 chains bit for bit.  A chain of
    fewer than two nodes was never filtered: its initial state and covariance, and no device is needed to say so."""
    kind = _kind(constantTurn, ais, "filtering")
    nx = _MODEL_CHECKS[kind](model)
    out, where, batch = _chains(model, nodes, lambda chain, inputs: (inputs[0].reshape(1, nx).copy(), inputs[1].reshape(1, nx, nx).copy()), ais)
    return _fill(out, where, _run(_filter, [], ctx, device, model, radarPeriod, batch, nx, kind))


IMM_MAX_MODES = 4      # (IMM_MAX_MODES of csrc/mht_imm.h)


def _check_scales(q, r):
    """The scales of `imm_modes` and `noise_grid`: flat float64 arrays of finite positive factors, at least one each, else ValueError"""
    for name, sc in (("qScales", q), ("rScales", r)):
        if sc.size == 0 or not (np.isfinite(sc).all() and (sc > 0).all()):
            raise ValueError("smoothing: %s are finite positive factors, at least one (got %r)" % (name, sc.tolist()))
    return q, r


def _noise32(model, radarPeriod):
    """(Q(T) [nx, nx], R_RADAR() [2, 2]) as the float32 matrices every seam is handed (`_model_x`), widened to float64"""
    nx = int(np.asarray(model.C_RADAR).shape[1])
    return (np.asarray(model.Q(float(radarPeriod)), dtype=np.float32).astype(np.float64).reshape(nx, nx),
            np.asarray(model.R_RADAR(), dtype=np.float32).astype(np.float64).reshape(2, 2))


def imm_modes(model, radarPeriod, qScales, rScales=None, stay=0.95):
    """The modes of an interacting-multiple-model filter over scalings of the model's own noise: (Q [r, nx, nx], R [r, 2, 2], Pi [r, r],
    mu0 [r]) float64, one mode per entry of qScales (1 .. 4 of them), mode j being qScales[j] * Q32 and rScales[j] * R32 as `noise_grid`
    makes candidates (the float32 matrices every seam is handed, times float64 scales; rScales defaults to all ones and has qScales'
    length otherwise).  Pi has `stay` on the diagonal and (1 - stay) / (r - 1) elsewhere ([[1.]] for one mode), mu0 is uniform.  Scales
    that are not finite and positive, too many of them, or a `stay` outside (0, 1] raise ValueError."""
    q = np.asarray(qScales, dtype=np.float64).reshape(-1)
    q, r = _check_scales(q, np.ones_like(q) if rScales is None else np.asarray(rScales, dtype=np.float64).reshape(-1))
    if len(q) > IMM_MAX_MODES or len(r) != len(q):
        raise ValueError("smoothing: 1 .. %d modes, a scale of Q and of R each (got %d and %d)" % (IMM_MAX_MODES, len(q), len(r)))
    if isinstance(stay, bool) or not isinstance(stay, (int, float, np.integer, np.floating)) or not 0.0 < float(stay) <= 1.0:
        raise ValueError("smoothing: stay is the probability of keeping a mode, in (0, 1] (got %r)" % (stay,))
    n = len(q)
    Q32, R32 = _noise32(model, radarPeriod)
    Pi = np.ones((1, 1)) if n == 1 else np.where(np.eye(n, dtype=bool), float(stay), (1.0 - float(stay)) / (n - 1))
    return q[:, None, None] * Q32, r[:, None, None] * R32, Pi, np.full(n, 1.0 / n)


def _check_modes(Q, R, Pi, mu0, nx):
    """(Q [r, nx, nx], R [r, 2, 2], Pi [r, r], mu0 [r]) float64 C-contiguous, or ValueError: `_check_candidates`' checks capped at four
    modes, and Pi's rows and mu0 distributions over them (the seam's own check, made before a device is needed)"""
    Q, R = _check_candidates(Q, R, nx)
    r = len(Q)
    if r > IMM_MAX_MODES:
        raise ValueError("smoothing: 1 .. %d modes a call (got %d)" % (IMM_MAX_MODES, r))
    Pi = np.ascontiguousarray(Pi, dtype=np.float64)
    mu0 = np.full(r, 1.0 / r) if mu0 is None else np.ascontiguousarray(mu0, dtype=np.float64)
    if Pi.shape != (r, r) or mu0.shape != (r,):
        raise ValueError("smoothing: Pi is [%d, %d] and mu0 [%d] for %d modes (got %r and %r)" % (r, r, r, r, Pi.shape, mu0.shape))
    for name, p in (("Pi", Pi), ("mu0", mu0[None, :])):
        if not ((p >= 0.0) & (p <= 1.0)).all() or not (np.abs(p.sum(axis=1) - 1.0) <= 1e-9).all():
            raise ValueError("smoothing: %s holds probabilities, every row adding up to 1 (got %r)" % (name, p.tolist()))
    return Q, R, Pi, mu0


def imm_tracks(model, radarPeriod, tracks, Q, R, Pi, mu0=None, device=0, ctx=None):
    """An interacting-multiple-model filter (Blom and Bar-Shalom 1988) over a batch of track histories: `filter_tracks`' float64 filter
    run under r <= 4 noise levels at once, mode j carrying Q[j] [nx, nx] and R[j] [2, 2] in place of the model's Q(T) and R_RADAR()
    (float64, symmetric; `imm_modes` makes scalings of the model's own), mixed through the Markov chain Pi [r, r] --
    Pi[i, j] = P(mode j at node k | mode i at node k - 1), rows adding up to 1, zeros allowed -- from the probabilities mu0 [r] at node 0
    (uniform by default).  `model` and `tracks` as for `filter_tracks`, with its checks and refusals; bad modes raise ValueError.
    Returns (per track (mu [L, r], x [L, nx], P [L, nx, nx]), ll [n], nObs [n]) in the order of `tracks`: per node the posterior
    probability of every mode -- a manoeuvre detector per track and scan -- and the combined state and covariance, in `filter_tracks`'
    layout (what `evaluation.nees_nodes` takes); per track the log-likelihood of its plots under the mixture, comparable with
    `score_tracks`' figure under one model, and their number.  Node 0 is (mu0, x_init, P_init).  With one mode (Pi = [[1.]]) x and P are
    `filter_tracks`' bits and ll, nObs `score_tracks`'.  A mode that is no covariance (det S not positive at some plot) makes that
    track's ll NaN, and no other's.  An empty list gives ([], shape (0,), shape (0,)).  One device launch (`mht_imm_tracks`), one
    (track, mode) per lane, no host fallback."""
    return _imm_run(_imm, ctx, device, model, radarPeriod, tracks, Q, R, Pi, mu0, _check_model(model), "linear")


def imm_tracks_ct(model, radarPeriod, tracks, Q, R, Pi, mu0=None, device=0, ctx=None):
    """`imm_tracks` under the constant-turn model `filter_tracks_ct` filters with (anything else raises ValueError): nx = 6, every mode's
    Phi(T, w) taken at the turn rate of its own mixed state."""
    return _imm_run(_imm, ctx, device, model, radarPeriod, tracks, Q, R, Pi, mu0, _check_ct_model(model), "ct")


def _imm_run(family, ctx, device, model, radarPeriod, tracks, Q, R, Pi, mu0, nx, kind):
    """`_run` behind the check of the modes, which an empty batch is held to as well"""
    empty = [] if family is _imm_smooth else ([], np.zeros(0), np.zeros(0, dtype=np.int32))
    return _run(family, empty, ctx, device, model, radarPeriod, tracks, nx, kind, *_check_modes(Q, R, Pi, mu0, nx))


def _imm_launch(ctx, model, period, tracks, nx, constant_turn, family, modes, n_mu):
    """An IMM seam over a batch: n_mu arrays of mode probabilities [L_max, r, n] around the combined state and covariance, then ll and
    nObs.  Returns (lens, order, the mode probabilities [track][node][mode] each, x, P, ll, nObs), the last two in packed order."""
    n, r, dev = len(tracks), len(modes[0]), ctx.device
    rows = lambda L_max, w: torch.empty((L_max, w, n), dtype=torch.float64, device=dev)
    lens, order, L_max, hp, outs = _launch(ctx, model, period, tracks, nx, constant_turn, family, None, (r,) + tuple(modes), lambda L_max: [
        rows(L_max, r), rows(L_max, nx), rows(L_max, nx * (nx + 1) // 2)] + [rows(L_max, r)] * (n_mu - 1) + [
        torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)])
    mus = [_per_track(outs[0])] + [_per_track(o) for o in outs[3:-2]]
    return lens, order, mus, _per_track(outs[1]), _per_track(outs[2], nx), outs[-2].cpu().numpy(), outs[-1].cpu().numpy()


def _imm(ctx, model, period, tracks, nx, Q, R, Pi, mu0, constant_turn, ais=None):
    lens, order, (mu,), xo, Po, ll, nobs = _imm_launch(ctx, model, period, tracks, nx, constant_turn, "imm", (Q, R, Pi, mu0), 1)
    back = _back(order)
    return [(mu[j, :lens[t]], xo[j, :lens[t]], Po[j, :lens[t]]) for t, j in enumerate(back)], ll[back], nobs[back]


def imm_nodes(model, radarPeriod, nodes, Q, R, Pi, mu0=None, device=0, ctx=None, constantTurn=False):
    """`imm_tracks` for many track nodes in one device call, built on `chain_inputs` like `filter_nodes`: (per node (mu [L, r], x [L, nx],
    P [L, nx, nx]) of its chain, ll [n], nObs [n]).  A chain of fewer than two nodes was never filtered: mu0, its initial state and
    covariance, ll = 0.0, nObs = 0, and no device is needed to say so.  constantTurn as for `filter_nodes`; the messages of an AIS-aided
    tracker are not taken (there is no AIS-aware IMM)."""
    kind = _kind(constantTurn)
    nx = _MODEL_CHECKS[kind](model)
    Q, R, Pi, mu0 = _check_modes(Q, R, Pi, mu0, nx)
    out, where, batch = _chains(model, nodes, lambda chain, inputs: (mu0.reshape(1, -1).copy(), inputs[0].reshape(1, nx).copy(),
                                                                     inputs[1].reshape(1, nx, nx).copy()))
    ll, nobs = np.zeros(len(nodes)), np.zeros(len(nodes), dtype=np.int32)
    res, ll[where], nobs[where] = _imm_run(_imm, ctx, device, model, radarPeriod, batch, Q, R, Pi, mu0,
                                           nx, kind)
    return _fill(out, where, res), ll, nobs


def imm_smooth_tracks(model, radarPeriod, tracks, Q, R, Pi, mu0=None, device=0, ctx=None):
    """The fixed-interval IMM smoother over a batch of track histories: `imm_tracks`' filter walked forward, then a mode-matched
    Rauch-Tung-Striebel pass walked backward (Nadarajah, Tharmarasa, McDonald, Kirubarajan 2012, restated in csrc/mht_imm_smooth.h) --
    the probability of every mode IN HINDSIGHT, which is on time at the start of a manoeuvre and at its end where the filter's is
    several scans late, and one smoothed state and covariance that needs no choice of a single noise level.  Arguments, checks and
    refusals are `imm_tracks`'.  Returns one dict per track, in the order of `tracks`:
        mu [L, r] the smoothed mode probabilities, muFiltered [L, r] `imm_tracks`' own (its bits),
        x [L, nx], P [L, nx, nx] the smoothed combined state and covariance in `filter_tracks`' layout -- `evaluation.nees_nodes`
        takes them as they are --, logLikelihood and nObs as `imm_tracks` gives them (its bits).
    At a track's last node mu, x, P are `imm_tracks`' bits.  With one mode (Pi = [[1.]]) x and P are `smooth_tracks`' bits and mu is
    exactly 1.  An empty list gives [].  One device launch (`mht_imm_smooth_tracks`), one (track, mode) per lane, no host fallback."""
    return _imm_run(_imm_smooth, ctx, device, model, radarPeriod, tracks, Q, R, Pi, mu0, _check_model(model), "linear")


def imm_smooth_tracks_ct(model, radarPeriod, tracks, Q, R, Pi, mu0=None, device=0, ctx=None):
    """`imm_smooth_tracks` under the constant-turn model `smooth_tracks_ct` smooths with (anything else raises ValueError): nx = 6, going
    backward every mode's Phi(T, w) is taken at the turn rate of its own filtered state."""
    return _imm_run(_imm_smooth, ctx, device, model, radarPeriod, tracks, Q, R, Pi, mu0, _check_ct_model(model), "ct")


def _imm_smooth(ctx, model, period, tracks, nx, Q, R, Pi, mu0, constant_turn, ais=None):
    lens, order, (mus, muf), xo, Po, ll, nobs = _imm_launch(ctx, model, period, tracks, nx, constant_turn, "imm_smooth", (Q, R, Pi, mu0), 2)
    return [dict(mu=mus[j, :lens[t]], muFiltered=muf[j, :lens[t]], x=xo[j, :lens[t]], P=Po[j, :lens[t]], logLikelihood=float(ll[j]), nObs=int(nobs[j]))
            for t, j in enumerate(_back(order))]


def imm_smooth_nodes(model, radarPeriod, nodes, Q, R, Pi, mu0=None, device=0, ctx=None, constantTurn=False):
    """`imm_smooth_tracks` for many track nodes in one device call, built on `chain_inputs` like `imm_nodes`: one dict per node.  A chain
    of fewer than two nodes was never filtered: mu0 twice, its initial state and covariance, logLikelihood 0.0, nObs 0, and no device
    is needed to say so.  constantTurn as for `imm_nodes`; AIS messages are not taken."""
    kind = _kind(constantTurn)
    nx = _MODEL_CHECKS[kind](model)
    Q, R, Pi, mu0 = _check_modes(Q, R, Pi, mu0, nx)
    out, where, batch = _chains(model, nodes, lambda chain, inputs: dict(
        mu=mu0.reshape(1, -1).copy(), muFiltered=mu0.reshape(1, -1).copy(), x=inputs[0].reshape(1, nx).copy(), P=inputs[1].reshape(1, nx, nx).copy(),
        logLikelihood=0.0, nObs=0))
    return _fill(out, where, _imm_run(_imm_smooth, ctx, device, model, radarPeriod, batch, Q, R, Pi, mu0, nx, kind))


def consistency(traces, alpha=0.05):
    """The filter-consistency tests of the tracking literature (Bar-Shalom, Li, Kirubarajan: Estimation with Applications to Tracking
    and Navigation, ch. 5.4) on the radar innovations of `trace_tracks*` dicts, pooled over `traces`; host only, float64.  A dict of
        nObs             the observed nodes
        nisMean          their nis summed, divided by nObs: 2 under a consistent filter
        nisInterval      (lo, hi) = chi2.ppf([alpha/2, 1 - alpha/2], 2 nObs) / nObs: where nisMean then lies with probability 1 - alpha
        nisInside        lo <= nisMean <= hi.  Below: the filter's S is too large (R or Q too large); above: too small, or a bias
        outlierFraction  the share of observed nodes with nis > chi2.ppf(1 - alpha, 2); alpha under a consistent filter
        rho1             the lag-one autocorrelation of the whitened innovations e_k = L_k^-1 v_k, S_k = L_k L_k', over the nPairs
                         pairs of consecutive nodes k, k + 1 of one track that both have a plot:
                         sum e_k . e_{k+1} / sqrt(sum |e_k|^2  sum |e_{k+1}|^2)
        rho1Bound        norm.ppf(1 - alpha/2) / sqrt(2 nPairs): |rho1| stays below it with probability 1 - alpha when the
                         innovations are white (a Q too small, or an unmodelled manoeuvre, correlates them)
        white            |rho1| <= rho1Bound
        nPairs, alpha
    Without an observed node (without a pair) the statistics that need one are NaN and their verdict is None; so is the verdict over a
    statistic that is NaN.  An observed node with a NaN nis (a det S that was not positive) makes nisMean and outlierFraction NaN, as it
    makes the track's score NaN.  alpha outside (0, 1) raises ValueError."""
    from scipy.stats import chi2, norm
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not 0.0 < float(alpha) < 1.0:
        raise ValueError("smoothing: alpha is a probability strictly between 0 and 1 (got %r)" % (alpha,))
    alpha = float(alpha)
    nan = float("nan")
    n_obs = n_pairs = 0
    nis_sum = num = den_a = den_b = 0.0
    outliers = 0
    threshold = float(chi2.ppf(1.0 - alpha, 2))
    for tr in traces:
        obs = np.asarray(tr["observed"], dtype=bool)
        nis = np.asarray(tr["nis"], dtype=np.float64)[obs]
        n_obs += int(obs.sum())
        nis_sum += float(np.sum(nis))
        outliers += int(np.sum(nis > threshold))
        pair = obs[:-1] & obs[1:]
        if not pair.any():
            continue
        v, S = np.asarray(tr["v"], dtype=np.float64), np.asarray(tr["S"], dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):      # (rows that are not observed are NaN, and are not read below)
            l00 = np.sqrt(S[:, 0, 0])
            l10 = S[:, 0, 1] / l00
            l11 = np.sqrt(S[:, 1, 1] - l10 * l10)
            e0 = v[:, 0] / l00
            e = np.stack([e0, (v[:, 1] - l10 * e0) / l11], axis=1)
        a, b = e[:-1][pair], e[1:][pair]
        n_pairs += int(pair.sum())
        num += float(np.sum(a * b))
        den_a += float(np.sum(a * a))
        den_b += float(np.sum(b * b))
    out = {"nObs": n_obs, "nPairs": n_pairs, "alpha": alpha, "nisMean": nan, "nisInterval": (nan, nan), "nisInside": None,
           "outlierFraction": nan, "rho1": nan, "rho1Bound": nan, "white": None}
    if n_obs > 0:
        lo, hi = (float(q) / n_obs for q in chi2.ppf([alpha / 2.0, 1.0 - alpha / 2.0], 2 * n_obs))
        out["nisMean"], out["nisInterval"] = nis_sum / n_obs, (lo, hi)
        if np.isfinite(out["nisMean"]):
            out["nisInside"] = bool(lo <= out["nisMean"] <= hi)
            out["outlierFraction"] = outliers / n_obs
    if n_pairs > 0:
        with np.errstate(invalid="ignore", divide="ignore"):
            out["rho1"] = float(np.float64(num) / np.sqrt(np.float64(den_a) * np.float64(den_b)))
        out["rho1Bound"] = float(norm.ppf(1.0 - alpha / 2.0) / np.sqrt(2.0 * n_pairs))
        if np.isfinite(out["rho1"]):
            out["white"] = bool(abs(out["rho1"]) <= out["rho1Bound"])
    return out


GRID_MAX_CAND = 4096      # (SCORE_GRID_MAX_CAND of csrc/mht_smooth_score_grid.hip)


def noise_grid(model, radarPeriod, qScales, rScales):
    """The candidates of a likelihood surface over scalings of the model's own noise: (Q [G, nx, nx], R [G, 2, 2]) float64 with
    G = len(qScales) * len(rScales), candidate iq * len(rScales) + ir being qScales[iq] * Q32 and rScales[ir] * R32 -- Q32 = Q(T) and
    R32 = R_RADAR() as float32, the matrices every seam is handed (`_model_x`), so that scale 1 is the tracker's model itself.  The
    products are float64: the grid is not rounded to float32.  Scales are finite and positive, else ValueError."""
    q, r = _check_scales(*(np.asarray(s, dtype=np.float64).reshape(-1) for s in (qScales, rScales)))
    Q32, R32 = _noise32(model, radarPeriod)
    Q = np.repeat(q, len(r))[:, None, None] * Q32
    R = np.tile(r, len(q))[:, None, None] * R32
    return Q, R


def _check_candidates(Q, R, nx):
    """(Q [G, nx, nx], R [G, 2, 2]) float64 C-contiguous, or ValueError"""
    Q, R = np.ascontiguousarray(Q, dtype=np.float64), np.ascontiguousarray(R, dtype=np.float64)
    if Q.ndim != 3 or Q.shape[1:] != (nx, nx) or R.ndim != 3 or R.shape[1:] != (2, 2) or len(Q) != len(R):
        raise ValueError("smoothing: the candidates are Q [G, %d, %d] and R [G, 2, 2] (got %r and %r)" % (nx, nx, Q.shape, R.shape))
    if not 1 <= len(Q) <= GRID_MAX_CAND:
        raise ValueError("smoothing: 1 .. %d candidates a call (got %d)" % (GRID_MAX_CAND, len(Q)))
    # (NaN is not symmetric either: the seam reads the upper triangle and would never see a bad lower one)
    if not (np.array_equal(Q, Q.transpose(0, 2, 1)) and np.array_equal(R, R.transpose(0, 2, 1))):
        raise ValueError("smoothing: a candidate covariance is not symmetric")
    return Q, R


def score_tracks_grid(model, radarPeriod, tracks, Q, R, device=0, ctx=None):
    """`score_tracks` under G candidate noise models in ONE device launch (`mht_score_tracks_grid`): the histories are packed and
    uploaded once, and every (track, candidate) is a lane of its own.  Q [G, nx, nx] and R [G, 2, 2] (float64, symmetric, 1 <= G <= 4096,
    else ValueError; `noise_grid` makes a grid of scalings) replace the model's Q(T) and R_RADAR(); Phi(T) and C_RADAR stay.  `model`
    and `tracks` as for `score_tracks`, with its checks and refusals.
    Returns (ll [G, n], nis [G, n], nObs [n]) as NumPy arrays in the order of `tracks`; nObs does not depend on the candidate.  Row g is
    what `score_tracks` gives for a model that carries candidate g -- bit for bit where the candidate is representable in float32, the
    precision a model's matrices are handed over in; the candidates themselves are not rounded.  A candidate that is no covariance
    (det S not positive at some plot) gives NaN in its (candidate, track) cells only.  An empty list gives shapes (G, 0), (G, 0), (0,)."""
    return _score_grid_run(ctx, device, model, radarPeriod, tracks, Q, R, _check_model(model), "linear")


def score_tracks_ct_grid(model, radarPeriod, tracks, Q, R, device=0, ctx=None):
    """`score_tracks_grid` under the constant-turn model `score_tracks_ct` scores with (anything else raises ValueError)."""
    return _score_grid_run(ctx, device, model, radarPeriod, tracks, Q, R, _check_ct_model(model), "ct")


def _score_grid_run(ctx, device, model, radarPeriod, tracks, Q, R, nx, kind):
    """`_run` behind the check of the candidates, which an empty batch is held to as well"""
    Q, R = _check_candidates(Q, R, nx)
    empty = np.zeros((len(Q), 0)), np.zeros((len(Q), 0)), np.zeros(0, dtype=np.int32)
    return _run(_score_grid, empty, ctx, device, model, radarPeriod, tracks, nx, kind, Q, R)


def _score_grid(ctx, model, period, tracks, nx, Q, R, constant_turn, ais=None):
    n, G, dev = len(tracks), len(Q), ctx.device
    lens, order, L_max, hp, (ll_d, nis_d, nobs_d) = _launch(ctx, model, period, tracks, nx, constant_turn, "score_grid", None, (G, Q, R), lambda L_max: [
        torch.empty((G, n), dtype=torch.float64, device=dev), torch.empty((G, n), dtype=torch.float64, device=dev),
        torch.empty(n, dtype=torch.int32, device=dev)])
    back = _back(order)
    return ll_d.cpu().numpy()[:, back], nis_d.cpu().numpy()[:, back], nobs_d.cpu().numpy()[back]


def chain_inputs(node, default_P0):
    """What the reference hands to its smoother for the track that ends in `node`: the initial state of the chain and
    backtrackMeasurement().  P_init is the first node's own covariance (the birth's), `default_P0` where it has none."""
    chain = node.backtrackNodes()
    first = chain[0]
    P = first.P_0
    return chain, (np.asarray(first.x_0, dtype=np.float64), np.asarray(default_P0 if P is None else P, dtype=np.float64),
                   [c.measurement for c in chain])


def chain_ais(chain, lookup):
    """The AIS entries `smooth_tracks_ais` takes for a chain of an AIS-aided tracker: a node with `mmsi` set took the message
    lookup(scanNumber, mmsi) -- made dT1 = message.time - parent.time behind its parent and dT2 = node.time - message.time in front of
    itself.  A node whose message the look-up does not have raises RuntimeError: it is never smoothed as radar-only."""
    ais = [None] * len(chain)
    for k in range(1, len(chain)):      # (node 0 is the chain's initial state, however it came about)
        node = chain[k]
        if node.mmsi is None:
            continue
        msg = lookup(node.scanNumber, node.mmsi)
        if msg is None:
            raise RuntimeError("smoothing: the node of scan %r was updated by an AIS message of mmsi %r, and the AIS history of that "
                               "scan has no such message" % (node.scanNumber, node.mmsi))
        ais[k] = (float(msg.time) - float(chain[k - 1].time), float(node.time) - float(msg.time), msg.state, bool(msg.highAccuracy))
    return ais


def _kind(constantTurn, ais=None, verb=None):
    """The model kind behind a *_nodes function's switches; the AIS look-up and constantTurn together are refused"""
    if ais is not None and constantTurn:
        raise ValueError("smoothing: AIS-aware %s is for 4-state linear models, not together with constantTurn" % verb)
    return "ais" if ais is not None else "ct" if constantTurn else "linear"


def _chains(model, nodes, short, lookup=None):
    """The chain loop of the *_nodes functions: (out, where, batch) -- out[i] = short(chain, inputs) for a chain of fewer than two
    nodes, which no device is needed for; the `chain_inputs` of every other node i in `batch` (with `chain_ais` behind them under an AIS
    look-up) and i in `where`"""
    out, batch, where = [None] * len(nodes), [], []
    for i, node in enumerate(nodes):
        chain, inputs = chain_inputs(node, model.P0)
        if len(chain) < 2:
            out[i] = short(chain, inputs)
        else:
            batch.append(inputs if lookup is None else inputs + (chain_ais(chain, lookup),))
            where.append(i)
    return out, where, batch


def _fill(out, where, results):
    for i, res in zip(where, results):
        out[i] = res
    return out


def smooth_nodes(model, radarPeriod, nodes, device=0, ctx=None, constantTurn=False, ais=None, em=0, emStart="model"):
    """`Target.getSmoothTrack` for many track nodes in one device call: per node (positions [L, 2], velocities [L, 2], ok) as the
    reference returns them.  A chain of fewer than two nodes has nothing to smooth: its measurements, NaN velocities and False.
    constantTurn=True: the nodes are a constant-turn tracker's and go through `smooth_tracks_ct` (ValueError for any other model); by
    default such a model is refused (NotImplementedError).
    ais: None, or a callable (scanNumber, mmsi) -> message (time, state, highAccuracy) of an AIS-aided tracker: the chains go through
    `smooth_tracks_ais` with the messages their nodes took (`chain_ais`).  Not together with constantTurn (ValueError).
    em > 0: the chains go through `smooth_tracks_em(n_iter=em, start=emStart)`; not together with constantTurn or ais (ValueError before
    anything runs).  ok is then False as well for a track whose output is not finite."""
    kind = _kind(constantTurn, ais, "smoothing")
    n_iter, emStart = _check_em(em, emStart)
    if n_iter > 0 and kind != "linear":
        raise ValueError("smoothing: em learns the noise of the plain linear model, not together with constantTurn or ais")
    nx = _MODEL_CHECKS[kind](model)

    def unsmoothed(chain, inputs):
        pos = _measurement_array(inputs[2])
        return pos, np.full_like(pos, np.nan), False
    out, where, batch = _chains(model, nodes, unsmoothed, ais)
    res = _run(_smooth, [], ctx, device, model, radarPeriod, batch, nx, kind, False, em=(n_iter, emStart) if n_iter > 0 else None)
    return _fill(out, where, [(xs[:, 0:2], xs[:, 2:4], n_iter == 0 or bool(np.isfinite(xs).all())) for xs, *_ in res])


def score_nodes(model, radarPeriod, nodes, device=0, ctx=None, constantTurn=False, ais=None):
    """`score_tracks` for many track nodes in one device call, built on `chain_inputs` / `chain_ais` like `smooth_nodes` (the same
    switches and refusals): per node (logLikelihood, nis, nObs), with ais also (.., nisAis, nAis).  A chain of fewer than two nodes has
    nothing to explain: (0.0, 0.0, 0)."""
    kind = _kind(constantTurn, ais, "scoring")
    nx = _MODEL_CHECKS[kind](model)
    out, where, batch = _chains(model, nodes, lambda chain, inputs: (0.0, 0.0, 0) + ((0.0, 0) if ais is not None else ()), ais)
    return _fill(out, where, _run(_score, [], ctx, device, model, radarPeriod, batch, nx, kind))


def best_cell(ll):
    """The index (a tuple of ints) of the largest finite entry of a likelihood surface, the first in C order on ties; None if no entry
    is finite (NaN marks a candidate that is no covariance, -inf is no likelihood either)."""
    ll = np.asarray(ll, dtype=np.float64)
    finite = np.isfinite(ll)
    if not finite.any():
        return None
    return tuple(int(i) for i in np.unravel_index(np.argmax(np.where(finite, ll, -np.inf)), ll.shape))


def score_nodes_grid(model, radarPeriod, nodes, Q, R, device=0, ctx=None, constantTurn=False):
    """`score_tracks_grid` for many track nodes in one device call, built on `chain_inputs` like `score_nodes`: (ll [G, n], nis [G, n],
    nObs [n]) with a column per node.  A chain of fewer than two nodes has nothing to explain: zeros in its column.  constantTurn as
    for `score_nodes`; the messages of an AIS-aided tracker are not scored (the grid has no AIS model)."""
    kind = _kind(constantTurn)
    nx = _MODEL_CHECKS[kind](model)
    Q, R = _check_candidates(Q, R, nx)
    out, where, batch = _chains(model, nodes, lambda chain, inputs: None)
    ll, nis, nobs = np.zeros((len(Q), len(nodes))), np.zeros((len(Q), len(nodes))), np.zeros(len(nodes), dtype=np.int32)
    ll[:, where], nis[:, where], nobs[where] = _score_grid_run(ctx, device, model, radarPeriod, batch, Q, R, nx, kind)
    return ll, nis, nobs
