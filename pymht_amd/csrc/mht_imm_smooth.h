// One track of the smoothers' models under the FIXED-INTERVAL IMM SMOOTHER: the interacting-multiple-model filter of mht_imm.h walked
// forward, then a mode-matched Rauch-Tung-Striebel pass walked backward, with the probability of every mode in hindsight and one
// smoothed state and covariance handed out per node (mht_imm_smooth_tracks, include/mht_amd.h).  The code the lanes of the kernels of
// mht_imm_smooth.hip run, and tests/hostmath/imm_smooth_host.cpp per track on the CPU.
//
// The method is the mode-matched RTS smoother of Nadarajah, Tharmarasa, McDonald and Kirubarajan (IEEE Trans. AES 48, 2012) for modes
// that share one state space.  The paper is RESTATED here, not quoted: the recursion below is this project's own wording and operation
// order, and it is what tests/imm_smooth_ref.py evaluates.
//
// Forward: imm_walk's phases (imm_mix, imm_step, imm_weigh, imm_normalise), call for call; on top every mode keeps per node its own
// row [xf_j | Pf_j packed | mu_j] in the workspace (at node 0: x_init, P_init, mu0_j).  The filter's combined state is not formed.
// Backward, last node L - 1: xs_j = xf_j, Ps_j = Pf_j, mus_j = mu_j; the combined (xs, Ps) is the filter's own (a track of one node:
// x_init, P_init as they are).  Backward, node k = L - 2 .. 0, sums over i ascending, every mode j:
//   terms     A_j = A (constant turn: Phi(T, xf_j(k)[4])), xp_j = A_j xf_j(k); for every mode i the prediction under ITS noise,
//             Pp_ji = A_j Pf_j(k) A_j' + Q_i by imm_advance's expressions, U' U = Pp_ji (smooth_cholesky), and
//             lam_ji = -1/2 |U'^-1 (xs_i(k+1) - xp_j)|^2 - sum_e ln U_ee  (the (N/2) ln 2 pi is common to all and left out);
//             m_j = max of lam_ji over the i with Pi[j][i] > 0, lnL_j = m_j + ln sum_i (Pi[j][i] > 0 ? Pi[j][i] exp(lam_ji - m_j) : 0)
//   back-mix  d_j = sum_i Pi[j][i] mus_i(k+1);  d_j > 0: b_i = Pi[j][i] mus_i(k+1) / d_j and (x0_j, P0_j) the moments of the
//             (xs_i(k+1), Ps_i(k+1)) under b;  d_j == 0: mode j's own (xs_j(k+1), Ps_j(k+1)), by a select.  This is imm_mix with row j of
//             Pi where the filter has column j
//   step      the policy's own backward (smooth_backward, smooth_ct_backward: their expressions, Q_j read from
//             the table) from (x0_j, P0_j), given (xf_j(k), Pf_j(k)):
//             Pp = A_j Pf_j A_j' + Q_j, G = Pf_j A_j' Pp^-1, xs_j(k) = xf_j + G (x0_j - xp_j), Ps_j(k) = Pf_j + G (P0_j - Pp) G'
//   weigh     top = max of lnL_j over the j with mu_j(k) > 0, u_j = mu_j(k) > 0 ? mu_j(k) exp(lnL_j - top) : 0, mus_j(k) = u_j / sum_j u_j
//   combine   xs(k), Ps(k): the moments of the (xs_j(k), Ps_j(k)) under mus(k)
// No logarithm of Pi or of a probability is taken and no product 0 * exp(..) is formed: zeros in Pi and modes of probability 0 are
// legal (with Pi = I and mu0 = (0, 1) mode 1 is the plain smoother under Q_1, bit for bit).  The terms come before the back-mix -- they
// need the filtered row and one factor at a time, the back-mix leaves the mixed state live -- which changes no figure.
//
// THE METHOD'S APPROXIMATION, kept as it is: the forward pass predicted mode j from its MIXED state, while the backward gain and the
// terms predict from the mode's own filtered (xf_j(k), Pf_j(k)).  With one mode the two are the same and the result is
// mht_smooth_tracks' (mht_smooth_tracks_ct's) bits.
//
// A lane is one (track, mode) and the Lanes policy is mht_imm.h's; going backward the shared row s = [x | P packed | mu | lam | u] holds
// [xs_j | Ps_j | mus_j (behind the step: mu_j(k)) | lnL_j | u_j].  A lane loads only the rows it stored itself; what it needs of the
// other modes comes through the policy, one element at a time, and every phase writes only what no mode reads in that phase.
#pragma once
#include "mht_imm.h"

namespace mht {

template <int N, typename Steps>
struct ImmSmoothArgs {
    ImmArgs<N, Steps> f;      // the filter's, with mu, x, P the SMOOTHED outputs mus, xs, Ps; ll and nobs may both be null
    double* muf;              // [L_max][r][n] the filtered probabilities, or null
    double* rows;             // workspace [L_max][r][NV + 1][n]: per node and mode [xf | Pf packed | mu]
};

template <int N, typename Steps>
MHT_HD void imm_smooth_keep(const ImmSmoothArgs<N, Steps>& b, int k, int t, int j, const double* s) {
    constexpr int NV = ImmLane<N, Steps>::NV;
    const size_t n = (size_t)b.f.n, at = ((size_t)k * b.f.r + j) * (NV + 1);
#pragma unroll
    for (int e = 0; e < NV + 1; ++e) b.rows[(at + e) * n + t] = s[e];      // (E_MU == NV)
    if (b.muf) b.muf[((size_t)k * b.f.r + j) * n + t] = s[NV];
}

template <int N, typename Steps>
MHT_HD void imm_smooth_kept(const ImmSmoothArgs<N, Steps>& b, int k, int t, int j, double* x, double* P) {
    constexpr int NS = N * (N + 1) / 2, NV = N + NS;
    const size_t n = (size_t)b.f.n, at = ((size_t)k * b.f.r + j) * (NV + 1);
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] = b.rows[(at + e) * n + t];
#pragma unroll
    for (int e = 0; e < NS; ++e) P[e] = b.rows[(at + N + e) * n + t];
}

// lnL_j: how well mode j's prediction from node k explains the smoothed states of node k + 1, over the modes it can go to.  The
// filtered row is loaded anew for every i: one prediction and its factor live at a time
template <int N, typename Steps, typename Lanes>
MHT_HD void imm_smooth_terms(const ImmSmoothArgs<N, Steps>& b, int k, int t, Lanes& L, int q, int r) {
    constexpr int NS = N * (N + 1) / 2;
    ImmLane<N, Steps>& me = L.lane(q);
    double lam[IMM_MAX_MODES] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int i = 0; i < r; ++i) {      // (a loop, not four copies: unrolled, the compiler keeps all four predictions in flight)
        double x[N], U[NS], inv_d[N], y[N];
        imm_smooth_kept(b, k, t, L.mode(q), x, U);
        imm_advance(me.steps, b.f.modes + (size_t)i * (NS + 3), b.f, k, t, x, U);
        smooth_cholesky<N>(U, inv_d);
        double quad = 0.0, ld = 0.0;
#pragma unroll
        for (int e = 0; e < N; ++e) {      // U' y = xs_i - xp_j (forward: U' is lower)
            double acc = L.get(q, i, e) - x[e];
#pragma unroll
            for (int c = 0; c < e; ++c) acc = fma(-y[c], U[sym_idx(N, c, e)], acc);
            y[e] = acc * inv_d[e];
            quad = e == 0 ? y[0] * y[0] : fma(y[e], y[e], quad);
            ld = e == 0 ? log(U[0]) : ld + log(U[sym_idx(N, e, e)]);
        }
        const double v = fma(-0.5, quad, -ld);
#pragma unroll
        for (int c = 0; c < IMM_MAX_MODES; ++c) lam[c] = i == c ? v : lam[c];      // (every index a constant: no array in memory)
    }
    double top = -__builtin_inf();
#pragma unroll
    for (int i = 0; i < IMM_MAX_MODES; ++i)
        if (i < r) top = me.pi[i] > 0.0 ? fmax(top, lam[i]) : top;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < IMM_MAX_MODES; ++i)
        if (i < r) {
            const double term = me.pi[i] * exp(lam[i] - top);
            sum += me.pi[i] > 0.0 ? term : 0.0;
        }
    me.s[ImmLane<N, Steps>::E_LAM] = top + log(sum);
}

// The policies' backward under the mode's Q [NS] packed, READ WHERE IT IS ADDED as imm_advance reads it: the prediction is
// smooth_predict's (smooth_ct_predict's), every element by the expression they have for it, and what follows is their own
// smooth_backward_gain -- so the bits are smooth_backward's and smooth_ct_backward's under a model whose Q is the mode's.  Held in
// registers the mode's Q is per lane, 42 registers at six states on top of a step that fills the file
template <int N>
MHT_HD void imm_smooth_backward(const LinearSteps<N>& s, const double* Q, const double* xf, const double* Pf, double* xs, double* Ps) {
    const SmoothModel<N>& m = s.model;
    double xp[N], AP[N * N], U[N * (N + 1) / 2];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double acc = m.A[i * N] * xf[0];
#pragma unroll
        for (int k = 1; k < N; ++k) acc = fma(m.A[i * N + k], xf[k], acc);
        xp[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double acc = m.A[i * N] * Pf[sym_idx(N, 0, j)];
#pragma unroll
            for (int k = 1; k < N; ++k) acc = fma(m.A[i * N + k], Pf[sym_idx(N, k, j)], acc);
            AP[i * N + j] = acc;
        }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) {
            double acc = Q[sym_idx(N, i, j)];
#pragma unroll
            for (int k = 0; k < N; ++k) acc = fma(AP[i * N + k], m.A[j * N + k], acc);
            U[sym_idx(N, i, j)] = acc;
        }
    smooth_backward_gain<N, true>(xf, Pf, xp, AP, U, xs, Ps);
}

MHT_HD void imm_smooth_backward(const ConstantTurnSteps& s, const double* Q, const double* xf, const double* Pf, double* xs, double* Ps) {
    const SmoothCtModel& m = s.model;
    const CtTransition t = ct_transition(m.T, xf[4]);
    double xp[6], AP[36], U[21];
    ct_apply(t, m.T, xf, xp);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double col[6], o[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) col[i] = Pf[sym_idx(6, i, j)];
        ct_apply(t, m.T, col, o);
#pragma unroll
        for (int i = 0; i < 6; ++i) AP[i * 6 + j] = o[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double o[6];
        ct_apply(t, m.T, AP + i * 6, o);
#pragma unroll
        for (int j = i; j < 6; ++j) U[sym_idx(6, i, j)] = o[j] + Q[sym_idx(6, i, j)];
    }
    smooth_backward_gain<6, true>(xf, Pf, xp, AP, U, xs, Ps);
}

// The smoother's step under the mode's Q, from the back-mixed (x0_j, P0_j) in me.m; then the row is the others' to read, with the
// FILTERED mu_j(k) in it for the weighing
template <int N, typename Steps>
MHT_HD void imm_smooth_step(const ImmSmoothArgs<N, Steps>& b, int k, int t, int j, ImmLane<N, Steps>& me) {
    constexpr int NS = N * (N + 1) / 2, NV = N + NS;
    double xf[N], Pf[NS];
    imm_smooth_kept(b, k, t, j, xf, Pf);
    imm_smooth_backward(me.steps, me.row, xf, Pf, me.m, me.m + N);
#pragma unroll
    for (int e = 0; e < NV; ++e) me.s[e] = me.m[e];
    me.s[ImmLane<N, Steps>::E_MU] = b.rows[(((size_t)k * b.f.r + j) * (NV + 1) + NV) * (size_t)b.f.n + t];
}

template <int N, typename Steps, typename Lanes>
MHT_HD void imm_smooth_weigh(Lanes& L, int q, int r) {
    ImmLane<N, Steps>& me = L.lane(q);
    constexpr int E_MU = ImmLane<N, Steps>::E_MU, E_LAM = ImmLane<N, Steps>::E_LAM;
    double top = -__builtin_inf();
#pragma unroll
    for (int i = 0; i < IMM_MAX_MODES; ++i)
        if (i < r) {
            const double mu_i = L.get(q, i, E_MU), lnl_i = L.get(q, i, E_LAM);
            top = mu_i > 0.0 ? fmax(top, lnl_i) : top;
        }
    const double u = me.s[E_MU] * exp(me.s[E_LAM] - top);
    me.s[ImmLane<N, Steps>::E_U] = me.s[E_MU] > 0.0 ? u : 0.0;
}

template <int N, typename Steps, typename Lanes>
MHT_HD void imm_smooth_normalise(Lanes& L, int q, int r) {
    ImmLane<N, Steps>& me = L.lane(q);
    constexpr int E_U = ImmLane<N, Steps>::E_U;
    double sum = L.get(q, 0, E_U);
#pragma unroll
    for (int i = 1; i < IMM_MAX_MODES; ++i)
        if (i < r) sum += L.get(q, i, E_U);
    me.s[ImmLane<N, Steps>::E_MU] = me.s[E_U] / sum;
}

// Row k of the smoothed outputs from the shared rows: the moments under mus
template <int N, typename Steps, typename Lanes>
MHT_HD void imm_smooth_combine(const ImmSmoothArgs<N, Steps>& b, int k, int t, Lanes& L, int q, int r) {
    constexpr int NV = ImmLane<N, Steps>::NV, E_MU = ImmLane<N, Steps>::E_MU;
    double w[IMM_MAX_MODES], out[NV];
#pragma unroll
    for (int i = 0; i < IMM_MAX_MODES; ++i) {
        w[i] = 0.0;
        if (i < r) w[i] = L.get(q, i, E_MU);
    }
    imm_moments<N, Steps>(L, q, r, w, out);
    imm_store(b.f, k, t, L.mode(q), L.lane(q).s[E_MU], out);
}

// Track t, forward and backward; L holds the modes this caller runs.  r stays a run-time number, as in imm_walk
template <int N, typename Steps, typename Lanes>
MHT_HD void imm_smooth_walk(const ImmSmoothArgs<N, Steps>& b, int t, Lanes& L) {
    const ImmArgs<N, Steps>& a = b.f;
    const int r = a.r;
    constexpr int NS = N * (N + 1) / 2, NV = N + NS, E_MU = ImmLane<N, Steps>::E_MU;
    const size_t n = (size_t)a.n;
    const int len = a.len[t];      // 1 <= len <= L_max: checked by the host before the launch
    // forward: imm_walk's, every mode keeping its row
    for (int q = 0; q < L.count(); ++q) {
        ImmLane<N, Steps>& me = L.lane(q);
        const int j = L.mode(q);
        const double* c = a.modes + (size_t)j * (NS + 3);
        me.steps = a.steps;
        me.row = c;
#pragma unroll
        for (int e = 0; e < 3; ++e) me.steps.model.R[e] = c[NS + e];
#pragma unroll
        for (int i = 0; i < IMM_MAX_MODES; ++i) {
            me.pi[i] = 0.0;
            if (i < r) me.pi[i] = a.Pi[i * r + j];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) me.s[i] = a.x_init[(size_t)i * n + t];
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int c2 = i; c2 < N; ++c2) me.s[N + sym_idx(N, i, c2)] = a.P_init[(size_t)(i * N + c2) * n + t];
        me.s[E_MU] = a.mu0[j];
        me.s[ImmLane<N, Steps>::E_LAM] = 0.0;
        me.s[ImmLane<N, Steps>::E_U] = 0.0;
        me.cbar = me.top = me.ll = 0.0;
        me.nobs = 0;
        imm_smooth_keep(b, 0, t, j, me.s);
    }
    for (int k = 1; k < len; ++k) {
        const bool has = a.has_z[(size_t)k * n + t] != 0;
        const double z0 = a.z[((size_t)k * 2) * n + t], z1 = a.z[((size_t)k * 2 + 1) * n + t];
        for (int q = 0; q < L.count(); ++q) imm_mix<N, Steps>(L, q, r);
        for (int q = 0; q < L.count(); ++q) imm_step<N>(L.lane(q), a, k, t, has, z0, z1);
        if (has) {
            for (int q = 0; q < L.count(); ++q) imm_weigh<N, Steps>(L, q, r);
            for (int q = 0; q < L.count(); ++q) imm_normalise<N, Steps>(L, q, r);
        } else {
            for (int q = 0; q < L.count(); ++q) L.lane(q).s[E_MU] = L.lane(q).cbar;
        }
        for (int q = 0; q < L.count(); ++q) imm_smooth_keep(b, k, t, L.mode(q), L.lane(q).s);
    }
    for (int q = 0; q < L.count(); ++q) {
        ImmLane<N, Steps>& me = L.lane(q);
        const int j = L.mode(q);
        if (j == 0 && a.ll) {
            a.ll[t] = me.ll;
            a.nobs[t] = me.nobs;
        }
#pragma unroll
        for (int i = 0; i < IMM_MAX_MODES; ++i) {      // from here on Pi[j][i]: out of this mode
            me.pi[i] = 0.0;
            if (i < r) me.pi[i] = a.Pi[j * r + i];
        }
    }
    // backward: the rows hold the last node's filtered states, which are its smoothed states
    for (int q = 0; q < L.count(); ++q) {
        if (len == 1) imm_store(a, 0, t, L.mode(q), L.lane(q).s[E_MU], L.lane(q).s);
        else imm_smooth_combine<N, Steps>(b, len - 1, t, L, q, r);
    }
    for (int k = len - 2; k >= 0; --k) {
        for (int q = 0; q < L.count(); ++q) imm_smooth_terms<N, Steps>(b, k, t, L, q, r);
        for (int q = 0; q < L.count(); ++q) imm_mix<N, Steps>(L, q, r);
        for (int q = 0; q < L.count(); ++q) imm_smooth_step<N, Steps>(b, k, t, L.mode(q), L.lane(q));
        for (int q = 0; q < L.count(); ++q) imm_smooth_weigh<N, Steps>(L, q, r);
        for (int q = 0; q < L.count(); ++q) imm_smooth_normalise<N, Steps>(L, q, r);
        for (int q = 0; q < L.count(); ++q) imm_smooth_combine<N, Steps>(b, k, t, L, q, r);
    }
    for (int q = 0; q < L.count(); ++q) {
        const int j = L.mode(q);
        double blank[NV];
#pragma unroll
        for (int e = 0; e < NV; ++e) blank[e] = __builtin_nan("");
        for (int k = len; k < a.L_max; ++k) {
            imm_store(a, k, t, j, __builtin_nan(""), blank);
            if (b.muf) b.muf[((size_t)k * r + j) * n + t] = __builtin_nan("");
        }
    }
}

}  // namespace mht
