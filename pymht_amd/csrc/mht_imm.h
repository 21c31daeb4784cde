// One track of the smoothers' models under an INTERACTING-MULTIPLE-MODEL filter (Blom and Bar-Shalom 1988): the same state run under
// r <= 4 noise levels (Q_j, R_j), mixed through a Markov chain Pi over the modes, with the posterior probability of every mode and one
// combined state and covariance handed out per node (mht_imm_tracks, include/mht_amd.h).  The code the lanes of the kernels of
// mht_imm.hip run, and tests/hostmath/imm_host.cpp per track on the CPU.
//
// It is the first walk here whose lanes talk to each other: A LANE IS ONE (TRACK, MODE), and what a mode needs of the others -- their
// probabilities, their likelihoods, their states for the mixing and the combination -- comes through a LANES policy:
//   count()        the modes this caller runs one after the other: 1 in a kernel (the lane's own), r on the host
//   mode(q)        the mode of the q-th of them
//   lane(q)        its ImmLane
//   get(q, i, e)   element e of mode i's shared row s = [x | P packed | mu | lam | u], asked for by the q-th
// A kernel's policy reads the lane's OWN element e in lane i of its quad; the host's reads an array.  The walk is written in phases,
// each run for every mode before the next begins, and a phase writes only what no mode reads in that phase -- on a wavefront, where
// the four lanes of a quad run in lock step, that is program order; on the host it is what makes the modes run in lock step.
//
// Node 0: every mode holds (x_init, P_init), mu = mu0, the combined state is (x_init, P_init).  Node k >= 1, sums over i ascending:
//   mix       cbar_j = sum_i Pi[i][j] mu_i;  cbar_j > 0: w_ij = Pi[i][j] mu_i / cbar_j, x0_j = sum_i w_ij x_i,
//             P0_j = sum_i w_ij (P_i + (x_i - x0_j)(x_i - x0_j)');  cbar_j == 0: mode j keeps its own (x_j, P_j)
//   step      the policy's advance of (x0_j, P0_j) under Q_j (constant turn: at x0_j[4]); with a plot smooth_score_update under R_j, whose
//             term of the score is lam_j = ln N(z; C xp_j, S_j)
//   weigh     with a plot: m = max_j lam_j, u_j = cbar_j exp(lam_j - m), s = sum_j u_j, mu_j = u_j / s, ll += m + ln s, nObs += 1;
//             without: mu_j = cbar_j.  No logarithm of cbar or mu is taken: zeros in Pi are legal
//   combine   x = sum_j mu_j x_j,  P = sum_j mu_j (P_j + (x_j - x)(x_j - x)')
// The mixing and the combination stream over the modes one element at a time (imm_moments), means first and then covariances: no other
// mode's state is ever wholly live.  Every mode of a track computes the same combined (x, P), ll and nObs from the same operands in the
// same order; mode 0 stores them.  A det S that is not positive in some mode gives NaN in lam_j, hence in s and in ll of that track.
//
// With one mode (Pi = [[1]]) every weight is exactly 1 and every difference exactly 0: x, P are mht_filter_tracks' bits and ll is
// mht_score_tracks'.  The AIS-aware step policy is not run here (its per-node message arrays have no place in ImmArgs).
#pragma once
#include "mht_smooth_score.h"
#include "mht_smooth_score_grid.h"

namespace mht {

constexpr int IMM_MAX_MODES = 4;

template <int N, typename Steps>
struct ImmArgs {
    Steps steps;              // A (or the period) and C; Q and R are the modes'
    int32_t n, L_max, r;      // tracks, rows, modes
    const int32_t* len;       // [n] (in the workspace)
    const double* x_init;     // [N][n]
    const double* P_init;     // [N*N][n]
    const double* z;          // [L_max][2][n]
    const uint8_t* has_z;     // [L_max][n]
    const double* modes;      // [r][NS + 3]: Q packed, R00, R01, R11 (smooth_score_grid_row; in the workspace)
    const double* Pi;         // [r][r] row-major (in the workspace)
    const double* mu0;        // [r] (in the workspace)
    double* mu;               // [L_max][r][n]
    double* x;                // [L_max][N][n]
    double* P;                // [L_max][N(N+1)/2][n]
    double* ll;               // [n]
    int32_t* nobs;            // [n]
};

template <int N, typename Steps>
struct ImmLane {
    static constexpr int NV = N + N * (N + 1) / 2;                             // [x | P packed]
    static constexpr int E_MU = NV, E_LAM = NV + 1, E_U = NV + 2, E = NV + 3;   // the shared row
    Steps steps;              // the batch's, with the mode's R (its Q: row)
    const double* row;        // the mode's Q, packed: read where the advance adds it, node after node (it stays in the cache)
    double pi[IMM_MAX_MODES]; // Pi[i][j]: into this mode
    double s[E];              // what the other modes may read
    double m[NV];             // the mode's own working state: mixed, advanced, updated
    double cbar, top, ll;
    int32_t nobs;
};

// out = sum_i w[i] v_i over [x | P]: out_x = sum_i w[i] x_i, then out_P = sum_i w[i] (P_i + (x_i - out_x)(x_i - out_x)'), one element of
// one mode live at a time
template <int N, typename Steps, typename Lanes>
MHT_HD void imm_moments(const Lanes& L, int q, int r, const double* w, double* out) {
    constexpr int NS = N * (N + 1) / 2;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        double acc = w[0] * L.get(q, 0, e);
#pragma unroll
        for (int i = 1; i < IMM_MAX_MODES; ++i)
            if (i < r) acc = fma(w[i], L.get(q, i, e), acc);
        out[e] = acc;
    }
#pragma unroll
    for (int e = 0; e < NS; ++e) out[N + e] = 0.0;
#pragma unroll
    for (int i = 0; i < IMM_MAX_MODES; ++i)
        if (i < r) {
            double d[N];
#pragma unroll
            for (int e = 0; e < N; ++e) d[e] = L.get(q, i, e) - out[e];
#pragma unroll
            for (int a = 0; a < N; ++a)
#pragma unroll
                for (int b = a; b < N; ++b) {
                    const int e = N + sym_idx(N, a, b);
                    const double term = fma(d[a], d[b], L.get(q, i, e));
                    out[e] = i == 0 ? w[0] * term : fma(w[i], term, out[e]);
                }
        }
}

template <int N, typename Steps, typename Lanes>
MHT_HD void imm_mix(Lanes& L, int q, int r) {
    ImmLane<N, Steps>& me = L.lane(q);
    constexpr int NV = ImmLane<N, Steps>::NV, E_MU = ImmLane<N, Steps>::E_MU;
    double w[IMM_MAX_MODES];
    double cbar = me.pi[0] * L.get(q, 0, E_MU);
    w[0] = cbar;
#pragma unroll
    for (int i = 1; i < IMM_MAX_MODES; ++i) {
        w[i] = 0.0;
        if (i < r) {
            const double mu_i = L.get(q, i, E_MU);
            w[i] = me.pi[i] * mu_i;
            cbar = fma(me.pi[i], mu_i, cbar);
        }
    }
#pragma unroll
    for (int i = 0; i < IMM_MAX_MODES; ++i) w[i] = w[i] / cbar;
    double mixed[NV];
    imm_moments<N, Steps>(L, q, r, w, mixed);      // (every mode reads here, whatever its cbar: the choice below is a select)
    const bool reached = cbar > 0.0;
#pragma unroll
    for (int e = 0; e < NV; ++e) me.m[e] = reached ? mixed[e] : me.s[e];
    me.cbar = cbar;
}

// The policies' advance under the mode's Q [NS] packed, READ WHERE IT IS ADDED: the prediction is made row by row -- row i of A P, then
// row i of (A P) A' + Q from it -- every element by the expression smooth_predict and smooth_ct_predict have for it, so the bits are
// theirs.  smooth_score_walk_theta holds its theta's Q in registers; a lane here carries its shared row and the mixed state on top of
// the filter kernel's, and with Q held as well the six-state kernels came to 246 registers (linear) and past 256 (constant turn: two
// in the accumulator half).  Read from the table, node after node -- 21 loads that stay in the cache -- they are 211 and 220.
template <int N, typename Args>
MHT_HD void imm_advance(const LinearSteps<N>& s, const double* Q, const Args&, int, int, double* x, double* P) {
    constexpr int NS = N * (N + 1) / 2;
    const SmoothModel<N>& m = s.model;
    double xp[N], Pp[NS];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double acc = m.A[i * N] * x[0];
#pragma unroll
        for (int k = 1; k < N; ++k) acc = fma(m.A[i * N + k], x[k], acc);
        xp[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double AP[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double acc = m.A[i * N] * P[sym_idx(N, 0, j)];
#pragma unroll
            for (int k = 1; k < N; ++k) acc = fma(m.A[i * N + k], P[sym_idx(N, k, j)], acc);
            AP[j] = acc;
        }
#pragma unroll
        for (int j = i; j < N; ++j) {
            double acc = Q[sym_idx(N, i, j)];
#pragma unroll
            for (int k = 0; k < N; ++k) acc = fma(AP[k], m.A[j * N + k], acc);
            Pp[sym_idx(N, i, j)] = acc;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = xp[i];
#pragma unroll
    for (int e = 0; e < NS; ++e) P[e] = Pp[e];
}

template <typename Args>
MHT_HD void imm_advance(const ConstantTurnSteps& s, const double* Q, const Args&, int, int, double* x, double* P) {
    const SmoothCtModel& m = s.model;
    const CtTransition t = ct_transition(m.T, x[4]);
    double xp[6], Pp[21];
    ct_apply(t, m.T, x, xp);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double AP[6], o[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {      // entry i of A (column j of P): ct_apply's expression for out[i]
            double col[6], oc[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) col[k] = P[sym_idx(6, k, j)];
            ct_apply(t, m.T, col, oc);
            AP[j] = oc[i];
        }
        ct_apply(t, m.T, AP, o);
#pragma unroll
        for (int j = i; j < 6; ++j) Pp[sym_idx(6, i, j)] = o[j] + Q[sym_idx(6, i, j)];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = xp[i];
#pragma unroll
    for (int e = 0; e < 21; ++e) P[e] = Pp[e];
}

// The mode's own filter step on its mixed state; then the state is the others' to read
template <int N, typename Steps, typename Args>
MHT_HD void imm_step(ImmLane<N, Steps>& me, const Args& a, int k, int t, bool has, double z0, double z1) {
    constexpr int NV = ImmLane<N, Steps>::NV;
    imm_advance(me.steps, me.row, a, k, t, me.m, me.m + N);
    double lam = 0.0;
    if (has) {
        ScoreSums acc;
        smooth_score_update<N>(me.steps.model, z0, z1, me.m, me.m + N, acc);
        lam = acc.ll + acc.poison;      // (0 - the score's term: its bits)
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) me.s[e] = me.m[e];
    me.s[ImmLane<N, Steps>::E_LAM] = lam;
}

template <int N, typename Steps, typename Lanes>
MHT_HD void imm_weigh(Lanes& L, int q, int r) {
    ImmLane<N, Steps>& me = L.lane(q);
    constexpr int E_LAM = ImmLane<N, Steps>::E_LAM;
    double top = L.get(q, 0, E_LAM);
#pragma unroll
    for (int i = 1; i < IMM_MAX_MODES; ++i)
        if (i < r) top = fmax(top, L.get(q, i, E_LAM));
    me.top = top;
    me.s[ImmLane<N, Steps>::E_U] = me.cbar * exp(me.s[E_LAM] - top);
}

template <int N, typename Steps, typename Lanes>
MHT_HD void imm_normalise(Lanes& L, int q, int r) {
    ImmLane<N, Steps>& me = L.lane(q);
    constexpr int E_U = ImmLane<N, Steps>::E_U;
    double sum = L.get(q, 0, E_U);
#pragma unroll
    for (int i = 1; i < IMM_MAX_MODES; ++i)
        if (i < r) sum += L.get(q, i, E_U);
    me.s[ImmLane<N, Steps>::E_MU] = me.s[E_U] / sum;
    me.ll += me.top + log(sum);
    me.nobs += 1;
}

// Row k of the outputs: every mode its probability, mode 0 the combined state
template <int N, typename Steps>
MHT_HD void imm_store(const ImmArgs<N, Steps>& a, int k, int t, int j, double mu, const double* xP) {
    constexpr int NS = N * (N + 1) / 2;
    const size_t n = (size_t)a.n;
    a.mu[((size_t)k * a.r + j) * n + t] = mu;
    if (j != 0) return;
#pragma unroll
    for (int i = 0; i < N; ++i) a.x[((size_t)k * N + i) * n + t] = xP[i];
#pragma unroll
    for (int e = 0; e < NS; ++e) a.P[((size_t)k * NS + e) * n + t] = xP[N + e];
}

// Track t; L holds the modes this caller runs (one lane's, or all of them in turn).  r STAYS A RUN-TIME NUMBER in the kernels: the
// wavefront-uniform branches around the modes that are not there are also what keeps the compiler from gathering every mode's elements
// ahead of the sums -- an instance per r, tried, holds r states after all (six states, four modes: 256 registers and 98 to 131 in the
// accumulator half, scratch under the constant-turn model).  The price is in profiles/imm_cost.txt: two modes run no faster than three.
template <int N, typename Steps, typename Lanes>
MHT_HD void imm_walk(const ImmArgs<N, Steps>& a, int t, Lanes& L) {
    const int r = a.r;
    constexpr int NS = N * (N + 1) / 2, NV = N + NS, E_MU = ImmLane<N, Steps>::E_MU;
    const size_t n = (size_t)a.n;
    const int len = a.len[t];      // 1 <= len <= L_max: checked by the host before the launch
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
            for (int b = i; b < N; ++b) me.s[N + sym_idx(N, i, b)] = a.P_init[(size_t)(i * N + b) * n + t];
        me.s[E_MU] = a.mu0[j];
        me.s[ImmLane<N, Steps>::E_LAM] = 0.0;
        me.s[ImmLane<N, Steps>::E_U] = 0.0;
        me.cbar = me.top = me.ll = 0.0;
        me.nobs = 0;
        imm_store(a, 0, t, j, me.s[E_MU], me.s);
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
        for (int q = 0; q < L.count(); ++q) {
            double w[IMM_MAX_MODES], out[NV];
#pragma unroll
            for (int i = 0; i < IMM_MAX_MODES; ++i) {
                w[i] = 0.0;
                if (i < r) w[i] = L.get(q, i, E_MU);
            }
            imm_moments<N, Steps>(L, q, r, w, out);
            imm_store(a, k, t, L.mode(q), L.lane(q).s[E_MU], out);
        }
    }
    for (int q = 0; q < L.count(); ++q) {
        double blank[NV];
#pragma unroll
        for (int e = 0; e < NV; ++e) blank[e] = __builtin_nan("");
        for (int k = len; k < a.L_max; ++k) imm_store(a, k, t, L.mode(q), __builtin_nan(""), blank);
        if (L.mode(q) == 0) {
            a.ll[t] = L.lane(q).ll;
            a.nobs[t] = L.lane(q).nobs;
        }
    }
}

}  // namespace mht
