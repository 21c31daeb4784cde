// Expectation-maximisation over one track of the linear smoother (mht_smooth_tracks_em, include/mht_amd.h): n_iter times the walk of
// mht_smooth_walk.h under theta = (Q, R, x0, P0) with the sums of the M-step taken on the way back, then one more walk under the learned
// theta that writes the output.  The code a lane of smooth_em_kernel runs, and tests/hostmath/smooth_em_host.cpp per track on the CPU.
//
// What the reference does per track with pykalman before it smooths (pyTarget.py:580-609: em(n_iter = 5), then smooth); the target is
// that algorithm restated (tests/smooth_em_ref.py), not pykalman's bits.  A = Phi(T) and C stay the batch's; per iteration
//   E-step   the forward filter and the backward pass of smooth_walk with covariances: xs_k, Ps_k, G_k = Pf_k A' Pp_{k+1}^-1, and the
//            lag-one covariance X_k = Cov(x_{k+1}, x_k | all z) = Ps_{k+1} G_k'
//   M-step   Q <- 1 / (L - 1) sum_{k = 0 .. L-2} [e e' + A Ps_k A' + Ps_{k+1} - X_k A' - A X_k'],  e = xs_{k+1} - A xs_k
//            R <- 1 / n_obs sum_{k: z_k present} [r r' + C Ps_k C'],  r = z_k - C xs_k   (n_obs == 0: R stays)
//            x0 <- xs_0,  P0 <- Ps_0                                                      (L == 1: nothing is learned)
// A backward step at k has (xs_{k+1}, Ps_{k+1}) on entry and G_k, (xs_k, Ps_k) on exit: one term of both sums, so there is no second
// sweep and no gain is kept per node.
//
// Registers and launches: the six-state backward step fills most of a lane's file on its own (mht_smooth.hip).  A loop of walks around
// it in ONE kernel does not fit: A and C sit in scalar registers, every multiply-add wants them in vector registers, and the compiler
// hoists those copies out of the forward loop, the backward loop and then the loop of walks, where both sets are live at once (476
// registers before a single sum, and spills with them).  So a kernel launch is ONE walk (smooth_em_pass), the host launches n_iter + 1
// of them on the stream, and between them theta stays in the workspace; a host caller loops over the same function (smooth_em_walk).
// Inside a pass nothing but the walk's own (x, P) is held from one step to the next; the rest is in the workspace and read where it is used:
//   theta   x0 [N], P0, Q (packed), R [3] of the track, written by a pass for the next; Q is read from there by every step's prediction
//   sq      the sums of the Q update, read-modify-write once per backward step; behind them those of the R update and their count
//   pn      Ps_{k+1} and xs_{k+1}, which a term needs BEHIND the step that overwrites them: parked, and read back instead of held
//           across the step
// all [element][n], track-minor like everything else.
#pragma once
#include "mht_smooth_walk.h"

namespace mht {

constexpr int SMOOTH_EM_MAX_ITER = 64;

// The step and the term behind it are one basic block, and the scheduler would start the term's loads in front of the step -- the very
// registers parking frees.  Nothing is scheduled across this line (device code; a host build has no such scheduler).
#if defined(__HIP_DEVICE_COMPILE__)
#define MHT_EM_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define MHT_EM_SCHED_FENCE() ((void)0)
#endif

template <int N>
struct SmoothEmArgs {
    SmoothArgs<N, LinearSteps<N>> s;      // the batch and the filtered slots, as for smooth_walk; s.Ps may be null
    double* theta;      // workspace [N + 2 NS + 3][n], NS = N (N + 1) / 2
    double* sq;         // workspace [NS + 4][n]
    double* pn;         // workspace [NS + N][n]
    double* Q_out;      // [NS][n]
    double* R_out;      // [3][n]
};

constexpr MHT_HD int smooth_em_track_doubles(int n) { return 2 * n + 4 * (n * (n + 1) / 2) + 7; }      // theta, sq and pn of one track

// S = e e' + A Ps A' + P1 - X A' - A X' (packed) with e = x1 - A xs and X = P1 G': one term of the Q update.  (x1, P1) the smoothed
// state of node k + 1, (xs, Ps) of node k; W holds the gain G of the step between them and is overwritten with A G: X A' = P1 (A G)'.
template <int N>
MHT_HD void smooth_em_q_term(const SmoothModel<N>& m, double* W, const double* x1, const double* P1, const double* xs, const double* Ps,
                             double* S) {
    double e[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double acc = x1[i];
#pragma unroll
        for (int k = 0; k < N; ++k) acc = fma(-m.A[i * N + k], xs[k], acc);
        e[i] = acc;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {      // column j of A G is A times column j of G: in place, the two are never held side by side
        double c[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double acc = m.A[i * N] * W[j];
#pragma unroll
            for (int k = 1; k < N; ++k) acc = fma(m.A[i * N + k], W[k * N + j], acc);
            c[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) W[i * N + j] = c[i];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double AP[N];      // row i of A Ps
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double acc = m.A[i * N] * Ps[sym_idx(N, 0, j)];
#pragma unroll
            for (int k = 1; k < N; ++k) acc = fma(m.A[i * N + k], Ps[sym_idx(N, k, j)], acc);
            AP[j] = acc;
        }
#pragma unroll
        for (int j = i; j < N; ++j) {
            double acc = P1[sym_idx(N, i, j)];
#pragma unroll
            for (int k = 0; k < N; ++k) acc = fma(AP[k], m.A[j * N + k], acc);
#pragma unroll
            for (int k = 0; k < N; ++k) acc = fma(-P1[sym_idx(N, i, k)], W[j * N + k], acc);
#pragma unroll
            for (int k = 0; k < N; ++k) acc = fma(-W[i * N + k], P1[sym_idx(N, k, j)], acc);
            S[sym_idx(N, i, j)] = fma(e[i], e[j], acc);
        }
    }
}

// S = r r' + C Ps C' (r00, r01, r11) with r = z - C xs: one term of the R update
template <int N>
MHT_HD void smooth_em_r_term(const SmoothModel<N>& m, double z0, double z1, const double* xs, const double* Ps, double* S) {
    double r0 = z0, r1 = z1;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        r0 = fma(-m.C[k], xs[k], r0);
        r1 = fma(-m.C[N + k], xs[k], r1);
    }
    double s00 = r0 * r0, s01 = r0 * r1, s11 = r1 * r1;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double c0 = m.C[0] * Ps[sym_idx(N, 0, j)], c1 = m.C[N] * Ps[sym_idx(N, 0, j)];      // column j of C Ps
#pragma unroll
        for (int k = 1; k < N; ++k) {
            c0 = fma(m.C[k], Ps[sym_idx(N, k, j)], c0);
            c1 = fma(m.C[N + k], Ps[sym_idx(N, k, j)], c1);
        }
        s00 = fma(c0, m.C[j], s00);
        s01 = fma(c0, m.C[N + j], s01);
        s11 = fma(c1, m.C[N + j], s11);
    }
    S[0] = s00; S[1] = s01; S[2] = s11;
}

// One walk of track t under its current theta.  first: theta is the call's -- x_init, P_init and the model's Q and R -- and not yet in
// the workspace.  LAST: the walk that writes xs (and Ps), Q_out and R_out; any other one takes the sums of the M-step on its way back
// and leaves the new theta in the workspace.  first && LAST is smooth_walk<N, true> with LinearSteps, call for call.  A track whose
// re-estimated covariances stop being positive definite runs into the square root of a negative number in the Cholesky factor: NaN
// from there on, in this track's outputs only.
template <int N, bool LAST>
MHT_HD void smooth_em_pass(const SmoothEmArgs<N>& a, int t, bool first) {
    constexpr int NS = N * (N + 1) / 2;
    SmoothArgs<N, LinearSteps<N>> s = a.s;      // this track's copy: the model's Q and R are the track's own, A and C stay the batch's
    SmoothModel<N>& m = s.steps.model;
    const size_t n = (size_t)s.n;
    const int len = s.len[t];      // 1 <= len <= L_max: checked by the host before the launch
    const bool learn = !LAST && len > 1;
    double* q = a.theta + (size_t)(N + NS) * n + t;      // the track's Q: read by every step's prediction, never held across a step
    double* r = a.theta + (size_t)(N + 2 * NS) * n + t;  // the track's R: the forward pass's, not held across the backward pass
    double x[N], P[NS];
    if (first) {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = s.x_init[(size_t)i * n + t];
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = i; j < N; ++j) P[sym_idx(N, i, j)] = s.P_init[(size_t)(i * N + j) * n + t];
#pragma unroll
        for (int e = 0; e < NS; ++e) q[(size_t)e * n] = m.Q[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) r[(size_t)e * n] = m.R[e];
    } else {
        const double* th = a.theta + t;
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = th[(size_t)i * n];
#pragma unroll
        for (int e = 0; e < NS; ++e) P[e] = th[(size_t)(N + e) * n];
#pragma unroll
        for (int e = 0; e < 3; ++e) m.R[e] = r[(size_t)e * n];
    }
    if (LAST) {      // (theta is final: out with it here, so that nothing of it is held across the walk)
#pragma unroll
        for (int e = 0; e < NS; ++e) a.Q_out[(size_t)e * n + t] = q[(size_t)e * n];
#pragma unroll
        for (int e = 0; e < 3; ++e) a.R_out[(size_t)e * n + t] = m.R[e];
    }
    // forward, as in smooth_walk (which is left as it is: the kernels built from it keep their registers)
    for (int k = 0; k < len; ++k) {
        if (k > 0) {
#pragma unroll
            for (int e = 0; e < NS; ++e) m.Q[e] = q[(size_t)e * n];
            s.steps.advance(s, k, t, x, P);
            if (s.has_z[(size_t)k * n + t]) smooth_update<N>(m, s.z[((size_t)k * 2) * n + t], s.z[((size_t)k * 2 + 1) * n + t], x, P);
        }
        if (k < len - 1) smooth_store_filtered(s, k, 0, t, x, P);
    }
    double* sr = a.sq + (size_t)NS * n + t;      // the sums of the R update, and behind them the number of measurements they hold
    if (learn) {
#pragma unroll
        for (int e = 0; e < NS + 4; ++e) a.sq[(size_t)e * n + t] = 0.0;
    }
    // backward: (x, P) is the smoothed state of node k + 1 on entry of a step and of node k afterwards
    for (int k = len - 1; k >= 0; --k) {
        if (k < len - 1) {
            double xf[N], Pf[NS], xp[N], AP[N * N], U[NS], G[N * N];
            smooth_load_filtered(s, k, 0, t, xf, Pf);
#pragma unroll
            for (int e = 0; e < NS; ++e) m.Q[e] = q[(size_t)e * n];
            smooth_predict<N>(m, xf, Pf, xp, AP, U);
            smooth_backward_gain<N, true, true>(xf, Pf, xp, AP, U, x, P, G);
            if (learn) {
                MHT_EM_SCHED_FENCE();
                double x1[N], P1[NS], S[NS];
#pragma unroll
                for (int i = 0; i < N; ++i) x1[i] = a.pn[(size_t)(NS + i) * n + t];
#pragma unroll
                for (int e = 0; e < NS; ++e) P1[e] = a.pn[(size_t)e * n + t];
                smooth_em_q_term<N>(m, G, x1, P1, x, P, S);
#pragma unroll
                for (int e = 0; e < NS; ++e) a.sq[(size_t)e * n + t] += S[e];
            }
        }
        if (learn && k > 0) {
#pragma unroll
            for (int e = 0; e < NS; ++e) a.pn[(size_t)e * n + t] = P[e];
#pragma unroll
            for (int i = 0; i < N; ++i) a.pn[(size_t)(NS + i) * n + t] = x[i];
            if (s.has_z[(size_t)k * n + t]) {
                double SR[3];
                smooth_em_r_term<N>(m, s.z[((size_t)k * 2) * n + t], s.z[((size_t)k * 2 + 1) * n + t], x, P, SR);
#pragma unroll
                for (int e = 0; e < 3; ++e) sr[(size_t)e * n] += SR[e];
                sr[3 * n] += 1.0;
            }
        }
        if (LAST) {
#pragma unroll
            for (int i = 0; i < N; ++i) s.xs[((size_t)k * N + i) * n + t] = x[i];
            if (s.Ps) {
#pragma unroll
                for (int e = 0; e < NS; ++e) s.Ps[((size_t)k * NS + e) * n + t] = P[e];
            }
        }
    }
    // M-step: Q and R in place; x0 <- xs_0 and P0 <- Ps_0 are (x, P) as they stand
    if (learn) {
        const double steps_taken = (double)(len - 1);
#pragma unroll
        for (int e = 0; e < NS; ++e) q[(size_t)e * n] = a.sq[(size_t)e * n + t] / steps_taken;
        const double seen = sr[3 * n];
        if (seen > 0.0) {
#pragma unroll
            for (int e = 0; e < 3; ++e) r[(size_t)e * n] = sr[(size_t)e * n] / seen;
        }
    }
    if (!LAST) {
        double* th = a.theta + t;
#pragma unroll
        for (int i = 0; i < N; ++i) th[(size_t)i * n] = x[i];
#pragma unroll
        for (int e = 0; e < NS; ++e) th[(size_t)(N + e) * n] = P[e];
    }
}

// Track t: n_iter learning walks, then the walk that writes the output (a host caller's loop; on the device the launches are the loop)
template <int N>
MHT_HD void smooth_em_walk(const SmoothEmArgs<N>& a, int t, int n_iter) {
    for (int it = 0; it < n_iter; ++it) smooth_em_pass<N, false>(a, t, it == 0);
    smooth_em_pass<N, true>(a, t, n_iter == 0);
}

}  // namespace mht
