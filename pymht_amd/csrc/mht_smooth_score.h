// One track of the smoothers' models SCORED: the forward (filter) half of smooth_walk (mht_smooth_walk.h) under the same step policies,
// with nothing stored per node -- no workspace slot, no xs, no Ps -- and per track the sums that say how well the model explains the
// plots it is given (mht_score_tracks, include/mht_amd.h).  The code a lane of the kernels of mht_smooth_score.hip runs, and
// tests/hostmath/smooth_score_host.cpp per track on the CPU.
//
// Node 0 is the initial state and contributes nothing, as in the smoothers (pykalman's loglikelihood() counts an observation at time 0:
// these are not its figures).  For every node k >= 1 with a radar plot z_k, with v = z_k - C xp_k and S = C Pp_k C' + R at the
// prediction (xp_k, Pp_k) of the node:
//   nis  += v' S^-1 v                                    the normalised innovation squared: chi-square with 2 nObs degrees of freedom
//   ll   -= 1/2 (ln det S + v' S^-1 v + 2 ln 2 pi)       ln N(z_k; C xp_k, S)                          over a consistent filter
//   nObs += 1
// and for a node that took an AIS message m (kind >= 2; AIS model only), at the message's time, with v = m - xp(t_m), S = Pp(t_m) + r I4:
//   nisAis += v' S^-1 v
//   ll     -= 1/2 (ln det S + v' S^-1 v + 4 ln 2 pi),    ln det S = 2 sum ln U_ii of the Cholesky factor S = U' U the update takes anyway
//   nAis   += 1
// nis and nObs stay radar-only.  A track of one node, or one never detected, gives exactly ll = 0.0, nis = 0.0, nObs = 0.  A det S
// that is not positive (a model that is no covariance) gives NaN in the floating-point outputs of that track, and of no other.
//
// The state updates are smooth_update's and smooth_ais_update's operations in their order, restated here with the innovation and S
// handed out (the functions the smoother kernels inline are left as they are: those kernels keep their registers): the filtered states
// behind a score are the smoother's own.
#pragma once
#include "mht_smooth_walk.h"

namespace mht {

constexpr double SMOOTH_SCORE_LN_2PI = 1.8378770664093454835606594728112;

template <int N, typename Steps>
struct ScoreArgs {
    Steps steps;
    int32_t n, L_max;
    const int32_t* len;       // [n] (in the workspace)
    const double* x_init;     // [N][n]
    const double* P_init;     // [N*N][n]
    const double* z;          // [L_max][2][n]
    const uint8_t* has_z;     // [L_max][n]
    const double* theta;      // null, or [N + 2 NS + 3][n]: x0, P0 (packed), Q (packed), R per track (smooth_score_walk_theta)
    double* ll;               // [n]
    double* nis;              // [n] or null
    int32_t* nobs;            // [n] or null
    double* nis_ais;          // [n] or null (AIS model)
    int32_t* nais;            // [n] or null (AIS model)
};

struct ScoreSums {
    double ll = 0.0, nis = 0.0, nis_ais = 0.0;
    double poison = 0.0;      // NaN once a det S was not positive; added to the sums at the end (0.0 leaves them as they are)
    int32_t nobs = 0, nais = 0;
};

// smooth_update (mht_smooth_math.h), operation for operation, and the node's terms into the sums
template <int N, typename M>
MHT_HD void smooth_score_update(const M& m, double z0, double z1, double* x, double* P, ScoreSums& acc) {
    double CP[2 * N];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double s = m.C[a * N] * P[sym_idx(N, 0, j)];
#pragma unroll
            for (int k = 1; k < N; ++k) s = fma(m.C[a * N + k], P[sym_idx(N, k, j)], s);
            CP[a * N + j] = s;
        }
    double s00 = m.R[0], s01 = m.R[1], s11 = m.R[2];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        s00 = fma(CP[k], m.C[k], s00);
        s01 = fma(CP[k], m.C[N + k], s01);
        s11 = fma(CP[N + k], m.C[N + k], s11);
    }
    const double det = fma(s00, s11, -(s01 * s01));
    const double i00 = s11 / det, i01 = -s01 / det, i11 = s00 / det;
    double K[2 * N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        K[2 * i] = fma(CP[N + i], i01, CP[i] * i00);
        K[2 * i + 1] = fma(CP[N + i], i11, CP[i] * i01);
    }
    double r0 = z0, r1 = z1;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        r0 = fma(-m.C[k], x[k], r0);
        r1 = fma(-m.C[N + k], x[k], r1);
    }
    // the score's own: v' S^-1 v and ln det S
    const double q = fma(r1, fma(i11, r1, i01 * r0), r0 * fma(i01, r1, i00 * r0));
    if (det > 0.0) {
        acc.nis += q;
        acc.ll -= fma(0.5, log(det) + q, SMOOTH_SCORE_LN_2PI);
    } else {
        acc.poison = __builtin_nan("");
    }
    acc.nobs += 1;
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = fma(K[2 * i + 1], r1, fma(K[2 * i], r0, x[i]));
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j)
            P[sym_idx(N, i, j)] = fma(-K[2 * i + 1], CP[N + j], fma(-K[2 * i], CP[j], P[sym_idx(N, i, j)]));
}

// smooth_ais_update (mht_smooth_ais_math.h), operation for operation, and the message's terms into the sums:
// v' S^-1 v = |y|^2 with y U = v through the factor S = U' U
MHT_HD void smooth_score_ais_update(const double* m, double r, double* x, double* P, ScoreSums& acc) {
    double U[10], inv_d[4];
#pragma unroll
    for (int e = 0; e < 10; ++e) U[e] = P[e];
#pragma unroll
    for (int i = 0; i < 4; ++i) U[sym_idx(4, i, i)] = P[sym_idx(4, i, i)] + r;
    smooth_cholesky<4>(U, inv_d);
    double K[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = P[sym_idx(4, i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s = fma(-y[k], U[sym_idx(4, k, j)], s);
            y[j] = s * inv_d[j];
        }
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            double s = y[j];
#pragma unroll
            for (int k = j + 1; k < 4; ++k) s = fma(-K[i * 4 + k], U[sym_idx(4, j, k)], s);
            K[i * 4 + j] = s * inv_d[j];
        }
    }
    double d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = m[j] - x[j];
    {      // the score's own
        double y[4], q = 0.0, ld = 0.0;
        bool pd = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = d[j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = fma(-y[k], U[sym_idx(4, k, j)], s);
            y[j] = s * inv_d[j];
            q = fma(y[j], y[j], q);
            ld += log(U[sym_idx(4, j, j)]);
            pd = pd && U[sym_idx(4, j, j)] > 0.0;      // (a pivot that is not positive left NaN or 0 here)
        }
        if (pd) {
            acc.nis_ais += q;
            acc.ll -= fma(0.5, 2.0 * ld + q, 2.0 * SMOOTH_SCORE_LN_2PI);
        } else {
            acc.poison = __builtin_nan("");
        }
        acc.nais += 1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double s = x[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fma(K[i * 4 + j], d[j], s);
        x[i] = s;
    }
    double Pn[10];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            double s = P[sym_idx(4, i, j)];
#pragma unroll
            for (int k = 0; k < 4; ++k) s = fma(-K[i * 4 + k], P[sym_idx(4, k, j)], s);
            Pn[sym_idx(4, i, j)] = s;
        }
#pragma unroll
    for (int e = 0; e < 10; ++e) P[e] = Pn[e];
}

// smooth_ais_forward with the scoring update; the filtered state at the message's time is not handed out (nothing walks back)
MHT_HD void smooth_score_ais_forward(const double* entry, const double* m, double r, double* x, double* P, ScoreSums& acc) {
    SmoothModel<4> lg;
    double AP[16], xm[4], Pm[10];
    smooth_ais_leg<0>(entry, lg);
    smooth_predict<4>(lg, x, P, xm, AP, Pm);
    smooth_score_ais_update(m, r, xm, Pm, acc);
    smooth_ais_leg<1>(entry, lg);
    smooth_predict<4>(lg, xm, Pm, x, AP, P);
}

// (x, P) from the filtered state of node k - 1 to the prediction of node k: the policy's own advance where it stores nothing ...
template <int N, typename Args>
MHT_HD void smooth_score_advance(const LinearSteps<N>& s, const Args& a, int k, int t, double* x, double* P, ScoreSums&) {
    s.advance(a, k, t, x, P);
}
template <typename Args>
MHT_HD void smooth_score_advance(const ConstantTurnSteps& s, const Args& a, int k, int t, double* x, double* P, ScoreSums&) {
    s.advance(a, k, t, x, P);
}
// ... and AisSteps::advance without its store, with the message scored
template <typename Args>
MHT_HD void smooth_score_advance(const AisSteps& s, const Args& a, int k, int t, double* x, double* P, ScoreSums& acc) {
    const size_t n = (size_t)a.n;
    if (s.kind[(size_t)k * n + t] >= 2) {
        const double* entry = s.legs + (size_t)s.leg[(size_t)k * n + t] * SMOOTH_AIS_LEG_DOUBLES;
        double m[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) m[i] = s.ais_z[((size_t)k * 4 + i) * n + t];
        smooth_score_ais_forward(entry, m, s.ais_r[(size_t)k * n + t], x, P, acc);
    } else {
        smooth_advance<4>(s.model, x, P);
    }
}

// Track t from (x, P) under `steps`, and its sums out
template <int N, typename Steps>
MHT_HD void smooth_score_from(const ScoreArgs<N, Steps>& a, const Steps& steps, int t, double* x, double* P) {
    const size_t n = (size_t)a.n;
    const int len = a.len[t];      // 1 <= len <= L_max: checked by the host before the launch
    ScoreSums acc;
    for (int k = 1; k < len; ++k) {
        smooth_score_advance(steps, a, k, t, x, P, acc);
        if (a.has_z[(size_t)k * n + t]) smooth_score_update<N>(steps.model, a.z[((size_t)k * 2) * n + t], a.z[((size_t)k * 2 + 1) * n + t], x, P, acc);
    }
    a.ll[t] = acc.ll + acc.poison;
    if (a.nis) a.nis[t] = acc.nis + acc.poison;
    if (a.nobs) a.nobs[t] = acc.nobs;
    if (a.nis_ais) a.nis_ais[t] = acc.nis_ais + acc.poison;
    if (a.nais) a.nais[t] = acc.nais;
}

// Track t under the batch's model, from (x_init, P_init)
template <int N, typename Steps>
MHT_HD void smooth_score_walk(const ScoreArgs<N, Steps>& a, int t) {
    constexpr int NS = N * (N + 1) / 2;
    const size_t n = (size_t)a.n;
    double x[N], P[NS];
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = a.x_init[(size_t)i * n + t];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) P[sym_idx(N, i, j)] = a.P_init[(size_t)(i * N + j) * n + t];
    smooth_score_from<N>(a, a.steps, t, x, P);
}

// Track t of the linear model under ITS OWN theta = (x0, P0, Q, R), read from the EM workspace's layout (mht_smooth_em.h); A and C stay
// the batch's
template <int N>
MHT_HD void smooth_score_walk_theta(const ScoreArgs<N, LinearSteps<N>>& a, int t) {
    constexpr int NS = N * (N + 1) / 2;
    const size_t n = (size_t)a.n;
    const double* th = a.theta + t;
    LinearSteps<N> steps = a.steps;
    double x[N], P[NS];
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = th[(size_t)i * n];
#pragma unroll
    for (int e = 0; e < NS; ++e) P[e] = th[(size_t)(N + e) * n];
#pragma unroll
    for (int e = 0; e < NS; ++e) steps.model.Q[e] = th[(size_t)(N + NS + e) * n];
#pragma unroll
    for (int e = 0; e < 3; ++e) steps.model.R[e] = th[(size_t)(N + 2 * NS + e) * n];
    smooth_score_from<N>(a, steps, t, x, P);
}

}  // namespace mht
