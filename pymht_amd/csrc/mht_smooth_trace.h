// One track of the smoothers' models TRACED: the score walk (mht_smooth_score.h) under the same step policies, with the innovation
// sequence the score sums up and discards handed out per node -- what the filter-consistency checks of the tracking literature need
// (NIS inside its chi-square interval over time, whiteness of the innovations), and what says WHERE a model stops fitting a track
// (mht_trace_tracks, include/mht_amd.h).  The code a lane of the kernels of mht_smooth_trace.hip runs, and
// tests/hostmath/smooth_trace_host.cpp per track on the CPU.
//
// Outputs are track-minor like everything a walk touches, out[(k * E + e) * n + t]: the stores of a wavefront are contiguous.
//   radar [L_max][TRACE_RADAR_DOUBLES][n], at every node k >= 1 with a radar plot z_k, at the prediction (xp_k, Pp_k) of the node:
//     0, 1      v = z_k - C xp_k
//     2, 3, 4   S00, S01, S11 of S = C Pp_k C' + R
//     5         nis_k = v' S^-1 v
//     6         ll_k = -1/2 (ln det S + nis_k + 2 ln 2 pi): the term the score walk subtracts, negated
//   ais [L_max][TRACE_AIS_DOUBLES][n] (AIS model only), at every node that took a message m (kind >= 2), at the message's time:
//     0 .. 3    v = m - xp(t_m)
//     4 .. 13   the upper triangle of S = Pp(t_m) + r I4, packed (sym_idx), as it is before its factorisation
//     14        nisAis_k = v' S^-1 v
//     15        llAis_k = -1/2 (ln det S + nisAis_k + 4 ln 2 pi)
// EVERY other cell of both arrays is written too, with a quiet NaN: node 0 (the initial state, no observation), a node without a plot
// or without a message, and the rows len[t] <= k < L_max behind a track's end.  A lane writes all L_max rows of its track: the caller
// may hand in uninitialised memory.  A det S that is not positive (a pivot, for a message) leaves v and S as computed and gives NaN in
// that node's nis and ll; the state update goes on with whatever it yields, as in the score walk, and no other track is touched.
//
// The state updates are smooth_score_update's and smooth_score_ais_update's operations -- smooth_update's and smooth_ais_update's --
// restated with the node's figures stored instead of summed (the functions the score kernels inline are left as they are: those
// kernels keep their registers).  What does not depend on the gain is computed and stored in front of it; no operation's operands
// change, so the filtered states behind a trace are the score's own bits, and a track's ll_k and nis_k added up in node order
// (llAis_k in front of ll_k at a node that has both) are the score's sums, bit for bit.
#pragma once
#include "mht_smooth_score.h"

namespace mht {

constexpr int TRACE_RADAR_DOUBLES = 7;
constexpr int TRACE_AIS_DOUBLES = 16;

template <int N, typename Steps>
struct TraceArgs {
    Steps steps;
    int32_t n, L_max;
    const int32_t* len;       // [n] (in the workspace)
    const double* x_init;     // [N][n]
    const double* P_init;     // [N*N][n]
    const double* z;          // [L_max][2][n]
    const uint8_t* has_z;     // [L_max][n]
    double* radar;            // [L_max][TRACE_RADAR_DOUBLES][n]
    double* ais;              // [L_max][TRACE_AIS_DOUBLES][n] (AIS model), else null
};

// E cells of track t at node k, all NaN
template <int E>
MHT_HD void smooth_trace_blank(double* out, int k, int t, size_t n) {
    double* o = out + ((size_t)k * E) * n + t;
#pragma unroll
    for (int e = 0; e < E; ++e) o[(size_t)e * n] = __builtin_nan("");
}

// smooth_score_update, operation for operation, with the node's figures to o[e * n], e < TRACE_RADAR_DOUBLES
template <int N, typename M>
MHT_HD void smooth_trace_update(const M& m, double z0, double z1, double* x, double* P, double* o, size_t n) {
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
    double r0 = z0, r1 = z1;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        r0 = fma(-m.C[k], x[k], r0);
        r1 = fma(-m.C[N + k], x[k], r1);
    }
    o[0] = r0; o[n] = r1;
    o[2 * n] = s00; o[3 * n] = s01; o[4 * n] = s11;
    const double det = fma(s00, s11, -(s01 * s01));
    const double i00 = s11 / det, i01 = -s01 / det, i11 = s00 / det;
    const double q = fma(r1, fma(i11, r1, i01 * r0), r0 * fma(i01, r1, i00 * r0));
    const bool pd = det > 0.0;
    o[5 * n] = pd ? q : __builtin_nan("");
    o[6 * n] = pd ? -fma(0.5, log(det) + q, SMOOTH_SCORE_LN_2PI) : __builtin_nan("");
    double K[2 * N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        K[2 * i] = fma(CP[N + i], i01, CP[i] * i00);
        K[2 * i + 1] = fma(CP[N + i], i11, CP[i] * i01);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = fma(K[2 * i + 1], r1, fma(K[2 * i], r0, x[i]));
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j)
            P[sym_idx(N, i, j)] = fma(-K[2 * i + 1], CP[N + j], fma(-K[2 * i], CP[j], P[sym_idx(N, i, j)]));
}

// smooth_score_ais_update, operation for operation, with the message's figures to o[e * n], e < TRACE_AIS_DOUBLES
MHT_HD void smooth_trace_ais_update(const double* m, double r, double* x, double* P, double* o, size_t n) {
    double U[10], inv_d[4];
#pragma unroll
    for (int e = 0; e < 10; ++e) U[e] = P[e];
#pragma unroll
    for (int i = 0; i < 4; ++i) U[sym_idx(4, i, i)] = P[sym_idx(4, i, i)] + r;
    double d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = m[j] - x[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[(size_t)j * n] = d[j];
#pragma unroll
    for (int e = 0; e < 10; ++e) o[(size_t)(4 + e) * n] = U[e];      // (S itself: the factor overwrites it below)
    smooth_cholesky<4>(U, inv_d);
    {
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
        o[(size_t)14 * n] = pd ? q : __builtin_nan("");
        o[(size_t)15 * n] = pd ? -fma(0.5, 2.0 * ld + q, 2.0 * SMOOTH_SCORE_LN_2PI) : __builtin_nan("");
    }
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

// smooth_score_ais_forward with the tracing update
MHT_HD void smooth_trace_ais_forward(const double* entry, const double* m, double r, double* x, double* P, double* o, size_t n) {
    SmoothModel<4> lg;
    double AP[16], xm[4], Pm[10];
    smooth_ais_leg<0>(entry, lg);
    smooth_predict<4>(lg, x, P, xm, AP, Pm);
    smooth_trace_ais_update(m, r, xm, Pm, o, n);
    smooth_ais_leg<1>(entry, lg);
    smooth_predict<4>(lg, xm, Pm, x, AP, P);
}

// (x, P) from the filtered state of node k - 1 to the prediction of node k, and node k's row of the AIS array where the model has one
template <int N, typename Args>
MHT_HD void smooth_trace_advance(const LinearSteps<N>& s, const Args& a, int k, int t, double* x, double* P) {
    s.advance(a, k, t, x, P);
}
template <typename Args>
MHT_HD void smooth_trace_advance(const ConstantTurnSteps& s, const Args& a, int k, int t, double* x, double* P) {
    s.advance(a, k, t, x, P);
}
template <typename Args>
MHT_HD void smooth_trace_advance(const AisSteps& s, const Args& a, int k, int t, double* x, double* P) {
    const size_t n = (size_t)a.n;
    if (s.kind[(size_t)k * n + t] >= 2) {
        const double* entry = s.legs + (size_t)s.leg[(size_t)k * n + t] * SMOOTH_AIS_LEG_DOUBLES;
        double m[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) m[i] = s.ais_z[((size_t)k * 4 + i) * n + t];
        smooth_trace_ais_forward(entry, m, s.ais_r[(size_t)k * n + t], x, P, a.ais + ((size_t)k * TRACE_AIS_DOUBLES) * n + t, n);
    } else {
        smooth_advance<4>(s.model, x, P);
        smooth_trace_blank<TRACE_AIS_DOUBLES>(a.ais, k, t, n);
    }
}

// Node k of track t takes no step (node 0, or behind the track's end): its rows are NaN
template <typename Steps, typename Args>
MHT_HD void smooth_trace_skip(const Steps&, const Args& a, int k, int t) {
    smooth_trace_blank<TRACE_RADAR_DOUBLES>(a.radar, k, t, (size_t)a.n);
}
template <typename Args>
MHT_HD void smooth_trace_skip(const AisSteps&, const Args& a, int k, int t) {
    smooth_trace_blank<TRACE_RADAR_DOUBLES>(a.radar, k, t, (size_t)a.n);
    smooth_trace_blank<TRACE_AIS_DOUBLES>(a.ais, k, t, (size_t)a.n);
}

// Track t under the batch's model, from (x_init, P_init): the loop of smooth_score_from, every row of the track written
template <int N, typename Steps>
MHT_HD void smooth_trace_walk(const TraceArgs<N, Steps>& a, int t) {
    constexpr int NS = N * (N + 1) / 2;
    const size_t n = (size_t)a.n;
    const int len = a.len[t];      // 1 <= len <= L_max: checked by the host before the launch
    double x[N], P[NS];
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = a.x_init[(size_t)i * n + t];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) P[sym_idx(N, i, j)] = a.P_init[(size_t)(i * N + j) * n + t];
    smooth_trace_skip(a.steps, a, 0, t);
    for (int k = 1; k < len; ++k) {
        smooth_trace_advance(a.steps, a, k, t, x, P);
        if (a.has_z[(size_t)k * n + t])
            smooth_trace_update<N>(a.steps.model, a.z[((size_t)k * 2) * n + t], a.z[((size_t)k * 2 + 1) * n + t], x, P,
                                   a.radar + ((size_t)k * TRACE_RADAR_DOUBLES) * n + t, n);
        else
            smooth_trace_blank<TRACE_RADAR_DOUBLES>(a.radar, k, t, n);
    }
    for (int k = len; k < a.L_max; ++k) smooth_trace_skip(a.steps, a, k, t);
}

}  // namespace mht
