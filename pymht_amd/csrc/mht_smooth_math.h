// Per-track arithmetic of the fixed-interval Rauch-Tung-Striebel smoother (mht_smooth_tracks, include/mht_amd.h), float64 throughout.
//
// NOT a restatement of reference code: the reference hands its track histories to pykalman (pyTarget.py:580-609), whose EM step is not
// reproducible; this is the textbook recursion with the tracker's own model, and its operation order is its own (no bit-exact target).
// What it is held to is accuracy: the worst error against an 80-bit evaluation of the same recursion stays within a small factor of a
// float64 NumPy evaluation's (tests/test_smooth_gpu.py).
//
// Everything is written for one track per lane: N is a template parameter, every loop is fully unrolled and every array statically indexed,
// so the matrices live in registers.  Covariances are SYMMETRIC PACKED (upper triangle, row-major: N (N + 1) / 2 entries -- 10 at four
// states, 21 at six): half the registers and half the workspace of full matrices, and a result that is symmetric by construction.
// Every multiply-add is an explicit fma (the library is compiled with -ffp-contract=off).
#pragma once
#include "mht_math.h"

namespace mht {

template <int N>
struct SmoothModel {        // the linear-Gaussian model in float64 (mht_model_x's float32 matrices, widened: exact)
    double A[N * N];        // row-major
    double Q[N * (N + 1) / 2];  // symmetric packed
    double C[2 * N];        // 2 x N row-major
    double R[3];            // r00, r01, r11
};

constexpr MHT_HD int sym_idx(int n, int i, int j) {      // packed index of entry (i, j) of a symmetric n x n matrix
    return i <= j ? i * n - i * (i - 1) / 2 + (j - i) : j * n - j * (j - 1) / 2 + (i - j);
}

// xp = A xf;  AP = A Pf (full, row-major);  Pp = AP A' + Q (packed)
template <int N>
MHT_HD void smooth_predict(const SmoothModel<N>& m, const double* xf, const double* Pf, double* xp, double* AP, double* Pp) {
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
            double acc = m.Q[sym_idx(N, i, j)];
#pragma unroll
            for (int k = 0; k < N; ++k) acc = fma(AP[i * N + k], m.A[j * N + k], acc);
            Pp[sym_idx(N, i, j)] = acc;
        }
}

// Measurement update of (x, P) in place with z:  S = C P C' + R (2 x 2, inverted in closed form), K = P C' S^-1,
// x += K (z - C x), P -= K (C P).  M: anything with C [2 N] and R [3] (SmoothModel<N>, or the constant-turn smoother's SmoothCtModel)
template <int N, typename M>
MHT_HD void smooth_update(const M& m, double z0, double z1, double* x, double* P) {
    double CP[2 * N];      // C P, 2 x N; (P C')' by symmetry
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double acc = m.C[a * N] * P[sym_idx(N, 0, j)];
#pragma unroll
            for (int k = 1; k < N; ++k) acc = fma(m.C[a * N + k], P[sym_idx(N, k, j)], acc);
            CP[a * N + j] = acc;
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
    double K[2 * N];      // N x 2
#pragma unroll
    for (int i = 0; i < N; ++i) {
        K[2 * i] = fma(CP[N + i], i01, CP[i] * i00);
        K[2 * i + 1] = fma(CP[N + i], i11, CP[i] * i01);
    }
    double r0 = z0, r1 = z1;      // innovation z - C x
#pragma unroll
    for (int k = 0; k < N; ++k) {
        r0 = fma(-m.C[k], x[k], r0);
        r1 = fma(-m.C[N + k], x[k], r1);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = fma(K[2 * i + 1], r1, fma(K[2 * i], r0, x[i]));
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j)
            P[sym_idx(N, i, j)] = fma(-K[2 * i + 1], CP[N + j], fma(-K[2 * i], CP[j], P[sym_idx(N, i, j)]));
}

// Cholesky factor of the symmetric positive definite packed P, in place: afterwards P holds U with P = U' U (upper, packed), and
// inv_d[i] = 1 / U_ii.  No pivoting: a predicted covariance A Pf A' + Q is positive definite.
template <int N>
MHT_HD void smooth_cholesky(double* P, double* inv_d) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double d = P[sym_idx(N, i, i)];
#pragma unroll
        for (int k = 0; k < i; ++k) d = fma(-P[sym_idx(N, k, i)], P[sym_idx(N, k, i)], d);
        d = sqrt(d);
        P[sym_idx(N, i, i)] = d;
        inv_d[i] = 1.0 / d;
#pragma unroll
        for (int j = i + 1; j < N; ++j) {
            double s = P[sym_idx(N, i, j)];
#pragma unroll
            for (int k = 0; k < i; ++k) s = fma(-P[sym_idx(N, k, i)], P[sym_idx(N, k, j)], s);
            P[sym_idx(N, i, j)] = s / d;
        }
    }
}

// The part of a backward step behind the prediction, whatever made it.  In: the filtered (xf, Pf) of node k, the prediction of node
// k + 1 from it (xp, AP = A Pf, U = Pp: destroyed), the smoothed (xs, Ps) of node k + 1.  Out, in place: (xs, Ps) of node k.
//   G = Pf A' Pp^-1 applied through Pp = U' U: row i of G solves g U' U = row i of Pf A' = column i of A Pf.
//   xs_k = xf + G (xs_{k+1} - xp),  Ps_k = Pf + G (Ps_{k+1} - Pp) G'.   COV = false: means only, Ps is not touched.
// GAIN = true: G [N][N] row-major is also handed out (the EM walk, mht_smooth_em.h, takes its lag-one covariance from it).
template <int N, bool COV, bool GAIN = false>
MHT_HD void smooth_backward_gain(const double* xf, const double* Pf, const double* xp, const double* AP, double* U, double* xs, double* Ps,
                                 double* G_out = nullptr) {
    constexpr int NS = N * (N + 1) / 2;
    double inv_d[N];
    double D[COV ? NS : 1];      // Ps_{k+1} - Pp
    if (COV) {
#pragma unroll
        for (int e = 0; e < NS; ++e) D[e] = Ps[e] - U[e];
    }
    smooth_cholesky<N>(U, inv_d);
    double G[N * N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double y[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {      // y U = b (forward: U' is lower), b_j = AP[j][i]
            double s = AP[j * N + i];
#pragma unroll
            for (int k = 0; k < j; ++k) s = fma(-y[k], U[sym_idx(N, k, j)], s);
            y[j] = s * inv_d[j];
        }
#pragma unroll
        for (int j = N - 1; j >= 0; --j) {      // g U' = y (backward)
            double s = y[j];
#pragma unroll
            for (int k = j + 1; k < N; ++k) s = fma(-G[i * N + k], U[sym_idx(N, j, k)], s);
            G[i * N + j] = s * inv_d[j];
        }
    }
    double dx[N];
#pragma unroll
    for (int j = 0; j < N; ++j) dx[j] = xs[j] - xp[j];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double acc = xf[i];
#pragma unroll
        for (int j = 0; j < N; ++j) acc = fma(G[i * N + j], dx[j], acc);
        xs[i] = acc;
    }
    if (COV) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double GD[N];      // row i of G D
#pragma unroll
            for (int j = 0; j < N; ++j) {
                double acc = G[i * N] * D[sym_idx(N, 0, j)];
#pragma unroll
                for (int k = 1; k < N; ++k) acc = fma(G[i * N + k], D[sym_idx(N, k, j)], acc);
                GD[j] = acc;
            }
#pragma unroll
            for (int j = i; j < N; ++j) {
                double acc = Pf[sym_idx(N, i, j)];
#pragma unroll
                for (int k = 0; k < N; ++k) acc = fma(GD[k], G[j * N + k], acc);
                Ps[sym_idx(N, i, j)] = acc;
            }
        }
    }
    if (GAIN) {
#pragma unroll
        for (int i = 0; i < N * N; ++i) G_out[i] = G[i];
    }
}

// One backward step of the linear model: Pp = A Pf A' + Q is recomputed here (the forward pass keeps xf and Pf only).
template <int N, bool COV>
MHT_HD void smooth_backward(const SmoothModel<N>& m, const double* xf, const double* Pf, double* xs, double* Ps) {
    double xp[N], AP[N * N], U[N * (N + 1) / 2];
    smooth_predict<N>(m, xf, Pf, xp, AP, U);
    smooth_backward_gain<N, COV>(xf, Pf, xp, AP, U, xs, Ps);
}

}  // namespace mht
