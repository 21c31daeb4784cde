// The normalised estimation error squared (NEES) of one state estimate against ground truth: e' P^-1 e with e = x - truth, the figure
// that says whether the covariance a filter reports is honest (Bar-Shalom, Li, Kirubarajan: Estimation with Applications to Tracking and
// Navigation, ch. 5.4) -- in the unmeasured states too, which the NIS and whiteness tests of the innovations cannot see
// (mht_nees_nodes, include/mht_amd.h).  The code a lane of the kernels of mht_nees.hip runs per cell, and tests/hostmath/nees_host.cpp on
// the CPU.
//
// One factorisation gives three figures.  With P = U' U (smooth_cholesky, mht_smooth_math.h: upper, packed) and U' y = e solved forward,
// e' P^-1 e = sum y_j^2; and the leading D x D block of U is the factor of the leading D x D block of P, so the sum over j < D is the
// NEES of the leading D components under their MARGINAL covariance, exactly.  Every model here orders its state [x, y, vx, vy, ...]:
//   nees2 = y_0^2 + y_1^2      position                2 degrees of freedom
//   nees4 = sum over j < 4     position and velocity   4
//   neesN = sum over j < N     the full state          N
// D, one of 2, 4, N, says how many leading components the truth carries: a figure that needs more is NaN.
//
// A cell's output is N + 3 doubles: e[0 .. N) (NaN at components >= D), nees2, nees4, neesN.  A pivot j of the factorisation that is not
// positive gives NaN in every figure that includes component j; the figures in front of it stay valid.  A cell that is absent, or whose
// x or P holds a NaN (the rows behind a track's end, as mht_filter_tracks* and mht_smooth_tracks* write them), is NaN throughout.
//
// Layouts are those the filter and smoother seams write, track-minor: x [L_max][N][n], P [L_max][N (N + 1) / 2][n], and with them
// truth [L_max][N][n] (components >= D are not read), present [L_max][n], out [L_max][N + 3][n].
#pragma once
#include "mht_smooth_math.h"

namespace mht {

struct NeesArgs {
    int32_t n, L_max, D;
    const double* x;          // [L_max][N][n]
    const double* P;          // [L_max][N(N+1)/2][n]
    const double* truth;      // [L_max][N][n]
    const uint8_t* present;   // [L_max][n]
    double* out;              // [L_max][N + 3][n]
};

// x [N], P [N (N + 1) / 2] packed, truth [N] (read below D only), out [N + 3]
template <int N>
MHT_HD void nees_eval(const double* x, const double* P, const double* truth, int D, double* out) {
    constexpr int NS = N * (N + 1) / 2;
    const double nan = __builtin_nan("");
    double e[N], U[NS], inv_d[N];
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = i < D ? x[i] - truth[i] : nan;
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = e[i];
#pragma unroll
    for (int c = 0; c < NS; ++c) U[c] = P[c];
    smooth_cholesky<N>(U, inv_d);
    double y[N], q = 0.0;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double s = e[j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = fma(-y[k], U[sym_idx(N, k, j)], s);
        y[j] = s * inv_d[j];
        q = fma(y[j], y[j], q);
        ok = ok && j < D && U[sym_idx(N, j, j)] > 0.0;      // (a pivot that is not positive left NaN or 0 here)
        if (j == 1) out[N] = ok ? q : nan;
        if (j == 3) out[N + 1] = ok ? q : nan;
        if (j == N - 1) out[N + 2] = ok ? q : nan;
    }
}

// Cell (k, t) of a batch: loaded, evaluated and stored, every one of its N + 3 outputs written
template <int N>
MHT_HD void nees_cell(const NeesArgs& a, int k, int t) {
    constexpr int NS = N * (N + 1) / 2;
    const size_t n = (size_t)a.n;
    double x[N], P[NS], truth[N], out[N + 3];
    bool there = a.present[(size_t)k * n + t] != 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        x[i] = a.x[((size_t)k * N + i) * n + t];
        there = there && x[i] == x[i];
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        P[c] = a.P[((size_t)k * NS + c) * n + t];
        there = there && P[c] == P[c];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) truth[i] = i < a.D ? a.truth[((size_t)k * N + i) * n + t] : 0.0;
    nees_eval<N>(x, P, truth, a.D, out);
    double* o = a.out + ((size_t)k * (N + 3)) * n + t;
#pragma unroll
    for (int i = 0; i < N + 3; ++i) o[(size_t)i * n] = there ? out[i] : __builtin_nan("");
}

}  // namespace mht
