// One track of the smoothers' models scored under ONE OF A GRID of candidate noise models: smooth_score_from (mht_smooth_score.h) with the
// step policy's Q and R replaced by candidate g's and nothing else -- A, C and the period stay the batch's, the start is the batch's
// (x_init, P_init).  The update and the advance are that header's functions as they are, so row g of the outputs holds the bits
// mht_score_tracks gives for a model that carries candidate g's matrices.  The code a lane of the kernels of mht_smooth_score_grid.hip
// runs, and tests/hostmath/smooth_score_grid_host.cpp per (track, candidate) on the CPU.
//
// The candidates are a table [G][NS + 3] of float64: Q's upper triangle packed in sym_idx order, then R00, R01, R11.  A walk reads row
// g of it; where g is the same for all lanes of a wavefront (the kernels: g = blockIdx.y) the row's address is wavefront-uniform and
// Q and R need no vector registers, unlike the per-track theta of smooth_score_walk_theta.
#pragma once
#include "mht_smooth_score.h"

namespace mht {

template <int N, typename Steps>
struct ScoreGridArgs {
    ScoreArgs<N, Steps> s;    // the batch; ll and nis are [G][n], nobs is [n] (written by candidate 0's walks only); theta, nis_ais, nais null
    const double* cand;       // [G][NS + 3] (in the workspace)
    int32_t n_cand;           // G
};

constexpr MHT_HD int smooth_score_grid_row(int nx) { return nx * (nx + 1) / 2 + 3; }      // doubles per candidate in the table

// Track t under candidate g, from (x_init, P_init)
template <int N, typename Steps>
MHT_HD void smooth_score_grid_walk(const ScoreGridArgs<N, Steps>& a, int t, int g) {
    constexpr int NS = N * (N + 1) / 2;
    const size_t n = (size_t)a.s.n;
    const double* c = a.cand + (size_t)g * (NS + 3);
    Steps steps = a.s.steps;
#pragma unroll
    for (int e = 0; e < NS; ++e) steps.model.Q[e] = c[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) steps.model.R[e] = c[NS + e];
    ScoreArgs<N, Steps> row = a.s;      // smooth_score_from writes element t of what it is handed: row g, and the counts once
    row.ll = a.s.ll + (size_t)g * n;
    row.nis = a.s.nis + (size_t)g * n;
    if (g != 0) row.nobs = nullptr;
    double x[N], P[NS];
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = a.s.x_init[(size_t)i * n + t];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) P[sym_idx(N, i, j)] = a.s.P_init[(size_t)(i * N + j) * n + t];
    smooth_score_from<N>(row, steps, t, x, P);
}

}  // namespace mht
