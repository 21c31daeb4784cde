// One track of the smoothers' models FILTERED: the forward loop of smooth_walk (mht_smooth_walk.h) under the same step policies, with the
// filtered state and covariance of every node -- what the smoothers keep in a private workspace and the score and trace walks discard --
// handed out (mht_filter_tracks, include/mht_amd.h).  What a comparison of the reported covariance with ground truth needs
// (mht_nees.h).  The code a lane of the kernels of mht_smooth_filter.hip runs, and tests/hostmath/filter_host.cpp per track on the CPU.
//
// Outputs are track-minor like everything a walk touches: xf [L_max][N][n], Pf [L_max][N (N + 1) / 2][n] packed (sym_idx) -- the layout
// mht_smooth_tracks* writes xs and Ps in.  Node 0 is the initial state (x_init, P_init); node k >= 1 is the state behind the advance and,
// with a plot, the radar update: at the scan's time.  The rows len[t] <= k < L_max behind a track's end are written too, with a quiet
// NaN: a lane writes all L_max rows of its track, the caller may hand in uninitialised memory.
//
// Nothing is restated: the steps are steps.advance and smooth_update<N>, called as smooth_walk calls them, so the filtered states are
// the smoother's own bits -- the last node of a track, whose filtered state is its smoothed state, equals xs and Ps of
// mht_smooth_tracks* there.  The AIS policy stores the filtered state at a message's time into slot 1 of the smoother's workspace
// (AisSteps::advance); a filter walk has no such slot and nothing reads it back: smooth_store_filtered is overloaded for FilterArgs, and
// slot 1 is a store that does not happen.
#pragma once
#include "mht_smooth_walk.h"

namespace mht {

template <int N, typename Steps>
struct FilterArgs {
    Steps steps;
    int32_t n, L_max;
    const int32_t* len;       // [n] (in the workspace)
    const double* x_init;     // [N][n]
    const double* P_init;     // [N*N][n]
    const double* z;          // [L_max][2][n]
    const uint8_t* has_z;     // [L_max][n]
    double* xf;               // [L_max][N][n]
    double* Pf;               // [L_max][N(N+1)/2][n]
};

// Track t's mean and packed covariance of node k: slot 0, the state at the scan's time, goes to the outputs; any other slot is its
// policy's own and has no place here
template <int N, typename Steps>
MHT_HD void smooth_store_filtered(const FilterArgs<N, Steps>& a, int k, int slot, int t, const double* x, const double* P) {
    constexpr int NS = N * (N + 1) / 2;
    if (slot != 0) return;
    const size_t n = (size_t)a.n;
#pragma unroll
    for (int i = 0; i < N; ++i) a.xf[((size_t)k * N + i) * n + t] = x[i];
#pragma unroll
    for (int e = 0; e < NS; ++e) a.Pf[((size_t)k * NS + e) * n + t] = P[e];
}

// Track t under the batch's model, from (x_init, P_init): the forward loop of smooth_walk, every row of the track written
template <int N, typename Steps>
MHT_HD void smooth_filter_walk(const FilterArgs<N, Steps>& a, int t) {
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
    for (int k = 0; k < len; ++k) {
        if (k > 0) {
            a.steps.advance(a, k, t, x, P);
            if (a.has_z[(size_t)k * n + t]) smooth_update<N>(a.steps.model, a.z[((size_t)k * 2) * n + t], a.z[((size_t)k * 2 + 1) * n + t], x, P);
        }
        smooth_store_filtered(a, k, 0, t, x, P);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = __builtin_nan("");
#pragma unroll
    for (int e = 0; e < NS; ++e) P[e] = __builtin_nan("");
    for (int k = len; k < a.L_max; ++k) smooth_store_filtered(a, k, 0, t, x, P);
}

}  // namespace mht
