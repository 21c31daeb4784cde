// One track of the Rauch-Tung-Striebel smoothers walked forward (filter) and backward (smoother): the loop the three kernels of
// mht_smooth.hip run per lane, and tests/hostmath/smooth_host.cpp runs per track on the CPU -- the same code, not a copy of it.
// The arithmetic is mht_smooth_math.h, mht_smooth_ct_math.h and mht_smooth_ais_math.h; mht_smooth.hip says why a track is a lane.
//
// Everything a walk touches in memory is track-minor, [node][element][track], and smooth_walk takes its track index t as an argument:
// a kernel passes its lane's, a host caller n = 1 and t = 0, where the layout is plain [node][element].
//
// What differs between the models is a step policy.  It holds what its steps read per batch (the model, and for the AIS model the
// per-node message arrays and the leg table), says how many filtered SLOTS a node has in the workspace, and makes the two steps:
//   advance   (x, P) from the filtered state of node k - 1 to the prediction of node k, in front of the radar update
//   backward  (x, P) from the smoothed state of node k + 1 to that of node k, given node k's filtered (xf, Pf)
// Slot 0 of a node is the walk's: the filtered state at the scan's time.  A further slot is its policy's.
#pragma once
#include "mht_smooth_ais_math.h"
#include "mht_smooth_ct_math.h"

namespace mht {

template <int N, typename Steps>
struct SmoothArgs {
    Steps steps;
    int32_t n, L_max;
    const int32_t* len;       // [n] (in the workspace)
    const double* x_init;     // [N][n]
    const double* P_init;     // [N*N][n]
    const double* z;          // [L_max][2][n]
    const uint8_t* has_z;     // [L_max][n]
    double* xs;               // [L_max][N][n]
    double* Ps;               // [L_max][N(N+1)/2][n] or null
    double* xf;               // workspace [L_max][SLOTS][N][n]
    double* Pf;               // workspace [L_max][SLOTS][N(N+1)/2][n]
};

// Track t's mean and packed covariance in filtered slot `slot` of node k
template <int N, typename Steps>
MHT_HD void smooth_store_filtered(const SmoothArgs<N, Steps>& a, int k, int slot, int t, const double* x, const double* P) {
    constexpr int NS = N * (N + 1) / 2;
    const size_t n = (size_t)a.n, at = (size_t)k * Steps::SLOTS + slot;
#pragma unroll
    for (int i = 0; i < N; ++i) a.xf[(at * N + i) * n + t] = x[i];
#pragma unroll
    for (int e = 0; e < NS; ++e) a.Pf[(at * NS + e) * n + t] = P[e];
}

template <int N, typename Steps>
MHT_HD void smooth_load_filtered(const SmoothArgs<N, Steps>& a, int k, int slot, int t, double* x, double* P) {
    constexpr int NS = N * (N + 1) / 2;
    const size_t n = (size_t)a.n, at = (size_t)k * Steps::SLOTS + slot;
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = a.xf[(at * N + i) * n + t];
#pragma unroll
    for (int e = 0; e < NS; ++e) P[e] = a.Pf[(at * NS + e) * n + t];
}

// The linear model's advance: (x, P) <- (A x, A P A' + Q)
template <int N>
MHT_HD void smooth_advance(const SmoothModel<N>& m, double* x, double* P) {
    constexpr int NS = N * (N + 1) / 2;
    double xp[N], AP[N * N], Pp[NS];
    smooth_predict<N>(m, x, P, xp, AP, Pp);
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = xp[i];
#pragma unroll
    for (int e = 0; e < NS; ++e) P[e] = Pp[e];
}

template <int N>
struct LinearSteps {
    static constexpr int SLOTS = 1;
    SmoothModel<N> model;
    template <typename Args>
    MHT_HD void advance(const Args&, int, int, double* x, double* P) const { smooth_advance<N>(model, x, P); }
    template <bool COV, typename Args>
    MHT_HD void backward(const Args&, int, int, const double* xf, const double* Pf, double* x, double* P) const {
        smooth_backward<N, COV>(model, xf, Pf, x, P);
    }
};

// A_k = Phi(T, w) at the filtered turn rate of the node stepped from: x[4] going forward, xf[4] (the same bits, read back) going backward
struct ConstantTurnSteps {
    static constexpr int SLOTS = 1;
    SmoothCtModel model;
    template <typename Args>
    MHT_HD void advance(const Args&, int, int, double* x, double* P) const {
        double xp[6], AP[36], Pp[21];
        smooth_ct_predict(model, ct_transition(model.T, x[4]), x, P, xp, AP, Pp);
#pragma unroll
        for (int i = 0; i < 6; ++i) x[i] = xp[i];
#pragma unroll
        for (int e = 0; e < 21; ++e) P[e] = Pp[e];
    }
    template <bool COV, typename Args>
    MHT_HD void backward(const Args&, int, int, const double* xf, const double* Pf, double* x, double* P) const {
        smooth_ct_backward<COV>(model, xf, Pf, x, P);
    }
};

// A node whose kind is >= 2 took an AIS message and steps over its two legs; slot 1 keeps its filtered state at the message's time
// (written and read for such nodes only).  Any other node is the linear smoother's, call for call.
struct AisSteps {
    static constexpr int SLOTS = 2;
    SmoothModel<4> model;     // the plain step's A, Q and the radar update's C, R
    const uint8_t* kind;      // [L_max][n]
    const double* ais_z;      // [L_max][4][n]
    const double* ais_r;      // [L_max][n]
    const int32_t* leg;       // [L_max][n]
    const double* legs;       // [n_legs][52]
    template <typename Args>
    MHT_HD void advance(const Args& a, int k, int t, double* x, double* P) const {
        const size_t n = (size_t)a.n;
        if (kind[(size_t)k * n + t] >= 2) {
            const double* entry = legs + (size_t)leg[(size_t)k * n + t] * SMOOTH_AIS_LEG_DOUBLES;
            double m[4], xm[4], Pm[10];
#pragma unroll
            for (int i = 0; i < 4; ++i) m[i] = ais_z[((size_t)k * 4 + i) * n + t];
            smooth_ais_forward(entry, m, ais_r[(size_t)k * n + t], x, P, xm, Pm);
            smooth_store_filtered(a, k, 1, t, xm, Pm);
        } else {
            smooth_advance<4>(model, x, P);
        }
    }
    template <bool COV, typename Args>
    MHT_HD void backward(const Args& a, int k, int t, const double* xf, const double* Pf, double* x, double* P) const {
        const size_t n = (size_t)a.n;
        if (kind[(size_t)(k + 1) * n + t] >= 2) {
            const double* entry = legs + (size_t)leg[(size_t)(k + 1) * n + t] * SMOOTH_AIS_LEG_DOUBLES;
            double xm[4], Pm[10];
            smooth_load_filtered(a, k + 1, 1, t, xm, Pm);
            smooth_ais_backward<COV>(entry, xm, Pm, xf, Pf, x, P);
        } else {
            smooth_backward<4, COV>(model, xf, Pf, x, P);
        }
    }
};

// Track t, forward and backward
template <int N, bool COV, typename Steps>
MHT_HD void smooth_walk(const SmoothArgs<N, Steps>& a, int t) {
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
    // forward: node 0 is the initial state; node k >= 1 advances and, with a measurement, updates
    for (int k = 0; k < len; ++k) {
        if (k > 0) {
            a.steps.advance(a, k, t, x, P);
            if (a.has_z[(size_t)k * n + t]) smooth_update<N>(a.steps.model, a.z[((size_t)k * 2) * n + t], a.z[((size_t)k * 2 + 1) * n + t], x, P);
        }
        if (k < len - 1) smooth_store_filtered(a, k, 0, t, x, P);      // (the last node's filtered state is its smoothed state: it stays in registers)
    }
    // backward: (x, P) is the smoothed state of node k + 1 on entry of a step and of node k afterwards
    for (int k = len - 1; k >= 0; --k) {
        if (k < len - 1) {
            double xf[N], Pf[NS];
            smooth_load_filtered(a, k, 0, t, xf, Pf);
            a.steps.template backward<COV>(a, k, t, xf, Pf, x, P);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) a.xs[((size_t)k * N + i) * n + t] = x[i];
        if (COV) {
#pragma unroll
            for (int e = 0; e < NS; ++e) a.Ps[((size_t)k * NS + e) * n + t] = P[e];
        }
    }
}

}  // namespace mht
