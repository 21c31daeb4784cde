// Per-track arithmetic of the AIS-aware Rauch-Tung-Striebel smoother (mht_smooth_tracks_ais, include/mht_amd.h), four states, float64
// throughout, under the rules of mht_smooth_math.h: one track per lane, every loop unrolled, every array statically indexed, covariances
// symmetric packed, every multiply-add an explicit fma.
//
// The model is the one the forest filters an AIS-aided track with (mht_ais_math.h, steps 1-6 of Tracker.__fuseRadarAndAis).  A node
// that took an AIS message did not step one radar period with Phi(T), Q(T): it went
//   leg 1    predict with A1 = Phi(dT1), Q1 = Q(dT1) to the message's time
//   AIS      update with the message m [4]: C = I4, R = r I4, r = sigma^2 of the message's accuracy class
//   leg 2    predict with A2 = Phi(dT2), Q2 = Q(dT2) to the scan's time
//   radar    update with the plot, if the node has one
// and the smoother of that model walks the same way back: two Rauch-Tung-Striebel steps per such node, over leg 2 to the message's
// time (from the filtered state stored there, behind the AIS update) and over leg 1 to the node in front.  Both legs ARE steps of the
// linear smoother with another A and Q, so they are smooth_predict<4> and smooth_backward<4, COV> called with a leg's matrices in a
// SmoothModel<4>; the radar update is smooth_update<4>; a node without a message is the linear smoother's step, call for call -- a
// batch without any message gives mht_smooth_tracks' bits.  What is new is the AIS update alone.
#pragma once
#include "mht_smooth_math.h"

namespace mht {

// One entry of the leg table: the two legs of every node whose message has this (dT1, dT2).  The matrices are the float32 ones the
// forest filtered with (pymht_amd/ais.py::group_messages), widened: exact.
constexpr int SMOOTH_AIS_LEG_DOUBLES = 52;      // A1 [16] row-major, Q1 [10] packed, A2 [16], Q2 [10]

// Leg WHICH (0: A1, Q1; 1: A2, Q2) of a table entry as the model smooth_predict / smooth_backward take (C and R are not theirs to read)
template <int WHICH>
MHT_HD void smooth_ais_leg(const double* entry, SmoothModel<4>& m) {
#pragma unroll
    for (int e = 0; e < 16; ++e) m.A[e] = entry[WHICH * 26 + e];
#pragma unroll
    for (int e = 0; e < 10; ++e) m.Q[e] = entry[WHICH * 26 + 16 + e];
}

// AIS update of (x, P) in place with the message m [4] and r = sigma^2:  S = P + r I, K = P S^-1, x += K (m - x), P -= K P.
// S is symmetric positive definite (P is a covariance, r > 0): K goes through its Cholesky factor S = U' U, row i of K solving
// k U' U = row i of P, as G does in smooth_backward_gain.  Only the upper triangle of P - K P is formed: symmetric by construction.
MHT_HD void smooth_ais_update(const double* m, double r, double* x, double* P) {
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
        for (int j = 0; j < 4; ++j) {      // y U = b (forward: U' is lower), b_j = P[i][j]
            double s = P[sym_idx(4, i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s = fma(-y[k], U[sym_idx(4, k, j)], s);
            y[j] = s * inv_d[j];
        }
#pragma unroll
        for (int j = 3; j >= 0; --j) {      // k U' = y (backward)
            double s = y[j];
#pragma unroll
            for (int k = j + 1; k < 4; ++k) s = fma(-K[i * 4 + k], U[sym_idx(4, j, k)], s);
            K[i * 4 + j] = s * inv_d[j];
        }
    }
    double d[4];      // innovation m - x
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = m[j] - x[j];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double acc = x[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = fma(K[i * 4 + j], d[j], acc);
        x[i] = acc;
    }
    double Pn[10];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            double acc = P[sym_idx(4, i, j)];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fma(-K[i * 4 + k], P[sym_idx(4, k, j)], acc);
            Pn[sym_idx(4, i, j)] = acc;
        }
#pragma unroll
    for (int e = 0; e < 10; ++e) P[e] = Pn[e];
}

// Forward pass over the two legs of an AIS node.  In: (x, P) the filtered state of the node in front.  Out: (xm, Pm) the filtered state
// at the message's time, behind the AIS update (the backward pass starts its second step from it); (x, P) the prediction at the
// scan's time, which the caller updates with the radar plot if the node has one.
MHT_HD void smooth_ais_forward(const double* entry, const double* m, double r, double* x, double* P, double* xm, double* Pm) {
    SmoothModel<4> lg;
    double AP[16];
    smooth_ais_leg<0>(entry, lg);
    smooth_predict<4>(lg, x, P, xm, AP, Pm);
    smooth_ais_update(m, r, xm, Pm);
    smooth_ais_leg<1>(entry, lg);
    smooth_predict<4>(lg, xm, Pm, x, AP, P);
}

// Backward pass over an AIS node.  In: (xs, Ps) its smoothed state, (xm, Pm) the filtered state at its message's time, (xf, Pf) the
// filtered state of the node in front.  Out, in place: (xs, Ps) of the node in front; the smoothed state at the message's time is an
// intermediate.  COV = false: means only.
template <bool COV>
MHT_HD void smooth_ais_backward(const double* entry, const double* xm, const double* Pm, const double* xf, const double* Pf, double* xs, double* Ps) {
    SmoothModel<4> lg;
    smooth_ais_leg<1>(entry, lg);
    smooth_backward<4, COV>(lg, xm, Pm, xs, Ps);
    smooth_ais_leg<0>(entry, lg);
    smooth_backward<4, COV>(lg, xf, Pf, xs, Ps);
}

}  // namespace mht
