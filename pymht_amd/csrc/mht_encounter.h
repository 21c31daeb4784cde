// Encounters ahead of the current scan: every live track propagated over a horizon with the tracker's own Phi and Q, and per pair of
// tracks the closest point of approach and the largest probability, over the horizon, that the two are within a safety radius of each
// other (mht_encounters, include/mht_amd.h).  The code a lane of the kernels of mht_encounter.hip runs per entry and per pair, and
// tests/hostmath/encounter_host.cpp on the CPU.  Every model here orders its state [x, y, vx, vy, ...].
//
// PROPAGATION (encounter_propagate).  An entry is x [N] and the packed upper P [N (N + 1) / 2] at one common time; for k = 0 .. K
//   x_k = Phi x_{k-1},   P_k = Phi P_{k-1} Phi' + Q                                                     (k = 0: the entry as it is)
// and what is kept is the position p_k = x_k[0:2] and its covariance S_k = (P_k[0][0], P_k[0][1], P_k[1][1]):
//   pos [K + 1][2][n], S [K + 1][3][n], track-minor.  A NaN in an entry's x or P makes the whole entry NaN.
//
// PAIR (encounter_pair), entries i < j, taken as INDEPENDENT: d_k = p_i,k - p_j,k, Sigma_k = S_i,k + S_j,k.
//   dcpa, tcpa   the minimum of |d(t)| over the piecewise-linear path through d_0 .. d_K and the time it is reached at: per segment
//                s* = clamp(-d_k . e / |e|^2, 0, 1) with e = d_{k+1} - d_k (s* = 0 for e = 0), the earliest minimum wins (strict <
//                on the squared distance, k upward), tcpa = (k + s*) dt.  Exact for a constant-velocity model; for a constant-
//                acceleration model it is this piecewise-linear figure.
//   md2          min over k of d_k' Sigma_k^-1 d_k (closed form of the 2 x 2 inverse)
//   pc, tpc      max over k of pc_k and the time k dt of it, the earliest k wins; pc_k is the mass of N(d_k, Sigma_k) inside the disc
//                of radius R around 0, BY THIS RULE (encounter_pc) and nothing else: Sigma_k = s1^2 v1 v1' + s2^2 v2 v2' in closed form
//                with s1 <= s2, d_k rotated into (m1, m2); the disc is symmetric under both reflections, so m1 = |m1| and
//                m2 = -|m2| are taken (the eigenvectors' signs are arbitrary: this makes the figure the same bits under a swap of
//                the pair).  lo = max(-R, m1 - 8 s1), hi = min(R, m1 + 8 s1); pc_k = 0 EXACTLY if hi <= lo; else the 64-node
//                Gauss-Legendre rule in theta over [asin(lo / R), asin(hi / R)] of
//                    phi((R sin theta - m1) / s1) / s1  [Phi((R cos theta - m2) / s2) - Phi((-R cos theta - m2) / s2)]  R cos theta
//                with the difference of the two Phi as 0.5 (erfc(u1 / sqrt 2) - erfc(u2 / sqrt 2)).  Against the exact mass this rule
//                is good to about 1e-6 absolute (worst where Sigma is isotropic and d lies near the disc's edge); it is not clamped
//                to 1.
// Sigma_k not positive definite at some k (Sigma_xx > 0 and det > 0 is the test): pc, tpc and md2 of the pair are NaN, dcpa and tcpa
// stay valid.  A NaN entry makes all five figures of its pairs NaN.
//
// Every sum here is written out in plain operations in one order (the library is compiled with -ffp-contract=off), the order
// tests/encounter_ref.py restates.
#pragma once
#include "mht_smooth_math.h"

namespace mht {

constexpr int ENCOUNTER_MAX_STEPS = 64;
constexpr int ENCOUNTER_FIGURES = 5;      // out [5][first][n]: tcpa, dcpa, md2, pc, tpc

// The positive nodes, ascending, and their weights of the 64-node Gauss-Legendre rule on [-1, 1] (32 symmetric pairs), 20 digits
struct EncounterRule {
    static constexpr double x[32] = {
        0.024350292663424432509, 0.07299312178779903945, 0.12146281929612055447, 0.16964442042399281804,
        0.21742364374000708415, 0.26468716220876741637, 0.31132287199021095616, 0.35722015833766811595,
        0.4022701579639916037, 0.44636601725346408798, 0.48940314570705295748, 0.53127946401989454566,
        0.57189564620263403428, 0.61115535517239325025, 0.64896547125465733986, 0.68523631305423324256,
        0.71988185017161082685, 0.75281990726053189661, 0.78397235894334140761, 0.81326531512279755974,
        0.84062929625258036275, 0.86599939815409281976, 0.88931544599511410585, 0.91052213707850280576,
        0.92956917213193957582, 0.94641137485840281606, 0.96100879965205371892, 0.97332682778991096374,
        0.98333625388462595693, 0.99101337147674432074, 0.99634011677195527935, 0.99930504173577213946};
    static constexpr double w[32] = {
        0.048690957009139720383, 0.048575467441503426935, 0.04834476223480295717, 0.047999388596458307728,
        0.047540165714830308662, 0.046968182816210017325, 0.046284796581314417296, 0.04549162792741814448,
        0.04459055816375656306, 0.043583724529323453377, 0.042473515123653589007, 0.04126256324262352861,
        0.039953741132720341387, 0.038550153178615629129, 0.03705512854024004604, 0.035472213256882383811,
        0.033805161837141609392, 0.032057928354851553585, 0.030234657072402478868, 0.028339672614259483228,
        0.026377469715054658672, 0.024352702568710873338, 0.022270173808383254159, 0.020134823153530209372,
        0.017951715775697343085, 0.015726030476024719322, 0.013463047896718642598, 0.011168139460131128819,
        0.008846759826363947723, 0.0065044579689783628561, 0.0041470332605624676353, 0.0017832807216964329473};
};

template <int N>
struct EncounterModel {
    double Phi[N * N], Q[N * N];      // row-major; of Q the upper triangle is read
};

// Entry t of n: x [N][n], P [N (N + 1) / 2][n] -> pos [K + 1][2][n], S [K + 1][3][n]
template <int N>
MHT_HD void encounter_propagate(const EncounterModel<N>& m, const double* x, const double* P, int n, int K, int t, double* pos, double* S) {
    constexpr int NS = N * (N + 1) / 2;
    const size_t nn = (size_t)n;
    const double nan = __builtin_nan("");
    double xk[N], Pf[N][N], T[N][N];
    bool there = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        xk[i] = x[(size_t)i * nn + t];
        there = there && xk[i] == xk[i];
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) {
            const double v = P[(size_t)sym_idx(N, i, j) * nn + t];
            there = there && v == v;
            Pf[i][j] = v;
            Pf[j][i] = v;
        }
    static_assert(NS == sym_idx(N, N - 1, N - 1) + 1, "packed upper triangle");
    for (int k = 0; k <= K; ++k) {
        if (k > 0) {
            double xn[N];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                double acc = m.Phi[i * N] * xk[0];
#pragma unroll
                for (int l = 1; l < N; ++l) acc = acc + m.Phi[i * N + l] * xk[l];
                xn[i] = acc;
            }
#pragma unroll
            for (int i = 0; i < N; ++i) xk[i] = xn[i];
#pragma unroll
            for (int i = 0; i < N; ++i)
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    double acc = m.Phi[i * N] * Pf[0][j];
#pragma unroll
                    for (int l = 1; l < N; ++l) acc = acc + m.Phi[i * N + l] * Pf[l][j];
                    T[i][j] = acc;
                }
#pragma unroll
            for (int i = 0; i < N; ++i)
#pragma unroll
                for (int j = i; j < N; ++j) {
                    double acc = T[i][0] * m.Phi[j * N];
#pragma unroll
                    for (int l = 1; l < N; ++l) acc = acc + T[i][l] * m.Phi[j * N + l];
                    acc = acc + m.Q[i * N + j];
                    Pf[i][j] = acc;
                    Pf[j][i] = acc;
                }
        }
        double* p = pos + (size_t)k * 2 * nn + t;
        double* s = S + (size_t)k * 3 * nn + t;
        p[0] = there ? xk[0] : nan;
        p[nn] = there ? xk[1] : nan;
        s[0] = there ? Pf[0][0] : nan;
        s[nn] = there ? Pf[0][1] : nan;
        s[2 * nn] = there ? Pf[1][1] : nan;
    }
}

// The integrand of the rule at theta, without the constant 1 / sqrt(2 pi)
MHT_HD double encounter_integrand(double theta, double R, double m1, double m2, double s1, double s2) {
    const double inv_sqrt2 = 0.70710678118654752440;
    const double sn = sin(theta), cs = cos(theta);
    const double z = (R * sn - m1) / s1;
    const double e = exp(-0.5 * z * z);
    const double rc = R * cs;
    const double u1 = (-rc - m2) / s2, u2 = (rc - m2) / s2;
    const double br = 0.5 * (erfc(u1 * inv_sqrt2) - erfc(u2 * inv_sqrt2));
    return e / s1 * br * rc;
}

// pc_k: the mass of N((dx, dy), [[a, b], [b, c]]) inside the disc of radius R around 0, by the rule at the head of this file.  The
// matrix is positive definite (the caller's test): det = a c - b b > 0, a > 0.
MHT_HD double encounter_pc(double dx, double dy, double a, double b, double c, double det, double R) {
    const double inv_sqrt_2pi = 0.39894228040143267794;
    const double h = 0.5 * (a + c), g = 0.5 * (a - c);
    const double r = sqrt(g * g + b * b);
    const double l2 = h + r, l1 = det / l2;      // (the smaller eigenvalue without the cancellation of h - r)
    double ux = g >= 0.0 ? g + r : b, uy = g >= 0.0 ? b : r - g;      // the axis of l2, in the form that does not cancel
    const double nrm = sqrt(ux * ux + uy * uy);
    if (nrm > 0.0) {
        ux = ux / nrm;
        uy = uy / nrm;
    } else {      // (isotropic: any axis)
        ux = 1.0;
        uy = 0.0;
    }
    const double m2 = -fabs(dx * ux + dy * uy), m1 = fabs(dy * ux - dx * uy);
    const double s1 = sqrt(l1), s2 = sqrt(l2);
    const double lo = fmax(-R, m1 - 8.0 * s1), hi = fmin(R, m1 + 8.0 * s1);
    if (!(hi > lo)) return 0.0;
    const double tl = asin(lo / R), th = asin(hi / R);
    const double mid = 0.5 * (th + tl), half = 0.5 * (th - tl);
    double sum = 0.0;
    for (int q = 0; q < 32; ++q) {
        const double t = half * EncounterRule::x[q];
        const double f = encounter_integrand(mid - t, R, m1, m2, s1, s2) + encounter_integrand(mid + t, R, m1, m2, s1, s2);
        sum = sum + EncounterRule::w[q] * f;
    }
    return half * sum * inv_sqrt_2pi;
}

// Pair (i, j) of the propagated entries: out5 = tcpa, dcpa, md2, pc, tpc
MHT_HD void encounter_pair(const double* pos, const double* S, int n, int K, double dt, double R, int i, int j, double* out5) {
    const size_t nn = (size_t)n;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    double best = inf, tcpa = 0.0, md2 = inf, pc = -1.0, tpc = 0.0, px = 0.0, py = 0.0;
    bool pd = true, there = true;
    for (int k = 0; k <= K; ++k) {
        const double* p = pos + (size_t)k * 2 * nn;
        const double* s = S + (size_t)k * 3 * nn;
        const double dx = p[i] - p[j], dy = p[nn + i] - p[nn + j];
        const double a = s[i] + s[j], b = s[nn + i] + s[nn + j], c = s[2 * nn + i] + s[2 * nn + j];
        there = there && dx == dx && dy == dy;
        if (k > 0) {      // segment k - 1: from (px, py) to (dx, dy)
            const double ex = dx - px, ey = dy - py;
            const double ee = ex * ex + ey * ey;
            double sp = 0.0;
            if (ee > 0.0) sp = fmin(fmax(-(px * ex + py * ey) / ee, 0.0), 1.0);
            const double cx = px + sp * ex, cy = py + sp * ey;
            const double dist2 = cx * cx + cy * cy;
            if (dist2 < best) {
                best = dist2;
                tcpa = ((double)(k - 1) + sp) * dt;
            }
        }
        const double det = a * c - b * b;
        pd = pd && a > 0.0 && det > 0.0;
        if (pd && there) {
            const double q = (c * dx * dx - 2.0 * b * dx * dy + a * dy * dy) / det;
            if (q < md2) md2 = q;
            const double pk = encounter_pc(dx, dy, a, b, c, det, R);
            if (pk > pc) {
                pc = pk;
                tpc = (double)k * dt;
            }
        }
        px = dx;
        py = dy;
    }
    out5[0] = there ? tcpa : nan;
    out5[1] = there ? sqrt(best) : nan;
    out5[2] = there && pd ? md2 : nan;
    out5[3] = there && pd ? pc : nan;
    out5[4] = there && pd ? tpc : nan;
}

// Cell (i, j) of out [5][first][n]: every figure written, NaN where j <= i
MHT_HD void encounter_cell(const double* pos, const double* S, int n, int first, int K, double dt, double R, int i, int j, double* out) {
    double o[ENCOUNTER_FIGURES];
    if (j > i) {
        encounter_pair(pos, S, n, K, dt, R, i, j, o);
    } else {
#pragma unroll
        for (int f = 0; f < ENCOUNTER_FIGURES; ++f) o[f] = __builtin_nan("");
    }
    double* cell = out + (size_t)i * (size_t)n + j;
#pragma unroll
    for (int f = 0; f < ENCOUNTER_FIGURES; ++f) cell[(size_t)f * (size_t)first * (size_t)n] = o[f];
}

}  // namespace mht
