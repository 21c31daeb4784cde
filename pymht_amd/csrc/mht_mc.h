// Encounters by Monte Carlo (mht_mc_encounters, include/mht_amd.h): every target is a GAUSSIAN MIXTURE of components (x_c, P_c) -- the
// leaves of the forest --, S particles per target are drawn from it, walked over K steps of the tracker's own model WITH process noise,
// and held against G paths of the own ship.  What is counted per (path, target) is how many particles are within the safety radius R at
// each step (within) and how many come within it AT ANY TIME of the horizon (ever): the first-passage figure no per-step Gaussian rule
// gives, for a mixture no single Gaussian stands for, and for the constant-turn model, whose transition depends on the state.  The code
// a lane of the kernels of mht_mc.hip runs per component and per particle, and tests/hostmath/mc_host.cpp on the CPU.  Every model here
// orders its state [x, y, vx, vy, ...]; the constant-turn one is models/ct.py's [x, y, vx, vy, w, a].
//
// Every sum here is written out in plain operations in one order (the library is compiled with -ffp-contract=off), the order
// tests/mc_ref.py restates.  The counts are integers: the same bits from run to run and under any split of a target's particles.
//
// RANDOM NUMBERS (mc_philox).  Philox4x32-10 of Random123 (Salmon, Moraes, Dror, Shaw 2011): multipliers 0xD2511F53 and 0xCD9E8D57, key
// increments 0x9E3779B9 and 0xBB67AE85, ten rounds, the key bumped in front of every round but the first.  Integer only: bit-identical on
// host and device.  The counter is (particle, step, target, block), the key (seed & 0xffffffff, seed >> 32):
//   block 0 of step k   the normals z0 .. z3 of step k (k = 0: the draw of X_0, k = 1 .. K: the process noise of step k)
//   block 1 of step k   z4 .. z7, six-state models only; z6 and z7 are not used (and not computed)
//   step 0xffffffff, block 0, word 0   the uniform that picks the particle's component
// The stream is keyed by TARGET, not by component: which leaf a particle picks does not move its noise.
// A word r becomes u = (r + 0.5) * 2^-32 in float64 (exact: 0 < u < 1), and a pair of words two normals by Box-Muller,
//   rad = sqrt(-2 * log(u0)), ang = 6.283185307179586 * u1, z0 = rad * cos(ang), z1 = rad * sin(ang)      (z2, z3 from u2, u3)
// so |z| <= sqrt(-2 log 2^-33) = 6.77 < 6.8: THE TAILS ARE CUT where 1.3e-11 of a normal's mass lies.
//
// FACTOR (mc_factor<N>).  The lower factor L, A = L L', of a symmetric positive-SEMIdefinite matrix (the upper triangle is read) by
// Cholesky with a zero-pivot rule -- a definition, not a measurement.  tol = 64 eps max_i A_ii; column j, d = A_jj - sum_{k<j} L_jk^2
// (k upward):
//   d > tol            L_jj = sqrt(d), L_ij = (A_ij - sum_{k<j} L_ik L_jk) / L_jj for i > j
//   -tol <= d <= tol   a zero column
//   d < -tol           not positive semidefinite (status 2)
// Used for every component's P (the own ship's P = 0 and an exactly known state are legitimate) and once for Q (models/ct.Q has rank 3:
// plain Cholesky fails on it).
// THE TOLERANCE OF Q is another one, tol_j = MC_Q_TOL Q_jj = 2^-20 of the column's OWN diagonal entry, and the reason is the number
// format of the models: their matrices are float32 (models/constants.defaultType), every entry rounded on its own to 2^-24 relative, so
// a Q of exact rank 3 arrives with pivots of a few 2^-24 of their own diagonal entry, in either sign.  models/ct.Q(5): the pivot of
// column 5 is -3.6e-12 where 64 eps max_i Q_ii is 2.2e-12 -- the rule above calls that matrix indefinite --, which is 1.4e-7 = 2.4 * 2^-24
// of Q_55 = 2.5e-5.  The scale is the column's own entry and not the largest one because ct.Q's turn-rate block is 1e-6 of its position
// block: measured against the largest entry, a tolerance that forgives float32 rounding would also delete the turn-rate noise at short
// steps.  2^-20 is sixteen roundings.  The components' P keep 64 eps max_i P_ii: they are float64 results of a filter.
//
// WALK (mc_walk<N, CT>).  Particle p of target t:
//   1. component c: the first of the target's range first[t] .. first[t + 1] - 1 with u < cdf[c], by binary search (none: the last);
//      a component of weight 0 has cdf[c] = cdf[c - 1] (or 0 as the first) and is never picked
//   2. X_0[i] = x_c[i] + ((L_c[i][0] * z0 + L_c[i][1] * z1) + ... + L_c[i][i] * zi)
//   3. k = 1 .. K, F the factor of Q, z the normals of step k:
//        linear          X_k[i] = ((Phi[i][0] * X[0] + Phi[i][1] * X[1]) + ... + Phi[i][N-1] * X[N-1]) + F[i][0] * z0 + ... + F[i][i] * zi
//        constant turn   the same with Phi(dt, w) at the particle's OWN turn rate w = X_{k-1}[4] -- the real model, not a linearisation --
//                        from mht_smooth_ct_math.h's ct_transition (sw, cw, c, s and its |w| < 1e-9 limits), the product in the linear
//                        product's order with the structural zeros and ones of Phi(dt, w) left out (for finite states the value of
//                        the dense product):
//                          (X0 + sw * X2) + (-cw) * X3,  (X1 + cw * X2) + sw * X3,  c * X2 + (-s) * X3,  s * X2 + c * X3,  X4 + dt * X5,  X5
// Against own path g, d_k = X_k[0:2] - own[g][k]:
//   within[g][k]   the particles with dx * dx + dy * dy < R * R at step k
//   ever[g]        the particles whose piecewise-linear path through d_0 .. d_K comes inside R: inside at a step, or on segment
//                  k - 1 -> k the point at mht_encounter.h's clamped s* = clamp(-d_{k-1} . e / |e|^2, 0, 1), e = d_k - d_{k-1} (s* = 0 for
//                  e = 0), has a squared distance < R * R.  (The steps are tested as well as the segments because d_{k-1} + 1 * e need not
//                  round to d_k: ever >= within[k] holds by construction.)
//
// STATUS PER TARGET.  0: scored.  1: a NaN in a component's x, P or cdf.  2: a component's P is not positive semidefinite (1 wins over
// 2).  A target of status 1 or 2 has every count 0 and valid = 0; a scored one has valid = S.
//
// THE SPLIT (mc_chunks).  A workgroup of MC_THREADS = 256 lanes walks a slab of one target's particles, one lane one particle, looped.
// A target's S particles are cut into chunks of `slab` particles, slab a multiple of 256: as many chunks as bring the launch to
// MC_FILL = 1024 workgroups (four for each of the 256 compute units), at most one per 256 particles; 1024 targets or more get one chunk.
// The split depends on (T, S) alone -- not on the device -- so the sizer and the launch agree, and it does not move a count.
#pragma once
#include <type_traits>
#include "mht_smooth_ct_math.h"

namespace mht {

constexpr int MC_MAX_PATHS = 64;              // MHT_MC_MAX_PATHS of include/mht_amd.h: one lane of a wavefront per path
constexpr int MC_MAX_STEPS = 64;              // MHT_MC_MAX_STEPS
constexpr int MC_MAX_PARTICLES = 1 << 20;     // MHT_MC_MAX_PARTICLES
constexpr int MC_WARP = 64;                   // MHT_MC_WARP: particles come in whole wavefronts
constexpr int MC_THREADS = 256;
constexpr int MC_FILL = 1024;
constexpr double MC_P_TOL = 64.0 * 2.220446049250313e-16;
constexpr double MC_Q_TOL = 9.5367431640625e-07;      // 2^-20
constexpr uint32_t MC_PICK_STEP = 0xffffffffu;

struct McSplit { int32_t chunks, slab; };

MHT_HD McSplit mc_chunks(int32_t T, int32_t S) {
    const int32_t most = (S + MC_THREADS - 1) / MC_THREADS, fill = (MC_FILL + T - 1) / T;
    const int32_t want = most < fill ? most : fill;      // (>= 1)
    McSplit s;
    s.slab = ((S + want - 1) / want + MC_THREADS - 1) / MC_THREADS * MC_THREADS;
    s.chunks = (S + s.slab - 1) / s.slab;
    return s;
}

struct McRand { uint32_t v[4]; };

MHT_HD McRand mc_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r > 0) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
    return McRand{{c0, c1, c2, c3}};
}

MHT_HD double mc_uniform(uint32_t r) { return ((double)r + 0.5) * 2.3283064365386963e-10; }

MHT_HD void mc_box_muller(uint32_t r0, uint32_t r1, double& z0, double& z1) {
    const double rad = sqrt(-2.0 * log(mc_uniform(r0))), ang = 6.283185307179586 * mc_uniform(r1);
    z0 = rad * cos(ang);
    z1 = rad * sin(ang);
}

// The N normals of (particle, step, target)
template <int N>
MHT_HD void mc_normals(uint32_t particle, uint32_t step, uint32_t target, uint64_t seed, double* z) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const McRand a = mc_philox(particle, step, target, 0u, k0, k1);
    mc_box_muller(a.v[0], a.v[1], z[0], z[1]);
    mc_box_muller(a.v[2], a.v[3], z[2], z[3]);
    if (N == 6) {
        const McRand b = mc_philox(particle, step, target, 1u, k0, k1);
        mc_box_muller(b.v[0], b.v[1], z[4], z[5]);
    }
}

// A [N][N] row-major (the upper triangle is read) -> L packed by rows (L[i][j], j <= i, at i (i + 1) / 2 + j).  Returns 0, or 2 for a
// matrix that is not positive semidefinite (L is then not to be used).  OWN false: tol = MC_P_TOL max_i A_ii (a component's P); true:
// tol_j = MC_Q_TOL A_jj (Q).
template <int N, bool OWN>
MHT_HD int mc_factor(const double* A, double* L) {
    double top = A[0];
#pragma unroll
    for (int i = 1; i < N; ++i) top = fmax(top, A[i * N + i]);
    int status = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double tol = OWN ? MC_Q_TOL * fabs(A[j * N + j]) : MC_P_TOL * top;
        double d = A[j * N + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        const bool live = d > tol;
        if (!live && !(d >= -tol)) status = 2;
        const double root = live ? sqrt(d) : 1.0;
        L[j * (j + 1) / 2 + j] = live ? root : 0.0;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double a = A[j * N + i];
#pragma unroll
            for (int k = 0; k < j; ++k) a = a - L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = live ? a / root : 0.0;
        }
    }
    return status;
}

// Component c of nComp: x [N][nComp], P packed upper [N (N + 1) / 2][nComp], cdf [nComp] -> L packed by rows [N (N + 1) / 2][nComp]
// and the component's status (1: a NaN, 2: not positive semidefinite)
template <int N>
MHT_HD void mc_component(const double* x, const double* P, const double* cdf, int nComp, int c, double* Lw, int32_t* status) {
    constexpr int NS = N * (N + 1) / 2;
    const size_t nn = (size_t)nComp;
    double A[N * N], L[NS];
    bool there = cdf[c] == cdf[c];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double v = x[(size_t)i * nn + c];
        there = there && v == v;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) {
            const double v = P[(size_t)sym_idx(N, i, j) * nn + c];
            there = there && v == v;
            A[i * N + j] = v;
        }
    const int f = mc_factor<N, false>(A, L);
#pragma unroll
    for (int i = 0; i < NS; ++i) Lw[(size_t)i * nn + c] = L[i];
    status[c] = there ? f : 1;
}

template <int N>
struct McModel {
    double Phi[N * N];               // row-major; not read by the constant-turn walk
    double F[N * (N + 1) / 2];       // the factor of Q, packed by rows
    double dt, R2;
};

MHT_HD bool mc_finite(double v) { return v - v == 0.0; }

// The model of a call: Phi copied (null: zeros, for the constant-turn walk, which does not read it) and Q factored.  False: Q is not
// positive semidefinite.
template <int N>
MHT_HD bool mc_model(const double* Phi, const double* Q, double dt, double R, McModel<N>& m) {
    for (int c = 0; c < N * N; ++c) m.Phi[c] = Phi ? Phi[c] : 0.0;
    m.dt = dt;
    m.R2 = R * R;
    return mc_factor<N, true>(Q, m.F) == 0;
}

// (nx, transition), as the seams admit them, to the instance <N, CT>: f(std::integral_constant<int, N>, std::bool_constant<CT>)
template <class F>
auto mc_dispatch(int nx, int transition, F&& f) {
    if (nx == 4) return f(std::integral_constant<int, 4>{}, std::false_type{});
    if (transition != 0) return f(std::integral_constant<int, 6>{}, std::true_type{});
    return f(std::integral_constant<int, 6>{}, std::false_type{});
}

// The status of target t from its components' (1 wins over 2): the serial form of the kernels' strided fold
MHT_HD int mc_target_status(const int32_t* first, const int32_t* cstatus, int t) {
    bool nan = false, indefinite = false;
    for (int c = first[t]; c < first[t + 1]; ++c) {
        nan = nan || cstatus[c] == 1;
        indefinite = indefinite || cstatus[c] == 2;
    }
    return nan ? 1 : (indefinite ? 2 : 0);
}

// The first component of lo .. hi (inclusive) with u < cdf[c]; hi if there is none
MHT_HD int mc_pick(const double* cdf, int lo, int hi, double u) {
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (u < cdf[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

template <int N, bool CT>
MHT_HD void mc_step(const McModel<N>& m, const double* z, double* X) {
    double Y[N];
    if constexpr (CT) {
        static_assert(N == 6, "the constant-turn model has six states");
        const CtTransition t = ct_transition(m.dt, X[4]);
        Y[0] = (X[0] + t.sw * X[2]) + (-t.cw) * X[3];
        Y[1] = (X[1] + t.cw * X[2]) + t.sw * X[3];
        Y[2] = t.c * X[2] + (-t.s) * X[3];
        Y[3] = t.s * X[2] + t.c * X[3];
        Y[4] = X[4] + m.dt * X[5];
        Y[5] = X[5];
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double acc = m.Phi[i * N] * X[0];
#pragma unroll
            for (int l = 1; l < N; ++l) acc = acc + m.Phi[i * N + l] * X[l];
            Y[i] = acc;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double acc = Y[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) acc = acc + m.F[i * (i + 1) / 2 + j] * z[j];
        X[i] = acc;
    }
}

// Is the closest point of the segment from (px, py) to (dx, dy) inside the disc?  mht_encounter.h's clamped s*.
MHT_HD bool mc_segment_inside(double px, double py, double dx, double dy, double R2) {
    const double ex = dx - px, ey = dy - py;
    const double ee = ex * ex + ey * ey;
    double sp = 0.0;
    if (ee > 0.0) sp = fmin(fmax(-(px * ex + py * ey) / ee, 0.0), 1.0);
    const double cx = px + sp * ex, cy = py + sp * ey;
    return cx * cx + cy * cy < R2;
}

// X_0 of a particle from component c of nn: step 2 of the walk
template <int N>
MHT_HD void mc_draw(const double* x, const double* Lw, size_t nn, int c, const double* z, double* X) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double acc = Lw[(size_t)(i * (i + 1) / 2) * nn + c] * z[0];
#pragma unroll
        for (int j = 1; j <= i; ++j) acc = acc + Lw[(size_t)(i * (i + 1) / 2 + j) * nn + c] * z[j];
        X[i] = x[(size_t)i * nn + c] + acc;
    }
}

// Particle p of target t, held against the G paths of own [G][K + 1][2].  `live` false: a lane beyond the slab's end, which walks along
// (the sink's ballots and barriers want every lane) and counts nowhere.  The sink takes
//   within(g, inside)   per step, g = 0 .. G - 1 in turn, then   step_done(k)
//   ever(g, came)       at the end, g in turn, then              particle_done()
template <int N, bool CT, class Sink>
MHT_HD void mc_walk(const McModel<N>& m, const double* x, const double* Lw, const int32_t* first, const double* cdf, const double* own, int nComp,
                    int G, int K, uint64_t seed, int t, uint32_t p, bool live, Sink& sink) {
    const size_t nn = (size_t)nComp;
    double X[N], z[N];
    const McRand pick = mc_philox(p, MC_PICK_STEP, (uint32_t)t, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int c = mc_pick(cdf, first[t], first[t + 1] - 1, mc_uniform(pick.v[0]));
    uint64_t came = 0;      // bit g: the path has come inside R of own path g
    double px = 0.0, py = 0.0;
    int k = 0;
    do {      // (K >= 1 and G >= 1, the seam's ranges: loops without a guard in front)
        mc_normals<N>(p, (uint32_t)k, (uint32_t)t, seed, z);
        if (k == 0) mc_draw<N>(x, Lw, nn, c, z, X);
        else mc_step<N, CT>(m, z, X);
        int g = 0;
        do {
            const double* o = own + ((size_t)g * (size_t)(K + 1) + (size_t)k) * 2;
            const double dx = X[0] - o[0], dy = X[1] - o[1];
            const bool inside = dx * dx + dy * dy < m.R2;
            bool hit = inside;
            if (k > 0) hit = hit || mc_segment_inside(px - o[-2], py - o[-1], dx, dy, m.R2);
            came |= (uint64_t)(hit ? 1 : 0) << g;
            sink.within(g, live && inside);
        } while (++g < G);
        sink.step_done(k);
        px = X[0];
        py = X[1];
    } while (++k <= K);
    int g = 0;
    do sink.ever(g, live && ((came >> g) & 1) != 0);
    while (++g < G);
    sink.particle_done();
}

}  // namespace mht
