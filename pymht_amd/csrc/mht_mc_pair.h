// Encounters by Monte Carlo between PAIRS OF TARGETS (mht_mc_pair_encounters, include/mht_amd.h): the target-against-target question of
// a VTS operator or a fleet monitor, with the engine of mht_mc.h -- the forest's own leaves sampled as a mixture per target, every
// particle walked with process noise and, under the constant-turn model, with Phi(dt, w) of its own turn rate, counts that are the
// same bits for one seed.  This header includes mht_mc.h and uses its functions unchanged: mc_philox keyed by (seed, target) -- the
// streams of two targets are independent by construction --, mc_normals, the zero-pivot factor (mc_factor, mc_component), mc_pick,
// mc_draw, mc_step<N, CT> and mc_segment_inside.  What it adds is a walk that carries two particles at once.  The code a lane of
// mc_pair_walk_kernel (mht_mc.hip) runs per pair-particle, and tests/hostmath/mc_pair_host.cpp on the CPU.
//
// DEFINITION.  For pair j = (a, b) of distinct targets and particle index p = 0 .. S - 1: particle p of target a and particle p of
// target b are walked EXACTLY as mc_walk walks them -- the same counter words (particle, step, target, block), the same order of every
// sum, the same pick of a component, the same mc_step<N, CT> --, so particle p of target t is the same particle whatever it is held
// against, an own path or another target.  With d_k = X^a_k[0:2] - X^b_k[0:2], k = 0 .. K:
//   within[k][j]    the particles with dx * dx + dy * dy < R * R at step k
//   hit_k           inside at step k, or, for k >= 1, mc_segment_inside(d_{k-1}, d_k, R2): the piecewise-linear RELATIVE path with
//                   mht_encounter.h's clamped s*, as against an own path
//   ever[j]         the particles with any hit_k
//   firstAt[k][j]   the particles whose smallest k with hit_k is k: the distribution of the time to the first violation
// By construction sum_k firstAt[k][j] == ever[j] and ever >= max_k within; and swapping a and b gives the same counts bit for bit:
// d changes its sign, negation is exact, and every product of the tests is even in the sign.
//
// STATUS PER PAIR.  0: scored.  1: either target has a component with a NaN in x, P or cdf.  2: either target has a component whose P
// is not positive semidefinite (1 wins over 2).  A pair that is not scored has every count 0 and valid = 0; a scored one valid = S.
//
// NO PARTICLE POSITION IS STORED: a target that is in many pairs is walked once per pair.  The alternative, the positions of every
// target kept as [T][K + 1][2][S] float64, is 0.8 GB for 500 targets, 24 steps and 4 096 particles, to be read once per pair, and the
// generator is cheap (integer Philox, one log, sin and cos per two normals).
//
// THE SPLIT is mc_chunks(nPair, S): a workgroup walks a slab of one pair's particle indices; the counts do not depend on it.
#pragma once
#include "mht_mc.h"

namespace mht {

constexpr int MC_MAX_PAIRS = 1 << 20;      // MHT_MC_MAX_PAIRS of include/mht_amd.h

// Particle p of target ta against particle p of target tb.  The sink takes
//   step(k, inside, first)   per step: the pair is inside R at step k; k is the first step with hit_k
//   done(came)               at the end: the relative path came inside R
// and may keep the two states and the relative position of every step (path(k, Xa, Xb, dx, dy): the host twin's; nothing on the device).
template <int N, bool CT, class Sink>
MHT_HD void mc_pair_walk(const McModel<N>& m, const double* x, const double* Lw, const int32_t* first, const double* cdf, int nComp, int K, uint64_t seed,
                         int ta, int tb, uint32_t p, Sink& sink) {
    const size_t nn = (size_t)nComp;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    double X[N], Y[N], z[N];
    uint32_t came = 0;      // (a word of the lane, not a predicate: a predicate carried over the walk is a pair of scalar registers)
    int tx = ta, ty = tb;
    double px = 0.0, py = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) X[i] = Y[i] = 0.0;
    // Particle a, then particle b, by ONE body run over the 2 (K + 1) HALF-steps h: X is the particle stepped next, Y the other, and they
    // change places after each half -- a's and b's sin, cos and log are the same instructions and the same temporaries, where two
    // inlined copies, interleaved by the scheduler, take a six-state lane past 256 vector registers.  The distance is taken after
    // every second half, when X is a's particle again and Y b's.
    int h = 0;
    do {      // (K >= 1, the seam's range)
        const int k = h >> 1;
        mc_normals<N>(p, (uint32_t)k, (uint32_t)tx, seed, z);
        if (k == 0) {      // (the particle's component and X_0, as mc_walk picks and draws them)
            const McRand u = mc_philox(p, MC_PICK_STEP, (uint32_t)tx, 0u, k0, k1);
            mc_draw<N>(x, Lw, nn, mc_pick(cdf, first[tx], first[tx + 1] - 1, mc_uniform(u.v[0])), z, X);
        } else {
            mc_step<N, CT>(m, z, X);
        }
        const int t = tx;
        tx = ty;
        ty = t;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double v = X[i];
            X[i] = Y[i];
            Y[i] = v;
        }
        if ((h & 1) == 0) continue;
        const double dx = X[0] - Y[0], dy = X[1] - Y[1];
        const bool inside = dx * dx + dy * dy < m.R2;
        bool hit = inside;
        if (k > 0) hit = hit || mc_segment_inside(px, py, dx, dy, m.R2);
        sink.path(k, X, Y, dx, dy);
        sink.step(k, inside, hit && came == 0u);
        came |= hit ? 1u : 0u;
        px = dx;
        py = dy;
    } while (++h <= 2 * K + 1);
    sink.done(came != 0u);
}

// The status of a pair from its two targets' (1 wins over 2)
MHT_HD int mc_pair_status(int sa, int sb) { return (sa == 1 || sb == 1) ? 1 : ((sa == 2 || sb == 2) ? 2 : 0); }

}  // namespace mht
