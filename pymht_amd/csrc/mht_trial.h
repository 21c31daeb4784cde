// Trial manoeuvres of the own ship (mht_trial_manoeuvres, include/mht_amd.h): G candidate alterations of course and speed, each held
// against every one of n tracks over a horizon of K steps, and per candidate the worst track.  The tracks are propagated with
// encounter_propagate<N> and a cell (candidate g, track j) is encounter_pair of mht_encounter.h, both as they are: the figures of a
// cell -- tcpa, dcpa, md2, pc by the rule, tpc -- are defined there.  What this header adds is the path of a manoeuvring own ship
// (trial_candidate) and the fold of a candidate's row (trial_fold); the code a lane of the kernels of mht_trial.hip runs, and
// tests/hostmath/trial_host.cpp on the CPU.
//
// THE MANOEUVRE.  The own ship at the current scan is at p0 with velocity v0 and may carry a constant 2 x 2 position covariance S_own
// (xx, xy, yy).  A candidate is (dpsi, f, t0): the course change in radians, positive counter-clockwise in the tracker's axes,
// |dpsi| <= pi; the speed factor f >= 0; the delay t0 >= 0 in seconds.  One turn rate w > 0 (rad/s) serves all candidates.  With
// sg = sign(dpsi) (0 for dpsi = 0), ad = |dpsi|, te = t0 + ad / w and Rot(a) the plane rotation by a:
//   t <= t0        p(t) = p0 + t v0
//   t0 < t <= te   tau = t - t0, s = sin(w tau), c = cos(w tau), sw = s / w, cw = (1 - c) / w:
//                  p(t) = p(t0) + f [sw, -sg cw; sg cw, sw] v0         (the arc of models/ct.Phi at rate sg w and speed f |v0|; the
//                                                                       speed changes at t0 at once, ARPA's convention)
//   t > te         p(t) = p(te) + (t - te) f Rot(dpsi) v0
// dpsi = 0 has te = t0 and no arc; a t0 beyond the horizon is "stand on"; a turn may end beyond the horizon.  The positions are
// evaluated in closed form at t = k dt, k = 0 .. K, never accumulated from step to step, and S_own is the own ship's S_k at every k.
// A NaN in the candidate, in p0, v0 or S_own makes the candidate's trajectory NaN, and with it the five figures of its whole row.
//
// THE OPERATIONS, in this order (the library is compiled with -ffp-contract=off; tests/trial_ref.py restates them):
//   a  = p0 + t0 * v0                                        (per component: p0x + t0 * v0x)
//   se = sin(ad), ce = cos(ad), swe = se / w, cwe = (1 - ce) / w
//   b  = a + f * (swe * v0x - (sg * cwe) * v0y),  a_y + f * ((sg * cwe) * v0x + swe * v0y)                               = p(te)
//   u  = f * (ce * v0x - (sg * se) * v0y),  f * ((sg * se) * v0x + ce * v0y)                                  = f Rot(dpsi) v0
//   per k, t = (double)k * dt:
//     t <= t0   p = p0 + t * v0
//     t <= te   tau = t - t0, s = sin(w * tau), c = cos(w * tau), sw = s / w, cw = (1 - c) / w,
//               p = a_x + f * (sw * v0x - (sg * cw) * v0y),  a_y + f * ((sg * cw) * v0x + sw * v0y)
//     else      p = b + (t - te) * u
//
// THE FOLD.  Of a candidate's row: the largest pc with its track and the smallest dcpa with its track.  A NaN figure does not take
// part; among equal figures the lowest track index wins.  That order is total, so the fold gives the same bits in any grouping --
// lanes, wavefronts, tiles -- and nothing depends on which workgroup runs first.  A row without a figure gives NaN and -1.
#pragma once
#include "mht_encounter.h"

namespace mht {

constexpr int TRIAL_MAX_CANDIDATES = 4096;      // MHT_TRIAL_MAX_CANDIDATES of include/mht_amd.h
constexpr int TRIAL_TILE = 256;                 // tracks per tile of the cell kernel: one candidate, 256 consecutive tracks
constexpr int TRIAL_SUMMARY = 4;                // summary [4][G]: pcMax, pcArg, dcpaMin, dcpaArg

struct TrialOwn {
    double p0[2], v0[2], S[3], w;      // position, velocity, the position covariance (xx, xy, yy), the turn rate
};

// Candidate (dpsi, f, t0) as entry e of nt: pos [K + 1][2][nt], S [K + 1][3][nt]
MHT_HD void trial_candidate(const TrialOwn& o, double dpsi, double f, double t0, int nt, int K, double dt, int e, double* pos, double* S) {
    const size_t nn = (size_t)nt;
    const double nan = __builtin_nan("");
    const double p0x = o.p0[0], p0y = o.p0[1], v0x = o.v0[0], v0y = o.v0[1], w = o.w;
    bool there = dpsi == dpsi && f == f && t0 == t0 && p0x == p0x && p0y == p0y && v0x == v0x && v0y == v0y;
    there = there && o.S[0] == o.S[0] && o.S[1] == o.S[1] && o.S[2] == o.S[2];
    const double ad = fabs(dpsi), sg = dpsi > 0.0 ? 1.0 : (dpsi < 0.0 ? -1.0 : 0.0);
    const double te = t0 + ad / w;
    const double ax = p0x + t0 * v0x, ay = p0y + t0 * v0y;
    const double se = sin(ad), ce = cos(ad);
    const double swe = se / w, cwe = (1.0 - ce) / w;
    const double bx = ax + f * (swe * v0x - (sg * cwe) * v0y), by = ay + f * ((sg * cwe) * v0x + swe * v0y);
    const double ux = f * (ce * v0x - (sg * se) * v0y), uy = f * ((sg * se) * v0x + ce * v0y);
    for (int k = 0; k <= K; ++k) {
        const double t = (double)k * dt;
        double px, py;
        if (t <= t0) {
            px = p0x + t * v0x;
            py = p0y + t * v0y;
        } else if (t <= te) {
            const double tau = t - t0;
            const double s = sin(w * tau), c = cos(w * tau);
            const double sw = s / w, cw = (1.0 - c) / w;
            px = ax + f * (sw * v0x - (sg * cw) * v0y);
            py = ay + f * ((sg * cw) * v0x + sw * v0y);
        } else {
            const double r = t - te;
            px = bx + r * ux;
            py = by + r * uy;
        }
        double* p = pos + (size_t)k * 2 * nn + e;
        double* s = S + (size_t)k * 3 * nn + e;
        p[0] = there ? px : nan;
        p[nn] = there ? py : nan;
        s[0] = there ? o.S[0] : nan;
        s[nn] = there ? o.S[1] : nan;
        s[2 * nn] = there ? o.S[2] : nan;
    }
}

// Track t of n: its x [N][n] and P [N (N + 1) / 2][n] copied into the staging of stride nt, xs [N][nt] and Ps [N (N + 1) / 2][nt] --
// encounter_propagate reads its entry with the stride it writes the trajectories with -- and propagated as entry t of nt
template <int N>
MHT_HD void trial_track(const EncounterModel<N>& m, const double* x, const double* P, int n, int nt, int K, int t, double* xs, double* Ps,
                        double* pos, double* S) {
    constexpr int NS = N * (N + 1) / 2;
#pragma unroll
    for (int i = 0; i < N; ++i) xs[(size_t)i * (size_t)nt + t] = x[(size_t)i * (size_t)n + t];
#pragma unroll
    for (int i = 0; i < NS; ++i) Ps[(size_t)i * (size_t)nt + t] = P[(size_t)i * (size_t)n + t];
    encounter_propagate<N>(m, xs, Ps, nt, K, t, pos, S);
}

// What a fold keeps: the largest pc and the smallest dcpa, each with its track (-1: none yet)
struct TrialBest {
    double pc, dcpa;
    int pcj, dj;
};

MHT_HD TrialBest trial_none() { return TrialBest{__builtin_nan(""), __builtin_nan(""), -1, -1}; }

// A cell's two figures as a fold of one: a NaN figure is none
MHT_HD TrialBest trial_cell_best(double pc, double dcpa, int j) { return TrialBest{pc, dcpa, pc == pc ? j : -1, dcpa == dcpa ? j : -1}; }

// a <- the better of a and b, per figure, by explicit selects: none loses; the larger pc (the smaller dcpa) wins; equal figures: the
// lower track
MHT_HD void trial_fold(TrialBest& a, const TrialBest& b) {
    const bool tp = b.pcj >= 0 && (a.pcj < 0 || b.pc > a.pc || (b.pc == a.pc && b.pcj < a.pcj));
    a.pc = tp ? b.pc : a.pc;
    a.pcj = tp ? b.pcj : a.pcj;
    const bool td = b.dj >= 0 && (a.dj < 0 || b.dcpa < a.dcpa || (b.dcpa == a.dcpa && b.dj < a.dj));
    a.dcpa = td ? b.dcpa : a.dcpa;
    a.dj = td ? b.dj : a.dj;
}

// A fold as four doubles at q[0], q[stride], q[2 stride], q[3 stride]: pc, its track, dcpa, its track (NaN and -1: none)
MHT_HD void trial_store(const TrialBest& a, double* q, size_t stride) {
    q[0] = a.pcj >= 0 ? a.pc : __builtin_nan("");
    q[stride] = (double)a.pcj;
    q[2 * stride] = a.dj >= 0 ? a.dcpa : __builtin_nan("");
    q[3 * stride] = (double)a.dj;
}

MHT_HD TrialBest trial_load(const double* q, size_t stride) { return TrialBest{q[0], q[2 * stride], (int)q[stride], (int)q[3 * stride]}; }

// Cell (g, j) of out [5][G][n]: candidate g is entry n + g of nt = n + G.  Returns the cell as a fold of one.
MHT_HD TrialBest trial_cell(const double* pos, const double* S, int n, int G, int K, double dt, double R, int g, int j, double* out) {
    double o[ENCOUNTER_FIGURES];
    encounter_pair(pos, S, n + G, K, dt, R, n + g, j, o);
    double* cell = out + (size_t)g * (size_t)n + j;
#pragma unroll
    for (int f = 0; f < ENCOUNTER_FIGURES; ++f) cell[(size_t)f * (size_t)G * (size_t)n] = o[f];
    return trial_cell_best(o[3], o[1], j);
}

}  // namespace mht
