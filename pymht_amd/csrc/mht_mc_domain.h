// SHIP DOMAINS by Monte Carlo (mht_mc_domain_encounters, include/mht_amd.h): will a target enter the own ship's DOMAIN -- the safety
// region around the own ship, which is no disc: longer ahead than astern, usually wider to starboard than to port --, with what
// probability within the horizon, and when, for every candidate path of the own ship.  A domain is a polygon drawn in the own ship's
// BODY FRAME; it translates and rotates with the ship, so a candidate manoeuvre moves it.  The engine is mht_mc.h's: the forest's own
// leaves sampled as a mixture per target, every particle walked with process noise and, under the constant-turn model, with Phi(dt, w)
// of its own turn rate.  This header includes mht_mc_zone.h and uses mc_zone_test, mc_zone_box, mc_philox, mc_normals, mc_pick, mc_draw
// and mc_step<N, CT> unchanged; what it adds is the transform into the body frame per (path, step) and a walk that counts per (domain,
// path, step).  The code a lane of mc_domain_walk_kernel (mht_mc_domain.hip) runs per particle, and tests/hostmath/mc_domain_host.cpp on
// the CPU.  A definition, not a measurement: the library is compiled with -ffp-contract=off, and every operation below is written out
// in one order, the order tests/mc_domain_ref.py restates.
//
// PARTICLES.  Particle p of target t is EXACTLY mc_walk's particle -- the same counter words, the same pick of a component, the same
// order of every sum.
//
// DOMAINS.  nDomain simple polygons, 1 .. MC_DOMAIN_MAX_DOMAINS (an inner "collision" and an outer "comfort" domain, say); domain d owns
// the vertices domFirst[d] .. domFirst[d + 1] - 1 of domXY [nVert][2], float64 metres in the own ship's body frame: THE FIRST
// COORDINATE IS TO THE RIGHT OF THE HEADING, THE SECOND AHEAD.  With the tracker's axes read as x east and y north that is starboard
// and ahead: a domain is drawn bow-up.  At least three vertices each, at most MC_DOMAIN_MAX_VERTS in all; either orientation, concave
// allowed, no holes.  The domain's box is mc_zone_box's.
//
// POSES.  ownPose [G][K + 1][4] = (ox, oy, ux, uy) per path and step: the own ship's position and its UNIT HEADING VECTOR.  A vector and
// not an angle: no sin or cos is evaluated for the transform.
//
// CELLS.  A (domain, path) is a cell, c = d * G + g; nCell = nDomain * G <= MC_DOMAIN_MAX_CELLS = 64: one lane of a wavefront owns one
// cell.  G >= 1.
//
// THE BODY-FRAME POINT of X_k under pose (g, k), in this order (mc_domain_body):
//   dx = X_k[0] - ox, dy = X_k[1] - oy
//   qx = dx * uy - dy * ux
//   qy = dx * ux + dy * uy
//
// PER STEP, for a cell: in_k is mc_zone_test's point test of q_k against the domain; cross_k (k >= 1) its segment test of q_{k-1} -> q_k,
// q_{k-1} taken under pose (g, k - 1) and q_k under pose (g, k); hit_k = in_k || cross_k.
// THE BODY-FRAME PATH BETWEEN TWO STEPS IS TAKEN AS STRAIGHT.  That is the relative path exactly when the own ship does not turn between
// the two steps; on a step inside an arc it is a chord of a curved path.  This is part of the definition, not an error of it: shorter
// steps during a manoeuvre are the remedy.
// The walk keeps X_{k-1}[0:2] -- two doubles -- and recomputes q_{k-1} for every path from it, with the same operations and therefore
// the same bits: keeping 64 previous body-frame points per lane would cost 256 vector registers.
//
// COUNTS, per (domain, path, target):
//   inside[d][g][k][t]    the particles with in_k
//   firstAt[d][g][k][t]   the particles whose smallest k with hit_k is k
//   ever[d][g][t]         the particles with any hit_k
// By construction sum_k firstAt == ever and ever >= max_k inside.  valid [T], status [T] and the split mc_chunks(T, S) are the engine's.
//
// THE SKIP.  A cell is skipped where the box of the segment q_{k-1} -> q_k (of the point q_0 at k = 0) does not overlap the domain's
// box; exact for the reason mht_mc_zone.h gives (an edge's box lies in its domain's, and q_k is a corner of the segment's box).  The
// walk asks its sink whether ANY of the particles walked together is near (sink.any): a wavefront's ballot on the device, the particle
// itself on the host.  There is NO FURTHER CULL: no distance test in front of the rotation, nothing that is not written here.
//
// OUT OF SCOPE: domains around targets or between pairs of targets, a domain that scales with speed, the own ship's covariance, a
// curved body-frame path inside a turning step, holes, more than 64 cells, a stationary own ship (it has no heading).
#pragma once
#include "mht_mc_zone.h"

namespace mht {

constexpr int MC_DOMAIN_MAX_DOMAINS = 4;      // MHT_MC_DOMAIN_MAX_DOMAINS of include/mht_amd.h
constexpr int MC_DOMAIN_MAX_VERTS = 256;      // MHT_MC_DOMAIN_MAX_VERTS: all domains together
constexpr int MC_DOMAIN_MAX_CELLS = 64;       // MHT_MC_DOMAIN_MAX_CELLS: nDomain * G, a lane of a wavefront per cell
constexpr double MC_DOMAIN_UNIT_TOL = 1e-9;   // |ux^2 + uy^2 - 1| of a heading the seam admits

// The domains of a call as a walk reads them (LDS on the device): first [nDomain + 1], xy [nVert][2], box [nDomain][4]
struct McDomains {
    const int32_t* first;
    const double* xy;
    const double* box;
    int nDomain;
};

// (x, y) in the body frame of the pose o = (ox, oy, ux, uy)
MHT_HD void mc_domain_body(const double* o, double x, double y, double& qx, double& qy) {
    const double dx = x - o[0], dy = y - o[1];
    qx = dx * o[3] - dy * o[2];
    qy = dx * o[2] + dy * o[3];
}

// Particle p of target t against every cell.  `live` false: a lane beyond the slab's end, which walks along and counts nowhere.  The
// sink takes
//   any(near)                 is one of the particles walked together near the domain?  (decides the skip; does not move a result)
//   step(c, k, in, first)     per step and cell c = d * G + g, g = 0 .. G - 1 in turn and, inside (one transform serves a path's
//                             domains), d = 0 .. nDomain - 1: in_k; k is the first step with hit_k.  Then step_done(k)
//   ever(c, came)             at the end, c = 0 .. nCell - 1 in turn: any hit_k.  Then particle_done()
// and may keep the particle's state at every step (path(k, X): the host twin's; nothing on the device).
template <int N, bool CT, class Sink>
MHT_HD void mc_domain_walk(const McModel<N>& m, const double* x, const double* Lw, const int32_t* first, const double* cdf, const double* pose, int nComp, int G,
                           int K, uint64_t seed, int t, uint32_t p, bool live, const McDomains& ds, Sink& sink) {
    const size_t nn = (size_t)nComp;
    double X[N], z[N];
    const McRand pick = mc_philox(p, MC_PICK_STEP, (uint32_t)t, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int c = mc_pick(cdf, first[t], first[t + 1] - 1, mc_uniform(pick.v[0]));
    uint64_t came = 0;      // bit c: some hit_k of cell c
    double lx = 0.0, ly = 0.0;      // X_{k-1}[0:2]
    int k = 0;
    do {      // (K >= 1, G >= 1 and nDomain >= 1, the seam's ranges: loops without a guard in front)
        mc_normals<N>(p, (uint32_t)k, (uint32_t)t, seed, z);
        if (k == 0) mc_draw<N>(x, Lw, nn, c, z, X);
        else mc_step<N, CT>(m, z, X);
        sink.path(k, X);
        if (k == 0) {
            lx = X[0];
            ly = X[1];
        }
        int g = 0;
        do {
            const double* o = pose + ((size_t)g * (size_t)(K + 1) + (size_t)k) * 4;
            double px, py, qx, qy;
            mc_domain_body(o, X[0], X[1], qx, qy);
            mc_domain_body(k > 0 ? o - 4 : o, lx, ly, px, py);      // (k = 0: the point itself, the same bits as q)
            const double sx0 = fmin(px, qx), sx1 = fmax(px, qx), sy0 = fmin(py, qy), sy1 = fmax(py, qy);
            int d = 0;
            do {
                const double* box = ds.box + 4 * d;
                const int cell = d * G + g;
                const bool near = sx0 <= box[2] && sx1 >= box[0] && sy0 <= box[3] && sy1 >= box[1];
                bool in = false, cross = false;
                if (sink.any(near)) mc_zone_test(ds.xy, ds.first[d], ds.first[d + 1], box, px, py, qx, qy, k > 0, in, cross);
                const uint64_t hit = (in || cross) ? 1ull : 0ull;
                sink.step(cell, k, live && in, live && hit != 0ull && ((came >> cell) & 1ull) == 0ull);
                came |= hit << cell;
            } while (++d < ds.nDomain);
        } while (++g < G);
        sink.step_done(k);
        lx = X[0];
        ly = X[1];
    } while (++k <= K);
    const int nCell = ds.nDomain * G;
    int cell = 0;
    do sink.ever(cell, live && ((came >> cell) & 1ull) != 0ull);
    while (++cell < nCell);
    sink.particle_done();
}

}  // namespace mht
