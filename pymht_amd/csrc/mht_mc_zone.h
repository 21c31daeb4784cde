// GUARD ZONES by Monte Carlo (mht_mc_zone_encounters, include/mht_amd.h): will a target enter a PLACE -- a restricted area, a shoal
// contour, an anchorage, a traffic-separation zone --, with what probability within the horizon, and when.  The engine is mht_mc.h's:
// the forest's own leaves sampled as a mixture per target, every particle walked with process noise and, under the constant-turn model,
// with Phi(dt, w) of its own turn rate, counts that are the same bits for one seed.  This header includes mht_mc.h and uses mc_philox,
// mc_normals, mc_pick, mc_draw and mc_step<N, CT> unchanged; what it adds is the geometry -- a point in a polygon, a path segment
// against a polygon's edges -- and a walk that counts per (zone, step).  The code a lane of mc_zone_walk_kernel (mht_mc_zone.hip) runs
// per particle, and tests/hostmath/mc_zone_host.cpp on the CPU.  A definition, not a measurement: the library is compiled with
// -ffp-contract=off, and every operation below is written out in one order, the order tests/mc_zone_ref.py restates.
//
// ZONES.  nZone simple polygons; zone z owns the vertices zoneFirst[z] .. zoneFirst[z + 1] - 1 of zoneXY [nVert][2] (float64, metres,
// the frame of the states), at least three; the edge from its last vertex back to its first is implied.  Either orientation, concave
// polygons included; no holes.  The zone's BOX is the exact minimum and maximum of its vertices (fmin, fmax: no rounding).
//
// PARTICLES.  Particle p of target t is EXACTLY mc_walk's particle -- the same counter words (particle, step, target, block), the same
// pick of a component, the same order of every sum --, so it is the same particle whatever it is held against: an own path, another
// target or a zone.
//
// PER STEP, for the particle's positions X_k, k = 0 .. K, and a zone:
//   in_k      X_k lies in the zone's box (closed comparisons) AND the crossing number is odd: over the edges (a, b) in order, an edge
//             counts when (ay > py) != (by > py) and px < (bx - ax) * (py - ay) / (by - ay) + ax                        (p = X_k)
//   cross_k   k >= 1: some edge (a, b) meets ALL THREE of these against the segment from p = X_{k-1} to q = X_k
//               1. the closed boxes of the two segments overlap
//               2. o1 = ex * (ay - py) - ey * (ax - px) and o2 = ex * (by - py) - ey * (bx - px), e = q - p, do not have the same
//                  strict sign: (o1 >= 0 && o2 <= 0) || (o1 <= 0 && o2 >= 0)
//               3. the same for o3 = fx * (py - ay) - fy * (px - ax) and o4 = fx * (qy - ay) - fy * (qx - ax), f = b - a
//             Signs are compared, not products (a product of two tiny numbers underflows to 0 and would read as "on the line").  The
//             box test is PART of the definition: it is what makes collinear disjoint segments miss (their four o are all 0), and it
//             makes the skip below exact.
//   hit_k     in_k || cross_k
// A zone thinner than one step's travel is crossed between two steps: that is what cross_k is for.
//
// COUNTS, per (zone, target):
//   inside[z][k][t]    the particles with in_k
//   firstAt[z][k][t]   the particles whose smallest k with hit_k is k: the distribution of the time of entry
//   ever[z][t]         the particles with any hit_k
// By construction sum_k firstAt == ever and ever >= max_k inside.  valid [T] and status [T] are mht_mc_encounters' (mht_mc.h).
//
// THE SKIP.  The box of the segment X_{k-1} -> X_k (of the point X_0 at k = 0) either overlaps the zone's box or it does not.  Where it
// does not, no edge's box overlaps it -- an edge's box lies inside its zone's --, so cross_k is false, and X_k, a corner of the segment's
// box, is outside the zone's box, so in_k is false: the edge loop may be left out, and the result is the same bits.  The walk asks its
// sink whether ANY of the particles walked together is near (sink.any): a wavefront's ballot on the device, the particle itself on the
// host.  A particle that is carried through a loop it did not need gets false from every test in it.
//
// THE SPLIT is mc_chunks(T, S), as for the own-ship engine; the counts do not depend on it.
#pragma once
#include "mht_mc.h"

namespace mht {

constexpr int MC_ZONE_MAX_ZONES = 32;        // MHT_MC_ZONE_MAX_ZONES of include/mht_amd.h: a lane of half a wavefront per zone
constexpr int MC_ZONE_MAX_VERTS = 1024;      // MHT_MC_ZONE_MAX_VERTS: all zones together
constexpr int MC_ZONE_MIN_VERTS = 3;

// The zones of a call as a walk reads them (LDS on the device): first [nZone + 1], xy [nVert][2], box [nZone][4] = xmin, ymin, xmax, ymax
struct McZones {
    const int32_t* first;
    const double* xy;
    const double* box;
    int nZone;
};

// The box of the vertices lo .. hi - 1 (hi > lo)
MHT_HD void mc_zone_box(const double* xy, int lo, int hi, double* box) {
    double x0 = xy[2 * lo], y0 = xy[2 * lo + 1], x1 = x0, y1 = y0;
    for (int i = lo + 1; i < hi; ++i) {
        x0 = fmin(x0, xy[2 * i]);
        y0 = fmin(y0, xy[2 * i + 1]);
        x1 = fmax(x1, xy[2 * i]);
        y1 = fmax(y1, xy[2 * i + 1]);
    }
    box[0] = x0;
    box[1] = y0;
    box[2] = x1;
    box[3] = y1;
}

MHT_HD bool mc_zone_signs_part(double a, double b) { return (a >= 0.0 && b <= 0.0) || (a <= 0.0 && b >= 0.0); }

// Edge (a, b) in the crossing number of the point (px, py)
MHT_HD bool mc_zone_edge_counts(double ax, double ay, double bx, double by, double px, double py) {
    if ((ay > py) == (by > py)) return false;      // (an edge that counts has by != ay)
    return px < (bx - ax) * (py - ay) / (by - ay) + ax;
}

// Edge (a, b) against the segment p -> q
MHT_HD bool mc_zone_edge_crossed(double ax, double ay, double bx, double by, double px, double py, double qx, double qy) {
    const bool boxes = fmin(px, qx) <= fmax(ax, bx) && fmax(px, qx) >= fmin(ax, bx) && fmin(py, qy) <= fmax(ay, by) && fmax(py, qy) >= fmin(ay, by);
    const double ex = qx - px, ey = qy - py, fx = bx - ax, fy = by - ay;
    const double o1 = ex * (ay - py) - ey * (ax - px), o2 = ex * (by - py) - ey * (bx - px);
    const double o3 = fx * (py - ay) - fy * (px - ax), o4 = fx * (qy - ay) - fy * (qx - ax);
    return boxes && mc_zone_signs_part(o1, o2) && mc_zone_signs_part(o3, o4);
}

// in_k and cross_k of the segment p -> q (segment false: k = 0, the point q alone) for the zone of vertices lo .. hi - 1 and `box`
MHT_HD void mc_zone_test(const double* xy, int lo, int hi, const double* box, double px, double py, double qx, double qy, bool segment, bool& in, bool& cross) {
    uint32_t odd = 0u, met = 0u;      // (words of the lane, not predicates)
    double ax = xy[2 * (hi - 1)], ay = xy[2 * (hi - 1) + 1];
    // The edges in the order (last, first), (first, second), ...: the crossing number's parity and the OR over the edges do not depend
    // on where the round starts, and every vertex is read once.
    for (int i = lo; i < hi; ++i) {
        const double bx = xy[2 * i], by = xy[2 * i + 1];
        odd ^= mc_zone_edge_counts(ax, ay, bx, by, qx, qy) ? 1u : 0u;
        if (segment) met |= mc_zone_edge_crossed(ax, ay, bx, by, px, py, qx, qy) ? 1u : 0u;
        ax = bx;
        ay = by;
    }
    in = qx >= box[0] && qx <= box[2] && qy >= box[1] && qy <= box[3] && odd != 0u;
    cross = met != 0u;
}

// Particle p of target t against every zone.  `live` false: a lane beyond the slab's end, which walks along (the sink's ballots and
// barriers want every lane) and counts nowhere.  The sink takes
//   any(near)                 is one of the particles walked together near the zone?  (decides the skip; does not move a result)
//   step(z, k, in, first)     per step and zone, z = 0 .. nZone - 1 in turn: in_k; k is the first step with hit_k.  Then step_done(k)
//   ever(z, came)             at the end, z in turn: any hit_k.  Then particle_done()
// and may keep the particle's state at every step (path(k, X): the host twin's; nothing on the device).
template <int N, bool CT, class Sink>
MHT_HD void mc_zone_walk(const McModel<N>& m, const double* x, const double* Lw, const int32_t* first, const double* cdf, int nComp, int K, uint64_t seed, int t,
                         uint32_t p, bool live, const McZones& zs, Sink& sink) {
    const size_t nn = (size_t)nComp;
    double X[N], z[N];
    const McRand pick = mc_philox(p, MC_PICK_STEP, (uint32_t)t, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int c = mc_pick(cdf, first[t], first[t + 1] - 1, mc_uniform(pick.v[0]));
    uint32_t came = 0;      // bit z: some hit_k of zone z
    double px = 0.0, py = 0.0;
    int k = 0;
    do {      // (K >= 1 and nZone >= 1, the seam's ranges: loops without a guard in front)
        mc_normals<N>(p, (uint32_t)k, (uint32_t)t, seed, z);
        if (k == 0) mc_draw<N>(x, Lw, nn, c, z, X);
        else mc_step<N, CT>(m, z, X);
        sink.path(k, X);
        const double qx = X[0], qy = X[1];
        if (k == 0) {
            px = qx;
            py = qy;
        }
        const double sx0 = fmin(px, qx), sx1 = fmax(px, qx), sy0 = fmin(py, qy), sy1 = fmax(py, qy);
        int zi = 0;
        do {
            const double* box = zs.box + 4 * zi;
            const bool near = sx0 <= box[2] && sx1 >= box[0] && sy0 <= box[3] && sy1 >= box[1];
            bool in = false, cross = false;
            if (sink.any(near)) mc_zone_test(zs.xy, zs.first[zi], zs.first[zi + 1], box, px, py, qx, qy, k > 0, in, cross);
            const uint32_t hit = (in || cross) ? 1u : 0u;
            sink.step(zi, k, live && in, live && hit != 0u && ((came >> zi) & 1u) == 0u);
            came |= hit << zi;
        } while (++zi < zs.nZone);
        sink.step_done(k);
        px = qx;
        py = qy;
    } while (++k <= K);
    int zi = 0;
    do sink.ever(zi, live && ((came >> zi) & 1u) != 0u);
    while (++zi < zs.nZone);
    sink.particle_done();
}

}  // namespace mht
