// TEST-ONLY host build of csrc/mht_mc_zone.h: mc_zone_walk itself -- what a lane of mc_zone_walk_kernel (mht_mc_zone.hip) runs per
// particle -- and mht_mc.h's mc_component, compiled for the CPU and run over a call in the seam's own layouts, the particles of a target
// as a loop, the wavefronts' ballots as plain increments and the wavefront-wide skip of a far zone as the particle's own, so that the
// zone engine's counts are checked against tests/mc_zone_ref.py without a GPU (tests/test_mc_zone_cpu.py), and the seam against this twin
// (tests/test_mc_zone_gpu.py).  tests/hostmath/mc_zone_host_main.cpp makes a stand-alone program of it for a sanitizer build.
#include "mc_host_common.h"
#include "../../pymht_amd/csrc/mht_mc_zone.h"

namespace {

struct ZoneCountSink {      // one particle at a time: a ballot's popcount is 0 or 1
    uint32_t* in;           // inside [nZone][K + 1][T] at target t
    uint32_t* fa;           // firstAt [nZone][K + 1][T] at target t
    uint32_t* ev;           // ever [nZone][T] at target t
    size_t K1, T;
    void path(int, const double*) {}
    bool any(bool near) { return near; }
    void step(int z, int k, bool inside, bool first) {
        in[((size_t)z * K1 + (size_t)k) * T] += inside ? 1u : 0u;
        fa[((size_t)z * K1 + (size_t)k) * T] += first ? 1u : 0u;
    }
    void step_done(int) {}
    void ever(int z, bool came) { ev[(size_t)z * T] += came ? 1u : 0u; }
    void particle_done() {}
};

template <int N>
struct ZonePathSink {       // one particle: its states and its flags; skip false: every zone's edge loop is run, near or not
    double* states;         // [K + 1][N]
    int32_t* flags;         // [nZone][K + 1][2]: in_k; k is the first step with hit_k.  Then [nZone]: came
    int K, nZone;
    bool skip;
    void path(int k, const double* X) {
        for (int i = 0; i < N; ++i) states[(size_t)k * N + i] = X[i];
    }
    bool any(bool near) { return near || !skip; }
    void step(int z, int k, bool inside, bool first) {
        flags[((size_t)z * (K + 1) + k) * 2] = inside ? 1 : 0;
        flags[((size_t)z * (K + 1) + k) * 2 + 1] = first ? 1 : 0;
    }
    void step_done(int) {}
    void ever(int z, bool came) { flags[(size_t)nZone * (K + 1) * 2 + z] = came ? 1 : 0; }
    void particle_done() {}
};

// The seam's checks of the zones; the boxes [nZone][4] where they pass
bool zones_fit(int32_t nZone, int32_t nVert, const int32_t* zoneFirst, const double* zoneXY, std::vector<double>& box) {
    if (nZone < 1 || nZone > MC_ZONE_MAX_ZONES || nVert < MC_ZONE_MIN_VERTS * nZone || nVert > MC_ZONE_MAX_VERTS) return false;
    if (zoneFirst[0] != 0 || zoneFirst[nZone] != nVert) return false;
    for (int z = 0; z < nZone; ++z)
        if (zoneFirst[z + 1] < zoneFirst[z] + MC_ZONE_MIN_VERTS) return false;
    for (int i = 0; i < 2 * nVert; ++i)
        if (!mc_finite(zoneXY[i])) return false;
    box.assign((size_t)nZone * 4, 0.0);
    for (int z = 0; z < nZone; ++z) mc_zone_box(zoneXY, zoneFirst[z], zoneFirst[z + 1], box.data() + 4 * z);      // a lane's zone
    return true;
}

template <int N, bool CT>
int run(int32_t nComp, int32_t T, int32_t K, int32_t S, uint64_t seed, double dt, const double* Phi, const double* Q, const double* x, const double* P,
        const int32_t* first, const double* cdf, const McZones& zs, uint32_t* inside, uint32_t* firstAt, uint32_t* ever, uint32_t* valid, int32_t* status) {
    McModel<N> m;
    std::vector<double> Lw;
    std::vector<int32_t> tst;
    if (!prepare<N, CT>(nComp, T, dt, 1.0, Phi, Q, x, P, first, cdf, m, Lw, tst)) return -1;
    const size_t nT = (size_t)T, K1 = (size_t)K + 1, cells = (size_t)zs.nZone * K1;
    for (size_t i = 0; i < cells * nT; ++i) inside[i] = firstAt[i] = 0;
    for (size_t i = 0; i < (size_t)zs.nZone * nT; ++i) ever[i] = 0;
    for (int t = 0; t < T; ++t) {
        status[t] = tst[t];
        valid[t] = tst[t] == 0 ? (uint32_t)S : 0u;
        if (tst[t] != 0) continue;
        ZoneCountSink sink{inside + t, firstAt + t, ever + t, K1, nT};
        for (int32_t p = 0; p < S; ++p)      // a lane's particle
            mc_zone_walk<N, CT>(m, x, Lw.data(), first, cdf, nComp, K, seed, t, (uint32_t)p, true, zs, sink);
    }
    return 0;
}

template <int N, bool CT>
int one(int32_t nComp, int32_t T, int32_t K, uint64_t seed, double dt, const double* Phi, const double* Q, const double* x, const double* P, const int32_t* first,
        const double* cdf, const McZones& zs, int32_t t, uint32_t p, bool skip, double* states, int32_t* flags) {
    McModel<N> m;
    std::vector<double> Lw;
    std::vector<int32_t> tst;
    if (!prepare<N, CT>(nComp, T, dt, 1.0, Phi, Q, x, P, first, cdf, m, Lw, tst)) return -1;
    if (tst[t] != 0) return -2;
    ZonePathSink<N> sink{states, flags, K, zs.nZone, skip};
    mc_zone_walk<N, CT>(m, x, Lw.data(), first, cdf, nComp, K, seed, t, p, true, zs, sink);
    return 0;
}

}  // namespace

// The seam's arguments on host arrays.  Returns 0, or -1 where the seam refuses (nothing written).
extern "C" int mc_zone_encounters_host(int32_t nx, int32_t transition, int32_t nComp, int32_t T, int32_t nZone, int32_t nVert, int32_t K, int32_t S, uint64_t seed,
                                       double dt, const double* Phi, const double* Q, const double* x, const double* P, const int32_t* first, const double* cdf,
                                       const int32_t* zoneFirst, const double* zoneXY, uint32_t* inside, uint32_t* firstAt, uint32_t* ever, uint32_t* valid,
                                       int32_t* status) {
    std::vector<double> box;
    if (!fits(nx, transition, nComp, T, K, dt, 1.0, Phi, Q, first) || !particles_fit(S) || !zones_fit(nZone, nVert, zoneFirst, zoneXY, box)) return -1;
    const McZones zs = {zoneFirst, zoneXY, box.data(), nZone};
    return mc_dispatch(nx, transition, [&](auto n, auto ct) {
        return run<decltype(n)::value, decltype(ct)::value>(nComp, T, K, S, seed, dt, Phi, Q, x, P, first, cdf, zs, inside, firstAt, ever, valid, status);
    });
}

// ONE particle: its states [K + 1][nx] and flags [nZone][K + 1][2] (in_k; step k is the first with hit_k) followed by [nZone] (came at
// all).  skip 0: every zone's edge loop is run, whether the particle is near the zone or not -- the same flags are expected.  Returns 0;
// -1 where the seam refuses; -2 for a target that is not scored.
extern "C" int mc_zone_path_host(int32_t nx, int32_t transition, int32_t nComp, int32_t T, int32_t nZone, int32_t nVert, int32_t K, uint64_t seed, double dt,
                                 const double* Phi, const double* Q, const double* x, const double* P, const int32_t* first, const double* cdf,
                                 const int32_t* zoneFirst, const double* zoneXY, int32_t t, uint32_t particle, int32_t skip, double* states, int32_t* flags) {
    std::vector<double> box;
    if (!fits(nx, transition, nComp, T, K, dt, 1.0, Phi, Q, first) || !zones_fit(nZone, nVert, zoneFirst, zoneXY, box) || t < 0 || t >= T) return -1;
    const McZones zs = {zoneFirst, zoneXY, box.data(), nZone};
    return mc_dispatch(nx, transition, [&](auto n, auto ct) {
        return one<decltype(n)::value, decltype(ct)::value>(nComp, T, K, seed, dt, Phi, Q, x, P, first, cdf, zs, t, particle, skip != 0, states, flags);
    });
}

// The predicates on their own, for hand-stated cases: poly [n][2] against the segment p -> q (segment 0: the point q alone).  out:
// in, cross.  Returns 0, or -1 for a polygon the seam would refuse.
extern "C" int mc_zone_test_host(int32_t n, const double* poly, double px, double py, double qx, double qy, int32_t segment, int32_t* out) {
    std::vector<double> box;
    const int32_t zf[2] = {0, n};
    if (!zones_fit(1, n, zf, poly, box)) return -1;
    bool in = false, cross = false;
    mc_zone_test(poly, 0, n, box.data(), px, py, qx, qy, segment != 0, in, cross);
    out[0] = in ? 1 : 0;
    out[1] = cross ? 1 : 0;
    return 0;
}
