// TEST-ONLY host build of csrc/mht_mc_domain.h: mc_domain_walk itself -- what a lane of mc_domain_walk_kernel (mht_mc_domain.hip) runs
// per particle -- and mht_mc.h's mc_component, compiled for the CPU and run over a call in the seam's own layouts, the particles of a
// target as a loop, the wavefronts' ballots as plain increments and the wavefront-wide skip of a far cell as the particle's own, so
// that the domain engine's counts are checked against tests/mc_domain_ref.py without a GPU (tests/test_mc_domain_cpu.py), and the seam
// against this twin (tests/test_mc_domain_gpu.py).  tests/hostmath/mc_domain_host_main.cpp makes a stand-alone program of it for a
// sanitizer build.
#include "mc_host_common.h"
#include "../../pymht_amd/csrc/mht_mc_domain.h"

namespace {

struct DomainCountSink {      // one particle at a time: a ballot's popcount is 0 or 1
    uint32_t* in;             // inside [nCell][K + 1][T] at target t
    uint32_t* fa;             // firstAt [nCell][K + 1][T] at target t
    uint32_t* ev;             // ever [nCell][T] at target t
    size_t K1, T;
    bool skip;                // false: every cell's edge loop is run, near or not
    void path(int, const double*) {}
    bool any(bool near) { return near || !skip; }
    void step(int c, int k, bool inside, bool first) {
        in[((size_t)c * K1 + (size_t)k) * T] += inside ? 1u : 0u;
        fa[((size_t)c * K1 + (size_t)k) * T] += first ? 1u : 0u;
    }
    void step_done(int) {}
    void ever(int c, bool came) { ev[(size_t)c * T] += came ? 1u : 0u; }
    void particle_done() {}
};

// The seam's checks of the cells, the domains and the poses; the boxes [nDomain][4] where they pass
bool domains_fit(int32_t G, int32_t nDomain, int32_t nVert, int32_t K, const double* pose, const int32_t* domFirst, const double* domXY, std::vector<double>& box) {
    if (nDomain < 1 || nDomain > MC_DOMAIN_MAX_DOMAINS || G < 1 || nDomain * (int64_t)G > MC_DOMAIN_MAX_CELLS) return false;
    if (nVert < MC_ZONE_MIN_VERTS * nDomain || nVert > MC_DOMAIN_MAX_VERTS) return false;
    if (domFirst[0] != 0 || domFirst[nDomain] != nVert) return false;
    for (int d = 0; d < nDomain; ++d)
        if (domFirst[d + 1] < domFirst[d] + MC_ZONE_MIN_VERTS) return false;
    for (int i = 0; i < 2 * nVert; ++i)
        if (!mc_finite(domXY[i])) return false;
    for (size_t i = 0; i < (size_t)G * (size_t)(K + 1) * 4; i += 4) {
        if (!mc_finite(pose[i]) || !mc_finite(pose[i + 1]) || !mc_finite(pose[i + 2]) || !mc_finite(pose[i + 3])) return false;
        if (!(fabs(pose[i + 2] * pose[i + 2] + pose[i + 3] * pose[i + 3] - 1.0) <= MC_DOMAIN_UNIT_TOL)) return false;
    }
    box.assign((size_t)nDomain * 4, 0.0);
    for (int d = 0; d < nDomain; ++d) mc_zone_box(domXY, domFirst[d], domFirst[d + 1], box.data() + 4 * d);      // a lane's domain
    return true;
}

template <int N, bool CT>
int run(int32_t nComp, int32_t T, int32_t G, int32_t K, int32_t S, uint64_t seed, double dt, const double* Phi, const double* Q, const double* x, const double* P,
        const int32_t* first, const double* cdf, const double* pose, const McDomains& ds, bool skip, uint32_t* inside, uint32_t* firstAt, uint32_t* ever,
        uint32_t* valid, int32_t* status) {
    McModel<N> m;
    std::vector<double> Lw;
    std::vector<int32_t> tst;
    if (!prepare<N, CT>(nComp, T, dt, 1.0, Phi, Q, x, P, first, cdf, m, Lw, tst)) return -1;
    const size_t nT = (size_t)T, K1 = (size_t)K + 1, nCell = (size_t)ds.nDomain * (size_t)G;
    for (size_t i = 0; i < nCell * K1 * nT; ++i) inside[i] = firstAt[i] = 0;
    for (size_t i = 0; i < nCell * nT; ++i) ever[i] = 0;
    for (int t = 0; t < T; ++t) {
        status[t] = tst[t];
        valid[t] = tst[t] == 0 ? (uint32_t)S : 0u;
        if (tst[t] != 0) continue;
        DomainCountSink sink{inside + t, firstAt + t, ever + t, K1, nT, skip};
        for (int32_t p = 0; p < S; ++p)      // a lane's particle
            mc_domain_walk<N, CT>(m, x, Lw.data(), first, cdf, pose, nComp, G, K, seed, t, (uint32_t)p, true, ds, sink);
    }
    return 0;
}

}  // namespace

// The seam's arguments on host arrays (skip 0: every cell's edge loop is run, near or not -- the same counts are expected).  Returns 0,
// or -1 where the seam refuses (nothing written).
extern "C" int mc_domain_encounters_host(int32_t nx, int32_t transition, int32_t nComp, int32_t T, int32_t G, int32_t nDomain, int32_t nVert, int32_t K, int32_t S,
                                         uint64_t seed, double dt, const double* Phi, const double* Q, const double* x, const double* P, const int32_t* first,
                                         const double* cdf, const double* ownPose, const int32_t* domFirst, const double* domXY, int32_t skip, uint32_t* inside,
                                         uint32_t* firstAt, uint32_t* ever, uint32_t* valid, int32_t* status) {
    std::vector<double> box;
    if (!fits(nx, transition, nComp, T, K, dt, 1.0, Phi, Q, first) || !particles_fit(S) || !domains_fit(G, nDomain, nVert, K, ownPose, domFirst, domXY, box)) return -1;
    const McDomains ds = {domFirst, domXY, box.data(), nDomain};
    return mc_dispatch(nx, transition, [&](auto n, auto ct) {
        return run<decltype(n)::value, decltype(ct)::value>(nComp, T, G, K, S, seed, dt, Phi, Q, x, P, first, cdf, ownPose, ds, skip != 0, inside, firstAt, ever, valid,
                                                            status);
    });
}

// The transform on its own: (x, y) in the body frame of pose [4].  out: qx, qy
extern "C" void mc_domain_body_host(const double* pose, double x, double y, double* out) { mc_domain_body(pose, x, y, out[0], out[1]); }
