// TEST-ONLY host build of csrc/mht_mc.h: mc_philox, mc_normals, mc_factor, mc_component and mc_walk themselves -- what a lane of the
// kernels of mht_mc.hip runs per component and per particle -- compiled for the CPU and run over a call in the seam's own layouts, the
// particles of a target as a loop and the wavefronts' ballots as plain increments, so that the generator, the factor, the pick, both
// walks and the counts are checked against tests/mc_ref.py without a GPU (tests/test_mc_cpu.py), and the seam against this twin
// (tests/test_mc_gpu.py).  tests/hostmath/mc_host_main.cpp makes a stand-alone program of it for a sanitizer build.
#include "mc_host_common.h"

namespace {

struct HostSink {      // one particle at a time: a ballot's popcount is 0 or 1
    uint32_t* w;       // within [G][K + 1][T] at target t
    uint32_t* e;       // ever [G][T] at target t
    size_t T;
    int K, k = 0;
    void within(int g, bool in) { w[((size_t)g * (size_t)(K + 1) + (size_t)k) * T] += in ? 1u : 0u; }
    void step_done(int) { ++k; }
    void ever(int g, bool in) { e[(size_t)g * T] += in ? 1u : 0u; }
    void particle_done() { k = 0; }
};

template <int N, bool CT>
int run(int32_t nComp, int32_t T, int32_t G, int32_t K, int32_t S, uint64_t seed, double dt, double R, const double* Phi, const double* Q, const double* x,
        const double* P, const int32_t* first, const double* cdf, const double* own, uint32_t* within, uint32_t* ever, uint32_t* valid, int32_t* status) {
    McModel<N> m;
    std::vector<double> Lw;
    std::vector<int32_t> tst;
    if (!prepare<N, CT>(nComp, T, dt, R, Phi, Q, x, P, first, cdf, m, Lw, tst)) return -1;
    for (size_t i = 0; i < (size_t)G * (size_t)(K + 1) * (size_t)T; ++i) within[i] = 0;
    for (size_t i = 0; i < (size_t)G * (size_t)T; ++i) ever[i] = 0;
    for (int t = 0; t < T; ++t) {
        status[t] = tst[t];
        valid[t] = status[t] == 0 ? (uint32_t)S : 0u;
        if (status[t] != 0) continue;
        HostSink sink{within + t, ever + t, (size_t)T, K};
        for (int32_t p = 0; p < S; ++p)      // a lane's particle
            mc_walk<N, CT>(m, x, Lw.data(), first, cdf, own, nComp, G, K, seed, t, (uint32_t)p, true, sink);
    }
    return 0;
}

// The states of one walk from x0 with the noise of (particle, target): out [K + 1][N]
template <int N, bool CT>
int path(int32_t K, double dt, const double* Phi, const double* Q, const double* x0, uint64_t seed, uint32_t particle, uint32_t target, double* out) {
    McModel<N> m;
    if (!mc_model<N>(CT ? nullptr : Phi, Q, dt, 0.0, m)) return -1;
    double X[N], z[N];
    for (int i = 0; i < N; ++i) out[i] = X[i] = x0[i];
    for (int k = 1; k <= K; ++k) {
        mc_normals<N>(particle, (uint32_t)k, target, seed, z);
        mc_step<N, CT>(m, z, X);
        for (int i = 0; i < N; ++i) out[k * N + i] = X[i];
    }
    return 0;
}

}  // namespace

extern "C" void mc_philox_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
    const McRand r = mc_philox(c0, c1, c2, c3, k0, k1);
    for (int i = 0; i < 4; ++i) out[i] = r.v[i];
}

extern "C" void mc_normals_host(int32_t nx, uint32_t particle, uint32_t step, uint32_t target, uint64_t seed, double* z) {
    if (nx == 4) mc_normals<4>(particle, step, target, seed, z);
    else mc_normals<6>(particle, step, target, seed, z);
}

// A [nx][nx] row-major -> L [nx][nx] row-major, lower; own: Q's tolerance.  Returns the status.
extern "C" int mc_factor_host(int32_t nx, int32_t own, const double* A, double* L) {
    double packed[21];
    int st;
    if (nx == 4) st = own ? mc_factor<4, true>(A, packed) : mc_factor<4, false>(A, packed);
    else st = own ? mc_factor<6, true>(A, packed) : mc_factor<6, false>(A, packed);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j) L[i * nx + j] = j <= i ? packed[i * (i + 1) / 2 + j] : 0.0;
    return st;
}

extern "C" void mc_chunks_host(int32_t T, int32_t S, int32_t* out) {
    const McSplit s = mc_chunks(T, S);
    out[0] = s.chunks;
    out[1] = s.slab;
}

// The states of ONE walk from x0 [nx] (no draw of X_0) with the noise of (particle, target): out [K + 1][nx]
extern "C" int mc_path_host(int32_t nx, int32_t transition, int32_t K, double dt, const double* Phi, const double* Q, const double* x0, uint64_t seed,
                            uint32_t particle, uint32_t target, double* out) {
    return mc_dispatch(nx, transition, [&](auto n, auto ct) { return path<decltype(n)::value, decltype(ct)::value>(K, dt, Phi, Q, x0, seed, particle, target, out); });
}

// The seam's arguments on host arrays.  Returns 0, or -1 where the seam refuses (nothing written).
extern "C" int mc_encounters_host(int32_t nx, int32_t transition, int32_t nComp, int32_t T, int32_t G, int32_t K, int32_t S, uint64_t seed, double dt, double R,
                                  const double* Phi, const double* Q, const double* x, const double* P, const int32_t* first, const double* cdf,
                                  const double* own, uint32_t* within, uint32_t* ever, uint32_t* valid, int32_t* status) {
    if (!fits(nx, transition, nComp, T, K, dt, R, Phi, Q, first) || !particles_fit(S) || G < 1 || G > MC_MAX_PATHS) return -1;
    return mc_dispatch(nx, transition, [&](auto n, auto ct) {
        return run<decltype(n)::value, decltype(ct)::value>(nComp, T, G, K, S, seed, dt, R, Phi, Q, x, P, first, cdf, own, within, ever, valid, status);
    });
}
