// TEST-ONLY host build of csrc/mht_mc_pair.h: mc_pair_walk itself -- what a lane of mc_pair_walk_kernel (mht_mc.hip) runs per
// pair-particle -- and mht_mc.h's mc_component, compiled for the CPU and run over a call in the seam's own layouts, the particle
// indices of a pair as a loop and the wavefronts' ballots as plain increments, so that the pair engine's counts are checked against
// tests/mc_pair_ref.py without a GPU (tests/test_mc_pair_cpu.py), and the seam against this twin (tests/test_mc_pair_gpu.py).
// tests/hostmath/mc_pair_host_main.cpp makes a stand-alone program of it for a sanitizer build.
#include "mc_host_common.h"

namespace {

struct PairCountSink {      // one pair-particle at a time: a ballot's popcount is 0 or 1
    uint32_t* w;            // within [K + 1][nPair] at pair j
    uint32_t* f;            // firstAt [K + 1][nPair] at pair j
    uint32_t* e;            // ever [nPair] at pair j
    size_t nPair;
    void path(int, const double*, const double*, double, double) {}
    void step(int k, bool inside, bool first) {
        w[(size_t)k * nPair] += inside ? 1u : 0u;
        f[(size_t)k * nPair] += first ? 1u : 0u;
    }
    void done(bool came) { e[0] += came ? 1u : 0u; }
};

template <int N>
struct PairPathSink {       // one pair-particle: its two states, its relative path and its flags
    double* states;         // [K + 1][2][N]
    double* rel;            // [K + 1][2]
    int32_t* flags;         // [K + 1][2]: inside, first; then [1]: came
    int K;
    void path(int k, const double* Xa, const double* Xb, double dx, double dy) {
        for (int i = 0; i < N; ++i) {
            states[((size_t)k * 2) * N + i] = Xa[i];
            states[((size_t)k * 2 + 1) * N + i] = Xb[i];
        }
        rel[2 * k] = dx;
        rel[2 * k + 1] = dy;
    }
    void step(int k, bool inside, bool first) {
        flags[2 * k] = inside ? 1 : 0;
        flags[2 * k + 1] = first ? 1 : 0;
    }
    void done(bool came) { flags[2 * (K + 1)] = came ? 1 : 0; }
};

template <int N, bool CT>
int run(int32_t nComp, int32_t T, int32_t nPair, int32_t K, int32_t S, uint64_t seed, double dt, double R, const double* Phi, const double* Q, const double* x,
        const double* P, const int32_t* first, const double* cdf, const int32_t* pairs, uint32_t* within, uint32_t* firstAt, uint32_t* ever, uint32_t* valid,
        int32_t* status) {
    McModel<N> m;
    std::vector<double> Lw;
    std::vector<int32_t> tst;
    if (!prepare<N, CT>(nComp, T, dt, R, Phi, Q, x, P, first, cdf, m, Lw, tst)) return -1;
    const size_t nP = (size_t)nPair;
    for (size_t i = 0; i < (size_t)(K + 1) * nP; ++i) within[i] = firstAt[i] = 0;
    for (size_t j = 0; j < nP; ++j) {
        const int ta = pairs[2 * j], tb = pairs[2 * j + 1];
        ever[j] = 0;
        status[j] = mc_pair_status(tst[ta], tst[tb]);
        valid[j] = status[j] == 0 ? (uint32_t)S : 0u;
        if (status[j] != 0) continue;
        PairCountSink sink{within + j, firstAt + j, ever + j, nP};
        for (int32_t p = 0; p < S; ++p)      // a lane's pair of particles
            mc_pair_walk<N, CT>(m, x, Lw.data(), first, cdf, nComp, K, seed, ta, tb, (uint32_t)p, sink);
    }
    return 0;
}

template <int N, bool CT>
int one(int32_t nComp, int32_t T, int32_t K, uint64_t seed, double dt, double R, const double* Phi, const double* Q, const double* x, const double* P,
        const int32_t* first, const double* cdf, int32_t ta, int32_t tb, uint32_t p, double* states, double* rel, int32_t* flags) {
    McModel<N> m;
    std::vector<double> Lw;
    std::vector<int32_t> tst;
    if (!prepare<N, CT>(nComp, T, dt, R, Phi, Q, x, P, first, cdf, m, Lw, tst)) return -1;
    if (mc_pair_status(tst[ta], tst[tb]) != 0) return -2;
    PairPathSink<N> sink{states, rel, flags, K};
    mc_pair_walk<N, CT>(m, x, Lw.data(), first, cdf, nComp, K, seed, ta, tb, p, sink);
    return 0;
}

}  // namespace

// The seam's arguments on host arrays.  Returns 0, or -1 where the seam refuses (nothing written).
extern "C" int mc_pair_encounters_host(int32_t nx, int32_t transition, int32_t nComp, int32_t T, int32_t nPair, int32_t K, int32_t S, uint64_t seed, double dt,
                                       double R, const double* Phi, const double* Q, const double* x, const double* P, const int32_t* first, const double* cdf,
                                       const int32_t* pairs, uint32_t* within, uint32_t* firstAt, uint32_t* ever, uint32_t* valid, int32_t* status) {
    if (!fits(nx, transition, nComp, T, K, dt, R, Phi, Q, first) || !particles_fit(S) || nPair < 1 || nPair > MC_MAX_PAIRS) return -1;
    for (int j = 0; j < nPair; ++j) {
        const int32_t a = pairs[2 * (size_t)j], b = pairs[2 * (size_t)j + 1];
        if (a < 0 || a >= T || b < 0 || b >= T || a == b) return -1;
    }
    return mc_dispatch(nx, transition, [&](auto n, auto ct) {
        return run<decltype(n)::value, decltype(ct)::value>(nComp, T, nPair, K, S, seed, dt, R, Phi, Q, x, P, first, cdf, pairs, within, firstAt, ever, valid, status);
    });
}

// ONE pair-particle: the two particles' states [K + 1][2][nx] (a, then b), the relative path d_k [K + 1][2], and flags [K + 1][2]
// (inside at step k; step k is the first with hit_k) followed by one word (came inside at all).  Returns 0; -1 where the seam refuses;
// -2 for a pair that is not scored.
extern "C" int mc_pair_path_host(int32_t nx, int32_t transition, int32_t nComp, int32_t T, int32_t K, uint64_t seed, double dt, double R, const double* Phi,
                                 const double* Q, const double* x, const double* P, const int32_t* first, const double* cdf, int32_t ta, int32_t tb,
                                 uint32_t particle, double* states, double* rel, int32_t* flags) {
    if (!fits(nx, transition, nComp, T, K, dt, R, Phi, Q, first) || ta < 0 || ta >= T || tb < 0 || tb >= T || ta == tb) return -1;
    return mc_dispatch(nx, transition, [&](auto n, auto ct) {
        return one<decltype(n)::value, decltype(ct)::value>(nComp, T, K, seed, dt, R, Phi, Q, x, P, first, cdf, ta, tb, particle, states, rel, flags);
    });
}

// The sizer's split of a pair's particle indices: (chunks, slab) of mc_chunks(nPair, S)
extern "C" void mc_pair_chunks_host(int32_t nPair, int32_t S, int32_t* out) {
    const McSplit s = mc_chunks(nPair, S);
    out[0] = s.chunks;
    out[1] = s.slab;
}
