// mht_mc_encounters (include/mht_amd.h): encounters by Monte Carlo -- particles drawn from every target's mixture of components, walked
// with process noise (linear or constant turn) and counted against G own paths (the method, the random numbers, the factor, the order of
// every sum and the split of a target's particles: mht_mc.h).  Three launches on the context's stream, no atomic: every word has one
// writer, and the counts are integers, so the result is the same bits from run to run whatever the grid.
//
// mc_factor_kernel<N>: ONE COMPONENT PER LANE, mc_component: the factor of its P, packed and component-minor, and its status into the
// work buffer.  (The factor of Q is computed once on the host side of the seam with the same function and travels in the arguments.)
//
// mc_walk_kernel<N, CT>: ONE WORKGROUP of 256 lanes PER (target, chunk), one lane one particle, looped over the chunk's slab.  Phi and F
// are by-value kernel arguments; the workgroup stages them in LDS (see the kernel); the own paths are read at addresses that are the
// same in every lane.  The workgroup first folds the status of its target's components (a target that is not scored is left at once,
// by the whole workgroup).  Its partial counts live in LDS, 64 rows of 65 words and 64 more, 16.9 KB: the limits' size whatever G and
// K are, so that lane g of the first wavefront owns row g.  Per (g, k) a wavefront takes __popcll(__ballot(inside)) -- the sum over
// its 64 lanes in one scalar instruction; a DPP sum of mht_wave.h would add lane values, a ballot counts predicates -- and lane g
// keeps it; per step every lane puts its figure into a staging row of its wavefront, and behind ONE barrier lane g of the first
// wavefront adds the four rows to word (g, k): one owner per word, no LDS atomic.  The staging is double-buffered by the parity of
// the event, so one barrier per step serves.  At its end the workgroup stores its slab to work[chunk][g][k][t].
//
// mc_fold_kernel: ONE OUTPUT WORD PER LANE, t fastest: sums the chunks in chunk order into within [G][K + 1][T] and ever [G][T], zero
// for a target that is not scored, and writes valid [T] and status [T].
#include <vector>
#include "mht_common.h"
#include "mht_mc.h"

namespace mht {

constexpr int MC_MAX_BLOCKS = 2048;
constexpr int MC_WAVES = MC_THREADS / 64;
constexpr int MC_ROW = MC_MAX_STEPS + 1;      // words of a path's row of the workgroup's counts, whatever K is

template <int N>
struct McFactorArgs {
    int32_t nComp;
    const double* x;        // [N][nComp]
    const double* P;        // [N (N + 1) / 2][nComp]
    const double* cdf;      // [nComp]
    double* Lw;             // [N (N + 1) / 2][nComp]
    int32_t* cstatus;       // [nComp]
};

template <int N>
struct McWalkArgs {
    McModel<N> m;
    int32_t nComp, T, G, K, S, chunks, slab;
    uint64_t seed;
    const double* x;
    const double* Lw;
    const int32_t* cstatus;
    const int32_t* first;      // dev [T + 1]
    const double* cdf;
    const double* own;         // dev [G][K + 1][2]
    uint32_t* part_within;     // [chunks][G][K + 1][T]
    uint32_t* part_ever;       // [chunks][G][T]
    int32_t* tstatus;          // [T]
    int32_t target, chunk;     // (not arguments: the workgroup's target and chunk, put here by its first lane)
};

struct McFoldArgs {
    int32_t T, G, K, S, chunks;
    const uint32_t* part_within;
    const uint32_t* part_ever;
    const int32_t* tstatus;
    uint32_t* within;
    uint32_t* ever;
    uint32_t* valid;
    int32_t* status;
};

// What mc_walk hands its predicates to, in a workgroup
struct McWaveSink {
    uint32_t* cnt;                       // LDS: within [MC_MAX_PATHS][MC_ROW], then ever [MC_MAX_PATHS]: a lane of the first wavefront a row
    uint32_t (*stage)[MC_WAVES][64];     // LDS [2]
    int lane, wave, event;
    uint32_t mine;                       // lane g: the wavefront's count of path g at this step

    __device__ void take(int g, bool in) {
        const uint32_t b = (uint32_t)__popcll(__ballot(in));
        mine = lane == g ? b : mine;
    }
    __device__ void flush(int word) {      // word: the word of path `lane` at this event
        stage[event & 1][wave][lane] = mine;
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(wave) == 0) {      // (a scalar branch: the first wavefront owns the words, a lane a path)
            uint32_t s = stage[event & 1][0][lane];
#pragma unroll
            for (int w = 1; w < MC_WAVES; ++w) s += stage[event & 1][w][lane];
            cnt[word] += s;
        }
        ++event;
        mine = 0;
    }
    __device__ void within(int g, bool in) { take(g, in); }
    __device__ void step_done(int k) { flush(lane * MC_ROW + k); }
    __device__ void ever(int g, bool in) { take(g, in); }
    __device__ void particle_done() { flush(MC_MAX_PATHS * MC_ROW + lane); }
};

template <int N>
__global__ void __launch_bounds__(MC_THREADS) mc_factor_kernel(const McFactorArgs<N> a) {
    for (size_t c = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; c < (size_t)a.nComp; c += (size_t)gridDim.x * MC_THREADS)
        mc_component<N>(a.x, a.P, a.cdf, a.nComp, (int)c, a.Lw, a.cstatus);
}

template <int N, bool CT>
__global__ void __launch_bounds__(MC_THREADS) mc_walk_kernel(const McWalkArgs<N> a) {
    __shared__ uint32_t cnt[MC_MAX_PATHS * MC_ROW + MC_MAX_PATHS];
    __shared__ uint32_t stage[2][MC_WAVES][64];
    // (the by-value arguments, staged: the model's 59 doubles at six states, and with them what a particle needs once, at its start --
    // sin, cos and log keep some eighty scalar registers of constants alive over the walk, and what is read from here lives in vector
    // registers, of which there are plenty)
    __shared__ McWalkArgs<N> s;
    const int tid = threadIdx.x;
    static_assert(sizeof(McWalkArgs<N>) % 4 == 0, "the arguments are copied dword-wise");
    for (int i = tid; i < (int)(sizeof(McWalkArgs<N>) / 4); i += MC_THREADS) reinterpret_cast<uint32_t*>(&s)[i] = reinterpret_cast<const uint32_t*>(&a)[i];
    const int t = (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x % (unsigned)a.chunks);
    int nan = 0, indefinite = 0;
    for (int c = a.first[t] + tid; c < a.first[t + 1]; c += MC_THREADS) {
        const int s = a.cstatus[c];
        nan |= s == 1;
        indefinite |= s == 2;
    }
    nan = __syncthreads_or(nan);
    indefinite = __syncthreads_or(indefinite);
    const int status = nan ? 1 : (indefinite ? 2 : 0);
    if (chunk == 0 && tid == 0) a.tstatus[t] = status;
    if (status != 0) return;      // (the whole workgroup: the fold writes this target's zeros without reading a slab)
    for (int i = tid; i < MC_MAX_PATHS * MC_ROW + MC_MAX_PATHS; i += MC_THREADS) cnt[i] = 0;
    if (tid == 0) {
        s.target = t;
        s.chunk = chunk;
    }
    __syncthreads();
    // (the particle index, the slab's end and the sink's event count start from staged words: vector registers, see above)
    const uint32_t begin = (uint32_t)s.chunk * (uint32_t)s.slab;
    const uint32_t end = begin + (uint32_t)s.slab < (uint32_t)s.S ? begin + (uint32_t)s.slab : (uint32_t)s.S;
    McWaveSink sink = {cnt, stage, tid & 63, tid >> 6, s.chunk - chunk, 0u};
    uint32_t base = begin;      // (begin < end: no chunk is empty)
    do {                        // (the same trips in every lane of the workgroup: the barriers)
        const uint32_t p = base + (uint32_t)tid;
        mc_walk<N, CT>(s.m, s.x, s.Lw, s.first, s.cdf, s.own, s.nComp, a.G, a.K, s.seed, s.target, p, p < end, sink);
        base += MC_THREADS;
    } while (__builtin_amdgcn_readfirstlane((int)(base < end)) != 0);
    __syncthreads();
    // (from the staged copy: nothing of the store stays in a scalar register over the walk)
    const size_t T = (size_t)s.T, cells = (size_t)s.G * (size_t)(s.K + 1), at = (size_t)s.chunk, tt = (size_t)s.target;
    for (int i = tid; i < (int)cells; i += MC_THREADS) s.part_within[(at * cells + (size_t)i) * T + tt] = cnt[i / (s.K + 1) * MC_ROW + i % (s.K + 1)];
    for (int g = tid; g < s.G; g += MC_THREADS) s.part_ever[(at * (size_t)s.G + (size_t)g) * T + tt] = cnt[MC_MAX_PATHS * MC_ROW + g];
}

__global__ void __launch_bounds__(MC_THREADS) mc_fold_kernel(const McFoldArgs a) {
    const size_t T = (size_t)a.T, nw = (size_t)a.G * (size_t)(a.K + 1) * T, ne = (size_t)a.G * T;
    for (size_t i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; i < nw + ne + T; i += (size_t)gridDim.x * MC_THREADS) {
        if (i >= nw + ne) {
            const size_t t = i - nw - ne;
            const int32_t s = a.tstatus[t];
            a.status[t] = s;
            a.valid[t] = s == 0 ? (uint32_t)a.S : 0u;
            continue;
        }
        const bool w = i < nw;
        const size_t j = w ? i : i - nw, n = w ? nw : ne;
        const uint32_t* part = w ? a.part_within : a.part_ever;
        uint32_t sum = 0;
        if (a.tstatus[j % T] == 0)
            for (int c = 0; c < a.chunks; ++c) sum += part[(size_t)c * n + j];
        (w ? a.within : a.ever)[j] = sum;
    }
}

struct McLayout {
    size_t Lw, part_within, part_ever, cstatus, tstatus, bytes;      // offsets in bytes, and their total
};

static bool mc_sizes_fit(int32_t nx, int32_t nComp, int32_t T, int32_t G, int32_t K, int32_t S) {
    return (nx == 4 || nx == 6) && nComp >= 1 && T >= 1 && T <= nComp && G >= 1 && G <= MC_MAX_PATHS && K >= 1 && K <= MC_MAX_STEPS && S >= MC_WARP &&
           S <= MC_MAX_PARTICLES && S % MC_WARP == 0;
}

static McLayout mc_layout(int32_t nx, int32_t nComp, int32_t T, int32_t G, int32_t K, int32_t S) {
    const size_t chunks = (size_t)mc_chunks(T, S).chunks;
    McLayout l;
    l.Lw = 0;
    l.part_within = l.Lw + (size_t)(nx * (nx + 1) / 2) * (size_t)nComp * sizeof(double);
    l.part_ever = l.part_within + chunks * (size_t)G * (size_t)(K + 1) * (size_t)T * sizeof(uint32_t);
    l.cstatus = l.part_ever + chunks * (size_t)G * (size_t)T * sizeof(uint32_t);
    l.tstatus = l.cstatus + (size_t)nComp * sizeof(int32_t);
    l.bytes = (l.tstatus + (size_t)T * sizeof(int32_t) + 255) / 256 * 256;
    return l;
}

static unsigned mc_blocks(size_t items) {
    const size_t b = (items + MC_THREADS - 1) / MC_THREADS;
    return (unsigned)(b < (size_t)MC_MAX_BLOCKS ? b : (size_t)MC_MAX_BLOCKS);
}

template <int N, bool CT>
static int mc_run(mht_ctx* ctx, int32_t nComp, int32_t T, int32_t G, int32_t K, int32_t S, uint64_t seed, const McModel<N>& m, const double* x, const double* P,
                  const int32_t* first, const double* cdf, const double* own, uint32_t* within, uint32_t* ever, uint32_t* valid, int32_t* status, char* work) {
    const McLayout l = mc_layout(N, nComp, T, G, K, S);
    const McSplit split = mc_chunks(T, S);
    double* Lw = (double*)(work + l.Lw);
    uint32_t* pw = (uint32_t*)(work + l.part_within);
    uint32_t* pe = (uint32_t*)(work + l.part_ever);
    int32_t* cs = (int32_t*)(work + l.cstatus);
    int32_t* ts = (int32_t*)(work + l.tstatus);
    const McFactorArgs<N> fa = {nComp, x, P, cdf, Lw, cs};
    int rc = launch_kernel(ctx, K_SMOOTH_SCORE, mc_factor_kernel<N>, dim3(mc_blocks((size_t)nComp)), dim3(MC_THREADS), 0, false, fa);
    if (rc != MHT_OK) return rc;
    const McWalkArgs<N> wa = {m, nComp, T, G, K, S, split.chunks, split.slab, seed, x, Lw, cs, first, cdf, own, pw, pe, ts, 0, 0};
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, mc_walk_kernel<N, CT>, dim3((unsigned)T * (unsigned)split.chunks), dim3(MC_THREADS), 0, false, wa);
    if (rc != MHT_OK) return rc;
    const McFoldArgs ga = {T, G, K, S, split.chunks, pw, pe, ts, within, ever, valid, status};
    return launch_kernel(ctx, K_SMOOTH_SCORE, mc_fold_kernel, dim3(mc_blocks((size_t)G * (size_t)(K + 2) * (size_t)T + (size_t)T)), dim3(MC_THREADS), 0, false, ga);
}

// The model of a call: Phi copied (zeros for the constant-turn walk, which does not read it) and Q factored.  False: Q is not
// positive semidefinite.
template <int N>
static bool mc_model(const double* Phi, const double* Q, double dt, double R, McModel<N>& m) {
    for (int c = 0; c < N * N; ++c) m.Phi[c] = Phi ? Phi[c] : 0.0;
    m.dt = dt;
    m.R2 = R * R;
    return mc_factor<N, true>(Q, m.F) == 0;
}

static bool mc_finite(double v) { return v - v == 0.0; }

}  // namespace mht

using namespace mht;

extern "C" size_t mht_mc_work_bytes(int32_t nx, int32_t nComp, int32_t nTarget, int32_t G, int32_t steps, int32_t particles) {
    if (!mc_sizes_fit(nx, nComp, nTarget, G, steps, particles)) return 0;
    return mc_layout(nx, nComp, nTarget, G, steps, particles).bytes;
}

extern "C" int mht_mc_encounters(mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t G, int32_t steps, int32_t particles,
                                 uint64_t seed, double dt, double radius, const double* Phi, const double* Q, const double* x, const double* P,
                                 const int32_t* first, const double* cdf, const double* ownPath, uint32_t* within, uint32_t* ever, uint32_t* valid,
                                 int32_t* status, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx, "mht_mc_encounters: null context");
    MHT_REQUIRE(nx == 4 || nx == 6, "mht_mc_encounters: nx must be 4 or 6 (got %d)", nx);
    MHT_REQUIRE(transition == 0 || (transition == 1 && nx == 6), "mht_mc_encounters: transition is 0 (linear) or, with nx 6, 1 (constant turn) (got %d, nx %d)",
                transition, nx);
    MHT_REQUIRE(nComp >= 1 && nTarget >= 1 && nTarget <= nComp, "mht_mc_encounters: 1 <= nTarget <= nComp is wanted (got %d targets, %d components)", nTarget, nComp);
    MHT_REQUIRE(G >= 1 && G <= MC_MAX_PATHS, "mht_mc_encounters: G must be 1 .. %d own paths (got %d)", MC_MAX_PATHS, G);
    MHT_REQUIRE(steps >= 1 && steps <= MC_MAX_STEPS, "mht_mc_encounters: steps must be 1 .. %d (got %d)", MC_MAX_STEPS, steps);
    MHT_REQUIRE(particles >= MC_WARP && particles <= MC_MAX_PARTICLES && particles % MC_WARP == 0,
                "mht_mc_encounters: particles must be a multiple of %d in %d .. %d (got %d)", MC_WARP, MC_WARP, MC_MAX_PARTICLES, particles);
    MHT_REQUIRE(radius > 0.0 && dt > 0.0 && mc_finite(radius) && mc_finite(dt), "mht_mc_encounters: the radius and the step must be positive and finite (R %g, dt %g)",
                radius, dt);
    MHT_REQUIRE((Phi || transition == 1) && Q && x && P && first && cdf && ownPath && within && ever && valid && status && work, "mht_mc_encounters: null array");
    for (int c = 0; c < nx * nx; ++c)
        MHT_REQUIRE(mc_finite(Q[c]) && (transition == 1 || mc_finite(Phi[c])), "mht_mc_encounters: Phi and Q must be finite (entry %d)", c);
    const size_t need = mht_mc_work_bytes(nx, nComp, nTarget, G, steps, particles);
    MHT_REQUIRE(work_bytes >= need, "mht_mc_encounters: the work buffer holds %zu bytes, %zu are needed", work_bytes, need);
    McModel<4> m4;
    McModel<6> m6;
    const bool psd = nx == 4 ? mc_model<4>(Phi, Q, dt, radius, m4) : mc_model<6>(transition == 1 ? nullptr : Phi, Q, dt, radius, m6);
    MHT_REQUIRE(psd, "mht_mc_encounters: Q is not positive semidefinite");
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    // (first lives on the device: it is read back and checked before anything is launched -- a walk indexes the components with it)
    std::vector<int32_t> f((size_t)nTarget + 1);
    MHT_HIP_CHECK(hipMemcpyAsync(f.data(), first, f.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MHT_REQUIRE(f[0] == 0 && f[(size_t)nTarget] == nComp, "mht_mc_encounters: first runs from 0 to nComp = %d (got %d .. %d)", nComp, f[0], f[(size_t)nTarget]);
    for (int t = 0; t < nTarget; ++t)
        MHT_REQUIRE(f[(size_t)t + 1] > f[(size_t)t], "mht_mc_encounters: first does not ascend at target %d (%d, then %d)", t, f[(size_t)t], f[(size_t)t + 1]);
    int rc;
    if (nx == 4) rc = mc_run<4, false>(ctx, nComp, nTarget, G, steps, particles, seed, m4, x, P, first, cdf, ownPath, within, ever, valid, status, (char*)work);
    else if (transition == 1) rc = mc_run<6, true>(ctx, nComp, nTarget, G, steps, particles, seed, m6, x, P, first, cdf, ownPath, within, ever, valid, status, (char*)work);
    else rc = mc_run<6, false>(ctx, nComp, nTarget, G, steps, particles, seed, m6, x, P, first, cdf, ownPath, within, ever, valid, status, (char*)work);
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
