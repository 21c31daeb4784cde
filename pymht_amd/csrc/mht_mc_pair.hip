// mht_mc_pair_encounters (include/mht_amd.h): Monte-Carlo encounters between pairs of targets -- particle p of target a against particle
// p of target b, both walked as mht_mc.h's mc_walk walks them (the definition, the counts and the status of a pair: mht_mc_pair.h).
// Three launches on the context's stream, no atomic: every word has one writer, and the counts are integers, so the result is the same
// bits from run to run whatever the grid.
//
// mc_pair_factor_kernel<N>: ONE COMPONENT PER LANE, mc_component: the factor of its P and its status into the work buffer.
//
// mc_pair_walk_kernel<N, CT>: ONE WORKGROUP of 256 lanes PER (pair, chunk), one lane one particle index, looped over the chunk's slab
// (mc_chunks(nPair, S)).  A lane steps particle a, then particle b, per step.  There is ONE relative path here -- mc_walk_kernel has 64
// own paths sharing the lanes, hence its barrier per step --, so the counts need no LDS and no barrier inside the particle loop: per
// step a wavefront takes __popcll(__ballot(pred)) for within and for firstAt, and lane k ADDS it into a register it keeps over the
// whole slab (65 words per array at K = 64: a lane holds two words per array, k and k + 64).  The wavefronts run the loop on their own
// -- one whose 64 particle indices all lie beyond the slab's end leaves it; S and the slab are multiples of 64, so no wavefront is
// partly live -- and meet once, after it: LDS, one barrier, and the first wavefront stores part[chunk][word][pair], the words of a
// pair being within[0 .. K], firstAt[0 .. K], ever.  The by-value model is staged in LDS as mc_walk_kernel stages it, for its reason:
// sin, cos and log hold some eighty scalar registers of constants over the walk, and read from the scalar argument block the model
// spills scalar registers.
//
// mc_pair_fold_kernel: ONE OUTPUT WORD PER LANE, pair fastest: sums the chunks in chunk order into within [K + 1][nPair], firstAt
// [K + 1][nPair] and ever [nPair], zero for a pair that is not scored, and writes valid [nPair] and status [nPair].
#include <vector>
#include "mht_common.h"
#include "mht_mc_pair.h"

namespace mht {

constexpr int MCP_MAX_BLOCKS = 2048;
constexpr int MCP_WAVES = MC_THREADS / 64;
constexpr int MCP_ROW = MC_MAX_STEPS + 1;           // words of an array in a wavefront's row of the meeting, whatever K is
constexpr int MCP_WORDS = 2 * MCP_ROW + 1;          // within, firstAt, ever

template <int N>
struct McPairFactorArgs {
    int32_t nComp;
    const double* x;        // [N][nComp]
    const double* P;        // [N (N + 1) / 2][nComp]
    const double* cdf;      // [nComp]
    double* Lw;             // [N (N + 1) / 2][nComp]
    int32_t* cstatus;       // [nComp]
};

template <int N>
struct McPairWalkArgs {
    McModel<N> m;
    int32_t nComp, nPair, K, S, chunks, slab;
    uint64_t seed;
    const double* x;
    const double* Lw;
    const int32_t* cstatus;
    const int32_t* first;      // dev [T + 1]
    const double* cdf;
    const int32_t* pairs;      // dev [nPair][2]
    uint32_t* part;            // [chunks][2 (K + 1) + 1][nPair]
    int32_t* pstatus;          // [nPair]
    int32_t pair, chunk, ta, tb;      // (not arguments: the workgroup's pair, chunk and targets, put here by its first lane)
};

struct McPairFoldArgs {
    int32_t nPair, K, S, chunks;
    const uint32_t* part;
    const int32_t* pstatus;
    uint32_t* within;
    uint32_t* firstAt;
    uint32_t* ever;
    uint32_t* valid;
    int32_t* status;
};

// What mc_pair_walk hands its predicates to, in a wavefront: lane l keeps the counts of steps l and l + 64
struct McPairWaveSink {
    int lane;
    uint32_t w0, w1, f0, f1, ev;

    __device__ void path(int, const double*, const double*, double, double) {}
    __device__ void step(int k, bool inside, bool first) {
        const uint32_t bw = (uint32_t)__popcll(__ballot(inside)), bf = (uint32_t)__popcll(__ballot(first));
        if (k < 64) {      // (k is the same in every lane: a scalar branch)
            w0 += lane == k ? bw : 0u;
            f0 += lane == k ? bf : 0u;
        } else {
            w1 += lane == k - 64 ? bw : 0u;
            f1 += lane == k - 64 ? bf : 0u;
        }
    }
    __device__ void done(bool came) { ev += (uint32_t)__popcll(__ballot(came)); }
};

template <int N>
__global__ void __launch_bounds__(MC_THREADS) mc_pair_factor_kernel(const McPairFactorArgs<N> a) {
    for (size_t c = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; c < (size_t)a.nComp; c += (size_t)gridDim.x * MC_THREADS)
        mc_component<N>(a.x, a.P, a.cdf, a.nComp, (int)c, a.Lw, a.cstatus);
}

template <int N, bool CT>
__global__ void __launch_bounds__(MC_THREADS) mc_pair_walk_kernel(const McPairWalkArgs<N> a) {
    __shared__ uint32_t meet[MCP_WAVES][MCP_WORDS];
    // (the by-value arguments, staged: see the head of the file)
    __shared__ McPairWalkArgs<N> s;
    const int tid = threadIdx.x;
    static_assert(sizeof(McPairWalkArgs<N>) % 4 == 0, "the arguments are copied dword-wise");
    for (int i = tid; i < (int)(sizeof(McPairWalkArgs<N>) / 4); i += MC_THREADS) reinterpret_cast<uint32_t*>(&s)[i] = reinterpret_cast<const uint32_t*>(&a)[i];
    const int pair = (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x % (unsigned)a.chunks);
    const int ta = a.pairs[2 * (size_t)pair], tb = a.pairs[2 * (size_t)pair + 1];      // (checked by the seam: 0 <= ta, tb < T, ta != tb)
    int nan = 0, indefinite = 0;
    for (int c = a.first[ta] + tid; c < a.first[ta + 1]; c += MC_THREADS) {
        const int st = a.cstatus[c];
        nan |= st == 1;
        indefinite |= st == 2;
    }
    for (int c = a.first[tb] + tid; c < a.first[tb + 1]; c += MC_THREADS) {
        const int st = a.cstatus[c];
        nan |= st == 1;
        indefinite |= st == 2;
    }
    nan = __syncthreads_or(nan);
    indefinite = __syncthreads_or(indefinite);
    const int status = nan ? 1 : (indefinite ? 2 : 0);
    if (chunk == 0 && tid == 0) a.pstatus[pair] = status;
    if (status != 0) return;      // (the whole workgroup: the fold writes this pair's zeros without reading a slab)
    if (tid == 0) {
        s.pair = pair;
        s.chunk = chunk;
        s.ta = ta;
        s.tb = tb;
    }
    __syncthreads();
    // (the particle index and the slab's end start from staged words: vector registers, of which there are plenty)
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t begin = (uint32_t)s.chunk * (uint32_t)s.slab;
    const uint32_t end = begin + (uint32_t)s.slab < (uint32_t)s.S ? begin + (uint32_t)s.slab : (uint32_t)s.S;
    McPairWaveSink sink = {lane, 0u, 0u, 0u, 0u, 0u};
    // (no barrier in here: a wavefront's trips are its own.  begin, end and 64 * wave are multiples of 64: a wavefront is live as a whole)
    for (uint32_t base = begin + 64u * (uint32_t)wave; __builtin_amdgcn_readfirstlane((int)(base < end)) != 0; base += MC_THREADS)
        mc_pair_walk<N, CT>(s.m, s.x, s.Lw, s.first, s.cdf, s.nComp, a.K, s.seed, s.ta, s.tb, base + (uint32_t)lane, sink);
    meet[wave][lane] = sink.w0;
    meet[wave][MCP_ROW + lane] = sink.f0;
    if (lane == 0) {
        meet[wave][64] = sink.w1;
        meet[wave][MCP_ROW + 64] = sink.f1;
        meet[wave][2 * MCP_ROW] = sink.ev;
    }
    __syncthreads();
    if (wave != 0) return;
    // (from the staged copy: nothing of the store stays in a scalar register over the walk)
    const int K1 = s.K + 1, words = 2 * K1 + 1;
    const size_t nP = (size_t)s.nPair, at = (size_t)s.chunk * (size_t)words, pp = (size_t)s.pair;
    for (int i = lane; i < words; i += 64) {
        const int from = i < K1 ? i : (i < 2 * K1 ? MCP_ROW + (i - K1) : 2 * MCP_ROW);
        uint32_t sum = meet[0][from];
#pragma unroll
        for (int w = 1; w < MCP_WAVES; ++w) sum += meet[w][from];
        s.part[(at + (size_t)i) * nP + pp] = sum;
    }
}

__global__ void __launch_bounds__(MC_THREADS) mc_pair_fold_kernel(const McPairFoldArgs a) {
    const size_t nP = (size_t)a.nPair, nc = (size_t)(2 * (a.K + 1) + 1) * nP, nw = (size_t)(a.K + 1) * nP;
    for (size_t i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; i < nc + nP; i += (size_t)gridDim.x * MC_THREADS) {
        if (i >= nc) {
            const size_t j = i - nc;
            const int32_t st = a.pstatus[j];
            a.status[j] = st;
            a.valid[j] = st == 0 ? (uint32_t)a.S : 0u;
            continue;
        }
        uint32_t sum = 0;
        if (a.pstatus[i % nP] == 0)
            for (int c = 0; c < a.chunks; ++c) sum += a.part[(size_t)c * nc + i];
        if (i < nw) a.within[i] = sum;
        else if (i < 2 * nw) a.firstAt[i - nw] = sum;
        else a.ever[i - 2 * nw] = sum;
    }
}

struct McPairLayout {
    size_t Lw, part, cstatus, pstatus, bytes;      // offsets in bytes, and their total
};

static bool mc_pair_sizes_fit(int32_t nx, int32_t nComp, int32_t T, int32_t nPair, int32_t K, int32_t S) {
    return (nx == 4 || nx == 6) && nComp >= 1 && T >= 1 && T <= nComp && nPair >= 1 && nPair <= MC_MAX_PAIRS && K >= 1 && K <= MC_MAX_STEPS && S >= MC_WARP &&
           S <= MC_MAX_PARTICLES && S % MC_WARP == 0;
}

static McPairLayout mc_pair_layout(int32_t nx, int32_t nComp, int32_t nPair, int32_t K, int32_t S) {
    const size_t chunks = (size_t)mc_chunks(nPair, S).chunks;
    McPairLayout l;
    l.Lw = 0;
    l.part = l.Lw + (size_t)(nx * (nx + 1) / 2) * (size_t)nComp * sizeof(double);
    l.cstatus = l.part + chunks * (size_t)(2 * (K + 1) + 1) * (size_t)nPair * sizeof(uint32_t);
    l.pstatus = l.cstatus + (size_t)nComp * sizeof(int32_t);
    l.bytes = (l.pstatus + (size_t)nPair * sizeof(int32_t) + 255) / 256 * 256;
    return l;
}

static unsigned mc_pair_blocks(size_t items) {
    const size_t b = (items + MC_THREADS - 1) / MC_THREADS;
    return (unsigned)(b < (size_t)MCP_MAX_BLOCKS ? b : (size_t)MCP_MAX_BLOCKS);
}

template <int N, bool CT>
static int mc_pair_run(mht_ctx* ctx, int32_t nComp, int32_t nPair, int32_t K, int32_t S, uint64_t seed, const McModel<N>& m, const double* x, const double* P,
                       const int32_t* first, const double* cdf, const int32_t* pairs, uint32_t* within, uint32_t* firstAt, uint32_t* ever, uint32_t* valid,
                       int32_t* status, char* work) {
    const McPairLayout l = mc_pair_layout(N, nComp, nPair, K, S);
    const McSplit split = mc_chunks(nPair, S);
    double* Lw = (double*)(work + l.Lw);
    uint32_t* part = (uint32_t*)(work + l.part);
    int32_t* cs = (int32_t*)(work + l.cstatus);
    int32_t* ps = (int32_t*)(work + l.pstatus);
    const McPairFactorArgs<N> fa = {nComp, x, P, cdf, Lw, cs};
    int rc = launch_kernel(ctx, K_SMOOTH_SCORE, mc_pair_factor_kernel<N>, dim3(mc_pair_blocks((size_t)nComp)), dim3(MC_THREADS), 0, false, fa);
    if (rc != MHT_OK) return rc;
    const McPairWalkArgs<N> wa = {m, nComp, nPair, K, S, split.chunks, split.slab, seed, x, Lw, cs, first, cdf, pairs, part, ps, 0, 0, 0, 0};
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, mc_pair_walk_kernel<N, CT>, dim3((unsigned)nPair * (unsigned)split.chunks), dim3(MC_THREADS), 0, false, wa);
    if (rc != MHT_OK) return rc;
    const McPairFoldArgs ga = {nPair, K, S, split.chunks, part, ps, within, firstAt, ever, valid, status};
    return launch_kernel(ctx, K_SMOOTH_SCORE, mc_pair_fold_kernel, dim3(mc_pair_blocks((size_t)(2 * (K + 1) + 2) * (size_t)nPair)), dim3(MC_THREADS), 0, false, ga);
}

// The model of a call: Phi copied (zeros for the constant-turn walk, which does not read it) and Q factored.  False: Q is not
// positive semidefinite.
template <int N>
static bool mc_pair_model(const double* Phi, const double* Q, double dt, double R, McModel<N>& m) {
    for (int c = 0; c < N * N; ++c) m.Phi[c] = Phi ? Phi[c] : 0.0;
    m.dt = dt;
    m.R2 = R * R;
    return mc_factor<N, true>(Q, m.F) == 0;
}

static bool mc_pair_finite(double v) { return v - v == 0.0; }

}  // namespace mht

using namespace mht;

extern "C" size_t mht_mc_pair_work_bytes(int32_t nx, int32_t nComp, int32_t nTarget, int32_t nPair, int32_t steps, int32_t particles) {
    if (!mc_pair_sizes_fit(nx, nComp, nTarget, nPair, steps, particles)) return 0;
    return mc_pair_layout(nx, nComp, nPair, steps, particles).bytes;
}

extern "C" int mht_mc_pair_encounters(mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t nPair, int32_t steps,
                                      int32_t particles, uint64_t seed, double dt, double radius, const double* Phi, const double* Q, const double* x,
                                      const double* P, const int32_t* first, const double* cdf, const int32_t* pairs, uint32_t* within, uint32_t* firstAt,
                                      uint32_t* ever, uint32_t* valid, int32_t* status, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx, "mht_mc_pair_encounters: null context");
    MHT_REQUIRE(nx == 4 || nx == 6, "mht_mc_pair_encounters: nx must be 4 or 6 (got %d)", nx);
    MHT_REQUIRE(transition == 0 || (transition == 1 && nx == 6),
                "mht_mc_pair_encounters: transition is 0 (linear) or, with nx 6, 1 (constant turn) (got %d, nx %d)", transition, nx);
    MHT_REQUIRE(nComp >= 1 && nTarget >= 1 && nTarget <= nComp, "mht_mc_pair_encounters: 1 <= nTarget <= nComp is wanted (got %d targets, %d components)", nTarget,
                nComp);
    MHT_REQUIRE(nPair >= 1 && nPair <= MC_MAX_PAIRS, "mht_mc_pair_encounters: nPair must be 1 .. %d pairs (got %d)", MC_MAX_PAIRS, nPair);
    MHT_REQUIRE(steps >= 1 && steps <= MC_MAX_STEPS, "mht_mc_pair_encounters: steps must be 1 .. %d (got %d)", MC_MAX_STEPS, steps);
    MHT_REQUIRE(particles >= MC_WARP && particles <= MC_MAX_PARTICLES && particles % MC_WARP == 0,
                "mht_mc_pair_encounters: particles must be a multiple of %d in %d .. %d (got %d)", MC_WARP, MC_WARP, MC_MAX_PARTICLES, particles);
    MHT_REQUIRE(radius > 0.0 && dt > 0.0 && mc_pair_finite(radius) && mc_pair_finite(dt),
                "mht_mc_pair_encounters: the radius and the step must be positive and finite (R %g, dt %g)", radius, dt);
    MHT_REQUIRE((Phi || transition == 1) && Q && x && P && first && cdf && pairs && within && firstAt && ever && valid && status && work,
                "mht_mc_pair_encounters: null array");
    for (int c = 0; c < nx * nx; ++c)
        MHT_REQUIRE(mc_pair_finite(Q[c]) && (transition == 1 || mc_pair_finite(Phi[c])), "mht_mc_pair_encounters: Phi and Q must be finite (entry %d)", c);
    const size_t need = mht_mc_pair_work_bytes(nx, nComp, nTarget, nPair, steps, particles);
    MHT_REQUIRE(work_bytes >= need, "mht_mc_pair_encounters: the work buffer holds %zu bytes, %zu are needed", work_bytes, need);
    McModel<4> m4;
    McModel<6> m6;
    const bool psd = nx == 4 ? mc_pair_model<4>(Phi, Q, dt, radius, m4) : mc_pair_model<6>(transition == 1 ? nullptr : Phi, Q, dt, radius, m6);
    MHT_REQUIRE(psd, "mht_mc_pair_encounters: Q is not positive semidefinite");
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    // (first and pairs live on the device: they are read back and checked before anything is launched -- a walk indexes the components
    // with first and first with pairs)
    std::vector<int32_t> f((size_t)nTarget + 1), pr((size_t)nPair * 2);
    MHT_HIP_CHECK(hipMemcpyAsync(f.data(), first, f.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MHT_HIP_CHECK(hipMemcpyAsync(pr.data(), pairs, pr.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MHT_REQUIRE(f[0] == 0 && f[(size_t)nTarget] == nComp, "mht_mc_pair_encounters: first runs from 0 to nComp = %d (got %d .. %d)", nComp, f[0], f[(size_t)nTarget]);
    for (int t = 0; t < nTarget; ++t)
        MHT_REQUIRE(f[(size_t)t + 1] > f[(size_t)t], "mht_mc_pair_encounters: first does not ascend at target %d (%d, then %d)", t, f[(size_t)t], f[(size_t)t + 1]);
    for (int j = 0; j < nPair; ++j) {
        const int32_t pa = pr[2 * (size_t)j], pb = pr[2 * (size_t)j + 1];
        MHT_REQUIRE(pa >= 0 && pa < nTarget && pb >= 0 && pb < nTarget && pa != pb,
                    "mht_mc_pair_encounters: pair %d is (%d, %d); two distinct targets in 0 .. %d are wanted", j, pa, pb, nTarget - 1);
    }
    char* w = (char*)work;
    int rc;
    if (nx == 4) rc = mc_pair_run<4, false>(ctx, nComp, nPair, steps, particles, seed, m4, x, P, first, cdf, pairs, within, firstAt, ever, valid, status, w);
    else if (transition == 1) rc = mc_pair_run<6, true>(ctx, nComp, nPair, steps, particles, seed, m6, x, P, first, cdf, pairs, within, firstAt, ever, valid, status, w);
    else rc = mc_pair_run<6, false>(ctx, nComp, nPair, steps, particles, seed, m6, x, P, first, cdf, pairs, within, firstAt, ever, valid, status, w);
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
