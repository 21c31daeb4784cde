// mht_mc_encounters and mht_mc_pair_encounters (include/mht_amd.h): encounters by Monte Carlo -- particles drawn from every target's
// mixture of components and walked with process noise (linear or constant turn), counted against G own paths (the method, the random
// numbers, the factor, the order of every sum and the split of a target's particles: mht_mc.h) or, particle p of target a against
// particle p of target b, between pairs of targets (the definition, the counts and the status of a pair: mht_mc_pair.h).  Either seam
// is three launches on the context's stream -- factor, walk, fold -- and no atomic: every word has one writer, and the counts are
// integers, so the result is the same bits from run to run whatever the grid.  The factor and the fold are one kernel for both; a walk
// kernel stores its workgroup's counts to part[chunk][word][item], item a target or a pair, and the fold sums the chunks.
//
// Both walk kernels keep their by-value arguments in LDS (mc_stage): sin, cos and log hold some eighty scalar registers of constants
// over the walk, and read from the scalar argument block the model's 59 doubles at six states and the launch's sizes spill scalar
// registers; what is read from LDS lives in vector registers, of which there are plenty.  The six-state linear pair walk stands at 248
// of 256 vector registers: mc_stage and mc_target_flags run before its loop and cost neither walk a register, a byte of LDS or a spill
// (tests/test_mc_resources.py; profiles/mc_seam_refactor.txt has every kernel's figures against the two units this one replaced, and
// the whole-call times -- with the one row, own ship at 65 536 particles and 16 paths, that the placement of the unchanged particle
// loop in the code object moved by 1 to 2.5 %).
//
// The per-kernel paragraphs stand with the kernels.
//
// mht_mc_seam.h declares what a seam in another unit launches through (mht_mc_zone.hip, the guard zones): the factor and the fold
// launches, the layout and the shared checks, all defined here.
#include <vector>
#include "mht_common.h"
#include "mht_mc_pair.h"
#include "mht_mc_seam.h"

namespace mht {

// (MC_ROW, mht_mc_seam.h: the words of a path's row (own ship) or of an array (pair) in LDS, whatever K is)
constexpr int MC_PAIR_WORDS = 2 * MC_ROW + 1;       // within, firstAt, ever

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
    uint32_t* part;            // [chunks][G (K + 1) + G][T]: within [G][K + 1], then ever [G]
    int32_t* tstatus;          // [T]
    int32_t target, chunk;     // (not arguments: the workgroup's target and chunk, put here by its first lane)
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
    uint32_t* part;            // [chunks][2 (K + 1) + 1][nPair]: within [K + 1], firstAt [K + 1], ever
    int32_t* pstatus;          // [nPair]
    int32_t pair, chunk, ta, tb;      // (not arguments: the workgroup's pair, chunk and targets, put here by its first lane)
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

// (mc_stage, the by-value arguments of a walk kernel into the workgroup's LDS, and mc_target_flags: mht_mc_seam.h)

// ONE COMPONENT PER LANE, mc_component: the factor of its P, packed and component-minor, and its status into the work buffer.  (The
// factor of Q is computed once on the host side of the seam with the same function and travels in the arguments.)
template <int N>
__global__ void __launch_bounds__(MC_THREADS) mc_factor_kernel(const McFactorArgs<N> a) {
    for (size_t c = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; c < (size_t)a.nComp; c += (size_t)gridDim.x * MC_THREADS)
        mc_component<N>(a.x, a.P, a.cdf, a.nComp, (int)c, a.Lw, a.cstatus);
}

// ONE WORKGROUP of 256 lanes PER (target, chunk), one lane one particle, looped over the chunk's slab.  Phi and F are staged in LDS;
// the own paths are read at addresses that are the same in every lane.  The workgroup first folds the status of its target's
// components (a target that is not scored is left at once, by the whole workgroup).  Its partial counts live in LDS, 64 rows of 65
// words and 64 more, 16.9 KB: the limits' size whatever G and K are, so that lane g of the first wavefront owns row g.  Per (g, k) a
// wavefront takes __popcll(__ballot(inside)) -- the sum over its 64 lanes in one scalar instruction; a DPP sum of mht_wave.h would add
// lane values, a ballot counts predicates -- and lane g keeps it; per step every lane puts its figure into a staging row of its
// wavefront, and behind ONE barrier lane g of the first wavefront adds the four rows to word (g, k): one owner per word, no LDS
// atomic.  The staging is double-buffered by the parity of the event, so one barrier per step serves.  At its end the workgroup stores
// its slab to part[chunk][word][t], the words of a target being within[g][k], then ever[g].
template <int N, bool CT>
__global__ void __launch_bounds__(MC_THREADS) mc_walk_kernel(const McWalkArgs<N> a) {
    __shared__ uint32_t cnt[MC_MAX_PATHS * MC_ROW + MC_MAX_PATHS];
    __shared__ uint32_t stage[2][MC_WAVES][64];
    // (with the model, what a particle needs once, at its start)
    __shared__ McWalkArgs<N> s;
    const int tid = threadIdx.x;
    mc_stage(s, a, tid);
    const int t = (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x % (unsigned)a.chunks);
    int nan = 0, indefinite = 0;
    mc_target_flags(a.first, a.cstatus, t, tid, nan, indefinite);
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
    // (the particle index, the slab's end and the sink's event count start from staged words: vector registers)
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
    const size_t T = (size_t)s.T, cells = (size_t)s.G * (size_t)(s.K + 1), at = (size_t)s.chunk * (cells + (size_t)s.G), tt = (size_t)s.target;
    for (int i = tid; i < (int)cells; i += MC_THREADS) s.part[(at + (size_t)i) * T + tt] = cnt[i / (s.K + 1) * MC_ROW + i % (s.K + 1)];
    for (int g = tid; g < s.G; g += MC_THREADS) s.part[(at + cells + (size_t)g) * T + tt] = cnt[MC_MAX_PATHS * MC_ROW + g];
}

// ONE WORKGROUP of 256 lanes PER (pair, chunk), one lane one particle index, looped over the chunk's slab (mc_chunks(nPair, S)).  A
// lane steps particle a, then particle b, per step.  There is ONE relative path here -- mc_walk_kernel has 64 own paths sharing the
// lanes, hence its barrier per step --, so the counts need no LDS and no barrier inside the particle loop: per step a wavefront takes
// __popcll(__ballot(pred)) for within and for firstAt, and lane k ADDS it into a register it keeps over the whole slab (65 words per
// array at K = 64: a lane holds two words per array, k and k + 64).  The wavefronts run the loop on their own -- one whose 64 particle
// indices all lie beyond the slab's end leaves it; S and the slab are multiples of 64, so no wavefront is partly live -- and meet once,
// after it: LDS, one barrier, and the first wavefront stores part[chunk][word][pair], the words of a pair being within[0 .. K],
// firstAt[0 .. K], ever.
template <int N, bool CT>
__global__ void __launch_bounds__(MC_THREADS) mc_pair_walk_kernel(const McPairWalkArgs<N> a) {
    __shared__ uint32_t meet[MC_WAVES][MC_PAIR_WORDS];
    __shared__ McPairWalkArgs<N> s;
    const int tid = threadIdx.x;
    mc_stage(s, a, tid);
    const int pair = (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x % (unsigned)a.chunks);
    const int ta = a.pairs[2 * (size_t)pair], tb = a.pairs[2 * (size_t)pair + 1];      // (checked by the seam: 0 <= ta, tb < T, ta != tb)
    int nan = 0, indefinite = 0;
    mc_target_flags(a.first, a.cstatus, ta, tid, nan, indefinite);
    mc_target_flags(a.first, a.cstatus, tb, tid, nan, indefinite);
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
    // (the particle index and the slab's end start from staged words: vector registers)
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t begin = (uint32_t)s.chunk * (uint32_t)s.slab;
    const uint32_t end = begin + (uint32_t)s.slab < (uint32_t)s.S ? begin + (uint32_t)s.slab : (uint32_t)s.S;
    McPairWaveSink sink = {lane, 0u, 0u, 0u, 0u, 0u};
    // (no barrier in here: a wavefront's trips are its own.  begin, end and 64 * wave are multiples of 64: a wavefront is live as a whole)
    for (uint32_t base = begin + 64u * (uint32_t)wave; __builtin_amdgcn_readfirstlane((int)(base < end)) != 0; base += MC_THREADS)
        mc_pair_walk<N, CT>(s.m, s.x, s.Lw, s.first, s.cdf, s.nComp, a.K, s.seed, s.ta, s.tb, base + (uint32_t)lane, sink);
    meet[wave][lane] = sink.w0;
    meet[wave][MC_ROW + lane] = sink.f0;
    if (lane == 0) {
        meet[wave][64] = sink.w1;
        meet[wave][MC_ROW + 64] = sink.f1;
        meet[wave][2 * MC_ROW] = sink.ev;
    }
    __syncthreads();
    if (wave != 0) return;
    // (from the staged copy: nothing of the store stays in a scalar register over the walk)
    const int K1 = s.K + 1, words = 2 * K1 + 1;
    const size_t nP = (size_t)s.nPair, at = (size_t)s.chunk * (size_t)words, pp = (size_t)s.pair;
    for (int i = lane; i < words; i += 64) {
        const int from = i < K1 ? i : (i < 2 * K1 ? MC_ROW + (i - K1) : 2 * MC_ROW);
        uint32_t sum = meet[0][from];
#pragma unroll
        for (int w = 1; w < MC_WAVES; ++w) sum += meet[w][from];
        s.part[(at + (size_t)i) * nP + pp] = sum;
    }
}

// ONE OUTPUT WORD PER LANE, item fastest: sums part[chunk][word][item] over the chunks in chunk order into the output array the word
// belongs to -- own ship: within [G][K + 1][T] and ever [G][T]; pairs: within [K + 1][nPair], firstAt [K + 1][nPair] and ever [nPair]
// --, zero for an item that is not scored, and writes valid [items] and status [items].
__global__ void __launch_bounds__(MC_THREADS) mc_fold_kernel(const McFoldArgs a) {
    const size_t n = (size_t)a.items, nc = (size_t)a.words * n, n0 = (size_t)a.end0 * n, n1 = (size_t)a.end1 * n;
    for (size_t i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; i < nc + n; i += (size_t)gridDim.x * MC_THREADS) {
        if (i >= nc) {
            const size_t j = i - nc;
            const int32_t st = a.istatus[j];
            a.status[j] = st;
            a.valid[j] = st == 0 ? (uint32_t)a.S : 0u;
            continue;
        }
        uint32_t sum = 0;
        if (a.istatus[i % n] == 0)
            for (int c = 0; c < a.chunks; ++c) sum += a.part[(size_t)c * nc + i];
        if (i < n0) a.out0[i] = sum;
        else if (i < n1) a.out1[i - n0] = sum;
        else a.out2[i - n1] = sum;
    }
}

// The work buffer of a call over `items` targets or pairs of `words` words each (McLayout: mht_mc_seam.h)
McLayout mc_layout(int32_t nx, int32_t nComp, int32_t items, int32_t words, int32_t S) {
    McLayout l;
    l.split = mc_chunks(items, S);
    l.Lw = 0;
    l.part = l.Lw + (size_t)(nx * (nx + 1) / 2) * (size_t)nComp * sizeof(double);
    l.cstatus = l.part + (size_t)l.split.chunks * (size_t)words * (size_t)items * sizeof(uint32_t);
    l.istatus = l.cstatus + (size_t)nComp * sizeof(int32_t);
    l.bytes = (l.istatus + (size_t)items * sizeof(int32_t) + 255) / 256 * 256;
    return l;
}

bool mc_sizes_fit(int32_t nx, int32_t nComp, int32_t T, int32_t K, int32_t S) {
    return (nx == 4 || nx == 6) && nComp >= 1 && T >= 1 && T <= nComp && K >= 1 && K <= MC_MAX_STEPS && S >= MC_WARP && S <= MC_MAX_PARTICLES && S % MC_WARP == 0;
}

static unsigned mc_blocks(size_t items) {
    const size_t b = (items + MC_THREADS - 1) / MC_THREADS;
    return (unsigned)(b < (size_t)MC_MAX_BLOCKS ? b : (size_t)MC_MAX_BLOCKS);
}

template <int N>
static int mc_launch_factor(mht_ctx* ctx, int32_t nComp, const double* x, const double* P, const double* cdf, double* Lw, int32_t* cstatus) {
    const McFactorArgs<N> fa = {nComp, x, P, cdf, Lw, cstatus};
    return launch_kernel(ctx, K_SMOOTH_SCORE, mc_factor_kernel<N>, dim3(mc_blocks((size_t)nComp)), dim3(MC_THREADS), 0, false, fa);
}

int mc_launch_factor(mht_ctx* ctx, int32_t nx, int32_t nComp, const double* x, const double* P, const double* cdf, double* Lw, int32_t* cstatus) {
    return nx == 4 ? mc_launch_factor<4>(ctx, nComp, x, P, cdf, Lw, cstatus) : mc_launch_factor<6>(ctx, nComp, x, P, cdf, Lw, cstatus);
}

int mc_launch_fold(mht_ctx* ctx, const McFoldArgs& ga) {
    return launch_kernel(ctx, K_SMOOTH_SCORE, mc_fold_kernel, dim3(mc_blocks((size_t)(ga.words + 1) * (size_t)ga.items)), dim3(MC_THREADS), 0, false, ga);
}

template <int N, bool CT>
static int mc_run(mht_ctx* ctx, int32_t nComp, int32_t T, int32_t G, int32_t K, int32_t S, uint64_t seed, const McModel<N>& m, const double* x, const double* P,
                  const int32_t* first, const double* cdf, const double* own, uint32_t* within, uint32_t* ever, uint32_t* valid, int32_t* status, char* work) {
    const int32_t words = G * (K + 2);
    const McLayout l = mc_layout(N, nComp, T, words, S);
    double* Lw = (double*)(work + l.Lw);
    uint32_t* part = (uint32_t*)(work + l.part);
    int32_t* cs = (int32_t*)(work + l.cstatus);
    int32_t* ts = (int32_t*)(work + l.istatus);
    int rc = mc_launch_factor<N>(ctx, nComp, x, P, cdf, Lw, cs);
    if (rc != MHT_OK) return rc;
    const McWalkArgs<N> wa = {m, nComp, T, G, K, S, l.split.chunks, l.split.slab, seed, x, Lw, cs, first, cdf, own, part, ts, 0, 0};
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, mc_walk_kernel<N, CT>, dim3((unsigned)T * (unsigned)l.split.chunks), dim3(MC_THREADS), 0, false, wa);
    if (rc != MHT_OK) return rc;
    return mc_launch_fold(ctx, McFoldArgs{T, words, l.split.chunks, S, part, ts, within, ever, nullptr, G * (K + 1), words, valid, status});
}

template <int N, bool CT>
static int mc_pair_run(mht_ctx* ctx, int32_t nComp, int32_t nPair, int32_t K, int32_t S, uint64_t seed, const McModel<N>& m, const double* x, const double* P,
                       const int32_t* first, const double* cdf, const int32_t* pairs, uint32_t* within, uint32_t* firstAt, uint32_t* ever, uint32_t* valid,
                       int32_t* status, char* work) {
    const int32_t words = 2 * (K + 1) + 1;
    const McLayout l = mc_layout(N, nComp, nPair, words, S);
    double* Lw = (double*)(work + l.Lw);
    uint32_t* part = (uint32_t*)(work + l.part);
    int32_t* cs = (int32_t*)(work + l.cstatus);
    int32_t* ps = (int32_t*)(work + l.istatus);
    int rc = mc_launch_factor<N>(ctx, nComp, x, P, cdf, Lw, cs);
    if (rc != MHT_OK) return rc;
    const McPairWalkArgs<N> wa = {m, nComp, nPair, K, S, l.split.chunks, l.split.slab, seed, x, Lw, cs, first, cdf, pairs, part, ps, 0, 0, 0, 0};
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, mc_pair_walk_kernel<N, CT>, dim3((unsigned)nPair * (unsigned)l.split.chunks), dim3(MC_THREADS), 0, false, wa);
    if (rc != MHT_OK) return rc;
    return mc_launch_fold(ctx, McFoldArgs{nPair, words, l.split.chunks, S, part, ps, within, firstAt, ever, K + 1, 2 * (K + 1), valid, status});
}

// The checks the seams share, under the seam's name `who`, in the seams' order: nx, transition, nComp and nTarget, steps,
// particles, radius and dt, Phi and Q finite (the seam has checked that they are there), and -- first lives on the device: it is read
// back and checked before anything is launched, a walk indexes the components with it -- first itself.  `also` (n words, into
// alsoHost) is the seam's own index array, read back in the same trip.  A seam makes its own checks -- the number of own paths, of
// pairs or of zones, the null arrays, the work buffer -- in front of this, so a call with one fault is refused with the text it always
// had, and of two faults the seam's own is the one named.  A seam without a radius (the zones') passes 1.
int mc_seam_checks(const char* who, mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t steps, int32_t particles, double dt,
                   double radius, const double* Phi, const double* Q, const int32_t* first, const int32_t* also, size_t n, std::vector<int32_t>& alsoHost) {
    MHT_REQUIRE(nx == 4 || nx == 6, "%s: nx must be 4 or 6 (got %d)", who, nx);
    MHT_REQUIRE(transition == 0 || (transition == 1 && nx == 6), "%s: transition is 0 (linear) or, with nx 6, 1 (constant turn) (got %d, nx %d)", who, transition, nx);
    MHT_REQUIRE(nComp >= 1 && nTarget >= 1 && nTarget <= nComp, "%s: 1 <= nTarget <= nComp is wanted (got %d targets, %d components)", who, nTarget, nComp);
    MHT_REQUIRE(steps >= 1 && steps <= MC_MAX_STEPS, "%s: steps must be 1 .. %d (got %d)", who, MC_MAX_STEPS, steps);
    MHT_REQUIRE(particles >= MC_WARP && particles <= MC_MAX_PARTICLES && particles % MC_WARP == 0, "%s: particles must be a multiple of %d in %d .. %d (got %d)", who,
                MC_WARP, MC_WARP, MC_MAX_PARTICLES, particles);
    MHT_REQUIRE(radius > 0.0 && dt > 0.0 && mc_finite(radius) && mc_finite(dt), "%s: the radius and the step must be positive and finite (R %g, dt %g)", who, radius, dt);
    for (int c = 0; c < nx * nx; ++c) MHT_REQUIRE(mc_finite(Q[c]) && (transition == 1 || mc_finite(Phi[c])), "%s: Phi and Q must be finite (entry %d)", who, c);
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<int32_t> f((size_t)nTarget + 1);
    alsoHost.resize(n);
    MHT_HIP_CHECK(hipMemcpyAsync(f.data(), first, f.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (n) MHT_HIP_CHECK(hipMemcpyAsync(alsoHost.data(), also, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MHT_REQUIRE(f[0] == 0 && f[(size_t)nTarget] == nComp, "%s: first runs from 0 to nComp = %d (got %d .. %d)", who, nComp, f[0], f[(size_t)nTarget]);
    for (int t = 0; t < nTarget; ++t)
        MHT_REQUIRE(f[(size_t)t + 1] > f[(size_t)t], "%s: first does not ascend at target %d (%d, then %d)", who, t, f[(size_t)t], f[(size_t)t + 1]);
    return MHT_OK;
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_mc_work_bytes(int32_t nx, int32_t nComp, int32_t nTarget, int32_t G, int32_t steps, int32_t particles) {
    if (!mc_sizes_fit(nx, nComp, nTarget, steps, particles) || G < 1 || G > MC_MAX_PATHS) return 0;
    return mc_layout(nx, nComp, nTarget, G * (steps + 2), particles).bytes;
}

extern "C" size_t mht_mc_pair_work_bytes(int32_t nx, int32_t nComp, int32_t nTarget, int32_t nPair, int32_t steps, int32_t particles) {
    if (!mc_sizes_fit(nx, nComp, nTarget, steps, particles) || nPair < 1 || nPair > MC_MAX_PAIRS) return 0;
    return mc_layout(nx, nComp, nPair, 2 * (steps + 1) + 1, particles).bytes;
}

extern "C" int mht_mc_encounters(mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t G, int32_t steps, int32_t particles,
                                 uint64_t seed, double dt, double radius, const double* Phi, const double* Q, const double* x, const double* P,
                                 const int32_t* first, const double* cdf, const double* ownPath, uint32_t* within, uint32_t* ever, uint32_t* valid,
                                 int32_t* status, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx, "mht_mc_encounters: null context");
    MHT_REQUIRE(G >= 1 && G <= MC_MAX_PATHS, "mht_mc_encounters: G must be 1 .. %d own paths (got %d)", MC_MAX_PATHS, G);
    MHT_REQUIRE((Phi || transition == 1) && Q && x && P && first && cdf && ownPath && within && ever && valid && status && work, "mht_mc_encounters: null array");
    const size_t need = mht_mc_work_bytes(nx, nComp, nTarget, G, steps, particles);
    MHT_REQUIRE(work_bytes >= need, "mht_mc_encounters: the work buffer holds %zu bytes, %zu are needed", work_bytes, need);
    std::vector<int32_t> none;
    int rc = mc_seam_checks("mht_mc_encounters", ctx, nx, transition, nComp, nTarget, steps, particles, dt, radius, Phi, Q, first, nullptr, 0, none);
    if (rc != MHT_OK) return rc;
    rc = mc_dispatch(nx, transition, [&](auto n, auto turning) -> int {
        constexpr int N = decltype(n)::value;
        constexpr bool CT = decltype(turning)::value;
        McModel<N> m;
        MHT_REQUIRE(mc_model<N>(CT ? nullptr : Phi, Q, dt, radius, m), "mht_mc_encounters: Q is not positive semidefinite");
        return mc_run<N, CT>(ctx, nComp, nTarget, G, steps, particles, seed, m, x, P, first, cdf, ownPath, within, ever, valid, status, (char*)work);
    });
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}

extern "C" int mht_mc_pair_encounters(mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t nPair, int32_t steps,
                                      int32_t particles, uint64_t seed, double dt, double radius, const double* Phi, const double* Q, const double* x,
                                      const double* P, const int32_t* first, const double* cdf, const int32_t* pairs, uint32_t* within, uint32_t* firstAt,
                                      uint32_t* ever, uint32_t* valid, int32_t* status, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx, "mht_mc_pair_encounters: null context");
    MHT_REQUIRE(nPair >= 1 && nPair <= MC_MAX_PAIRS, "mht_mc_pair_encounters: nPair must be 1 .. %d pairs (got %d)", MC_MAX_PAIRS, nPair);
    MHT_REQUIRE((Phi || transition == 1) && Q && x && P && first && cdf && pairs && within && firstAt && ever && valid && status && work,
                "mht_mc_pair_encounters: null array");
    const size_t need = mht_mc_pair_work_bytes(nx, nComp, nTarget, nPair, steps, particles);
    MHT_REQUIRE(work_bytes >= need, "mht_mc_pair_encounters: the work buffer holds %zu bytes, %zu are needed", work_bytes, need);
    // (pairs lives on the device as first does, and is read back with it: a walk indexes first with pairs)
    std::vector<int32_t> pr;
    int rc = mc_seam_checks("mht_mc_pair_encounters", ctx, nx, transition, nComp, nTarget, steps, particles, dt, radius, Phi, Q, first, pairs, (size_t)nPair * 2, pr);
    if (rc != MHT_OK) return rc;
    for (int j = 0; j < nPair; ++j) {
        const int32_t pa = pr[2 * (size_t)j], pb = pr[2 * (size_t)j + 1];
        MHT_REQUIRE(pa >= 0 && pa < nTarget && pb >= 0 && pb < nTarget && pa != pb,
                    "mht_mc_pair_encounters: pair %d is (%d, %d); two distinct targets in 0 .. %d are wanted", j, pa, pb, nTarget - 1);
    }
    rc = mc_dispatch(nx, transition, [&](auto n, auto turning) -> int {
        constexpr int N = decltype(n)::value;
        constexpr bool CT = decltype(turning)::value;
        McModel<N> m;
        MHT_REQUIRE(mc_model<N>(CT ? nullptr : Phi, Q, dt, radius, m), "mht_mc_pair_encounters: Q is not positive semidefinite");
        return mc_pair_run<N, CT>(ctx, nComp, nPair, steps, particles, seed, m, x, P, first, cdf, pairs, within, firstAt, ever, valid, status, (char*)work);
    });
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
