// mht_mc_domain_encounters (include/mht_amd.h): ship domains by Monte Carlo -- the particles of mht_mc_encounters, drawn from every
// target's mixture of components and walked with process noise (linear or constant turn), taken into the own ship's body frame under
// every candidate path's pose and counted against nDomain polygons drawn in that frame: inside a domain at a step, entering it first
// at a step (at the step, or on the segment that ends in it), entering it at all (the definition, the transform, the straight-chord
// rule and the skip of a far cell: mht_mc_domain.h).  Three launches on the context's stream -- factor, walk, fold -- and no atomic:
// every word has one writer, and the counts are integers, so the result is the same bits from run to run whatever the grid.  The
// factor and the fold are mht_mc.hip's kernels, launched through mht_mc_seam.h; the walk kernel is this unit's, and stores its
// workgroup's counts to part[chunk][word][target], which the fold sums over the chunks into inside, firstAt and ever.
#include <vector>
#include "mht_common.h"
#include "mht_mc_domain.h"
#include "mht_mc_seam.h"

namespace mht {

constexpr int MC_DOMAIN_ROWS = MC_DOMAIN_MAX_CELLS * MC_ROW;      // words of one array, inside or firstAt, in LDS, whatever nCell and K are
constexpr int MC_DOMAIN_WORDS = 2 * MC_DOMAIN_ROWS + MC_DOMAIN_MAX_CELLS;      // inside, firstAt, ever: 8 384 words, 33.5 KB

template <int N>
struct McDomainWalkArgs {
    McModel<N> m;
    int32_t nComp, T, G, nDomain, nVert, K, S, chunks, slab, pad;
    uint64_t seed;
    const double* x;
    const double* Lw;
    const int32_t* cstatus;
    const int32_t* first;         // dev [T + 1]
    const double* cdf;
    const double* pose;           // dev [G][K + 1][4]
    const int32_t* domFirst;      // dev [nDomain + 1]
    const double* domXY;          // dev [nVert][2]
    uint32_t* part;               // [chunks][2 nCell (K + 1) + nCell][T]: inside [nCell][K + 1], firstAt [nCell][K + 1], then ever [nCell]
    int32_t* tstatus;             // [T]
    int32_t target, chunk;        // (not arguments: the workgroup's target and chunk, put here by its first lane)
};

// What mc_domain_walk hands its predicates to, in a workgroup.  Lane c of a wavefront keeps the wavefront's two figures of cell c at
// this step, inside and firstAt; at the end of a particle lane c keeps cell c's ever.
struct McDomainWaveSink {
    uint32_t* cnt;                            // LDS: inside [64][MC_ROW], firstAt [64][MC_ROW], ever [64]: a lane of the first wavefront a cell
    uint32_t (*stage)[MC_WAVES][2][64];       // LDS [2]: a row of inside and of firstAt per wavefront, by the parity of the event
    int lane, wave, event;
    uint32_t mi, mf;

    __device__ void path(int, const double*) {}
    __device__ bool any(bool near) { return __ballot(near) != 0ull; }      // (the same in every lane of the wavefront: a scalar branch)
    __device__ void step(int c, int, bool in, bool first) {
        const uint32_t bi = (uint32_t)__popcll(__ballot(in)), bf = (uint32_t)__popcll(__ballot(first));
        mi = lane == c ? bi : mi;
        mf = lane == c ? bf : mf;
    }
    // ONE barrier per event, in control flow that is the same over the workgroup; the first wavefront owns the words
    __device__ void step_done(int k) {
        stage[event & 1][wave][0][lane] = mi;
        stage[event & 1][wave][1][lane] = mf;
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(wave) == 0) {
            uint32_t si = stage[event & 1][0][0][lane], sf = stage[event & 1][0][1][lane];
#pragma unroll
            for (int w = 1; w < MC_WAVES; ++w) {
                si += stage[event & 1][w][0][lane];
                sf += stage[event & 1][w][1][lane];
            }
            cnt[lane * MC_ROW + k] += si;
            cnt[MC_DOMAIN_ROWS + lane * MC_ROW + k] += sf;
        }
        ++event;
        mi = 0;
        mf = 0;
    }
    __device__ void ever(int c, bool came) {
        const uint32_t b = (uint32_t)__popcll(__ballot(came));
        mi = lane == c ? b : mi;
    }
    __device__ void particle_done() {
        stage[event & 1][wave][0][lane] = mi;
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(wave) == 0) {
            uint32_t s = stage[event & 1][0][0][lane];
#pragma unroll
            for (int w = 1; w < MC_WAVES; ++w) s += stage[event & 1][w][0][lane];
            cnt[2 * MC_DOMAIN_ROWS + lane] += s;
        }
        ++event;
        mi = 0;
    }
};

// ONE WORKGROUP of 256 lanes PER (target, chunk) by mc_chunks(T, S), one lane one particle, looped over the chunk's slab, as
// mc_walk_kernel (mht_mc.hip) and mc_zone_walk_kernel (mht_mc_zone.hip).  The domains are staged in LDS -- the vertices (4 KB at the
// limit), domFirst and the boxes, which lane d takes from domain d's staged vertices -- and read there at addresses that are the same
// in every lane.  THE POSES STAY IN GLOBAL MEMORY, read at addresses that are the same over the wavefront: at the limits they are 133 KB
// and do not fit LDS.  Per (path, step) a lane takes its particle into the path's body frame once, and its previous position under the
// previous pose (mht_mc_domain.h: two doubles kept, not 64 body-frame points); per cell a wavefront asks by a ballot whether any of its
// lanes' segment boxes overlaps the domain's box and, if none does, leaves the edge loop out by a scalar branch.  The counts live in
// LDS at the limits' size, 33.5 KB, so that a lane of the first wavefront owns a cell's rows: per cell a wavefront takes
// __popcll(__ballot(in)) and __popcll(__ballot(first)) and lane c keeps both; per step every lane puts its two figures into its
// wavefront's staging rows, and behind ONE barrier the lanes of the first wavefront add the four wavefronts' rows to their words: one
// owner per word, no LDS atomic.  The staging is double-buffered by the parity of the event, so one barrier per step serves.  EVERY
// BARRIER is in control flow that is the same over the workgroup -- the step loop and the slab loop, never inside the skip and never
// behind a lane's data; a lane beyond the slab's end walks along and counts nowhere.  At its end the workgroup stores its slab to
// part[chunk][word][t].
template <int N, bool CT>
__global__ void __launch_bounds__(MC_THREADS) mc_domain_walk_kernel(const McDomainWalkArgs<N> a) {
    __shared__ double dxy[MC_DOMAIN_MAX_VERTS * 2];
    __shared__ double dbox[MC_DOMAIN_MAX_DOMAINS * 4];
    __shared__ int32_t dfirst[MC_DOMAIN_MAX_DOMAINS + 1];
    __shared__ uint32_t cnt[MC_DOMAIN_WORDS];
    __shared__ uint32_t stage[2][MC_WAVES][2][64];
    __shared__ McDomainWalkArgs<N> s;
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
    // (nDomain <= 4, nVert <= 256 and nDomain * G <= 64, the seam's checks: the staged arrays hold them)
    for (int i = tid; i < 2 * a.nVert; i += MC_THREADS) dxy[i] = a.domXY[i];
    for (int i = tid; i <= a.nDomain; i += MC_THREADS) dfirst[i] = a.domFirst[i];
    for (int i = tid; i < MC_DOMAIN_WORDS; i += MC_THREADS) cnt[i] = 0;
    if (tid == 0) {
        s.target = t;
        s.chunk = chunk;
    }
    __syncthreads();
    if (tid < s.nDomain) mc_zone_box(dxy, dfirst[tid], dfirst[tid + 1], dbox + 4 * tid);
    __syncthreads();
    // (the particle index, the slab's end and the sink's event count start from staged words: vector registers)
    const uint32_t begin = (uint32_t)s.chunk * (uint32_t)s.slab;
    const uint32_t end = begin + (uint32_t)s.slab < (uint32_t)s.S ? begin + (uint32_t)s.slab : (uint32_t)s.S;
    McDomainWaveSink sink = {cnt, stage, tid & 63, tid >> 6, s.chunk - chunk, 0u, 0u};
    const McDomains ds = {dfirst, dxy, dbox, a.nDomain};
    uint32_t base = begin;      // (begin < end: no chunk is empty)
    do {                        // (the same trips in every lane of the workgroup: the barriers)
        const uint32_t p = base + (uint32_t)tid;
        mc_domain_walk<N, CT>(s.m, s.x, s.Lw, s.first, s.cdf, a.pose, s.nComp, a.G, a.K, s.seed, s.target, p, p < end, ds, sink);
        base += MC_THREADS;
    } while (__builtin_amdgcn_readfirstlane((int)(base < end)) != 0);
    __syncthreads();
    // (from the staged copy: nothing of the store stays in a scalar register over the walk)
    const int K1 = s.K + 1, nCell = s.nDomain * s.G, cells = nCell * K1;
    const size_t T = (size_t)s.T, at = (size_t)s.chunk * (size_t)(2 * cells + nCell), tt = (size_t)s.target;
    for (int i = tid; i < 2 * cells; i += MC_THREADS) {
        const int arr = i / cells, j = i % cells;
        s.part[(at + (size_t)i) * T + tt] = cnt[arr * MC_DOMAIN_ROWS + j / K1 * MC_ROW + j % K1];
    }
    for (int c = tid; c < nCell; c += MC_THREADS) s.part[(at + 2 * (size_t)cells + (size_t)c) * T + tt] = cnt[2 * MC_DOMAIN_ROWS + c];
}

static int32_t mc_domain_words(int32_t nCell, int32_t K) { return 2 * nCell * (K + 1) + nCell; }

static bool mc_domain_cells_fit(int32_t G, int32_t nDomain) {
    return G >= 1 && G <= MC_DOMAIN_MAX_CELLS && nDomain >= 1 && nDomain <= MC_DOMAIN_MAX_DOMAINS && nDomain * G <= MC_DOMAIN_MAX_CELLS;
}

template <int N, bool CT>
static int mc_domain_run(mht_ctx* ctx, int32_t nComp, int32_t T, int32_t G, int32_t nDomain, int32_t nVert, int32_t K, int32_t S, uint64_t seed, const McModel<N>& m,
                         const double* x, const double* P, const int32_t* first, const double* cdf, const double* pose, const int32_t* domFirst,
                         const double* domXY, uint32_t* inside, uint32_t* firstAt, uint32_t* ever, uint32_t* valid, int32_t* status, char* work) {
    const int32_t nCell = nDomain * G, words = mc_domain_words(nCell, K);
    const McLayout l = mc_layout(N, nComp, T, words, S);
    double* Lw = (double*)(work + l.Lw);
    uint32_t* part = (uint32_t*)(work + l.part);
    int32_t* cs = (int32_t*)(work + l.cstatus);
    int32_t* ts = (int32_t*)(work + l.istatus);
    int rc = mc_launch_factor(ctx, N, nComp, x, P, cdf, Lw, cs);
    if (rc != MHT_OK) return rc;
    const McDomainWalkArgs<N> wa = {m, nComp, T, G, nDomain, nVert, K, S, l.split.chunks, l.split.slab, 0, seed, x, Lw, cs, first, cdf, pose, domFirst, domXY, part, ts, 0, 0};
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, mc_domain_walk_kernel<N, CT>, dim3((unsigned)T * (unsigned)l.split.chunks), dim3(MC_THREADS), 0, false, wa);
    if (rc != MHT_OK) return rc;
    return mc_launch_fold(ctx, McFoldArgs{T, words, l.split.chunks, S, part, ts, inside, firstAt, ever, nCell * (K + 1), 2 * nCell * (K + 1), valid, status});
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_mc_domain_work_bytes(int32_t nx, int32_t nComp, int32_t nTarget, int32_t G, int32_t nDomain, int32_t steps, int32_t particles) {
    if (!mc_sizes_fit(nx, nComp, nTarget, steps, particles) || !mc_domain_cells_fit(G, nDomain)) return 0;
    return mc_layout(nx, nComp, nTarget, mc_domain_words(nDomain * G, steps), particles).bytes;
}

extern "C" int mht_mc_domain_encounters(mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t G, int32_t nDomain, int32_t nVert,
                                        int32_t steps, int32_t particles, uint64_t seed, double dt, const double* Phi, const double* Q, const double* x,
                                        const double* P, const int32_t* first, const double* cdf, const double* ownPose, const int32_t* domFirst,
                                        const double* domXY, uint32_t* inside, uint32_t* firstAt, uint32_t* ever, uint32_t* valid, int32_t* status, void* work,
                                        size_t work_bytes) {
    const char* who = "mht_mc_domain_encounters";
    MHT_REQUIRE(ctx, "%s: null context", who);
    MHT_REQUIRE(nDomain >= 1 && nDomain <= MC_DOMAIN_MAX_DOMAINS, "%s: nDomain must be 1 .. %d domains (got %d)", who, MC_DOMAIN_MAX_DOMAINS, nDomain);
    MHT_REQUIRE(mc_domain_cells_fit(G, nDomain), "%s: G must be 1 own path at least, and nDomain * G %d cells at most (got %d domains x %d paths)", who,
                MC_DOMAIN_MAX_CELLS, nDomain, G);
    MHT_REQUIRE(nVert >= MC_ZONE_MIN_VERTS * nDomain && nVert <= MC_DOMAIN_MAX_VERTS, "%s: nVert must be %d per domain at least and %d in all at most (got %d for %d domains)",
                who, MC_ZONE_MIN_VERTS, MC_DOMAIN_MAX_VERTS, nVert, nDomain);
    MHT_REQUIRE((Phi || transition == 1) && Q && x && P && first && cdf && ownPose && domFirst && domXY && inside && firstAt && ever && valid && status && work,
                "%s: null array", who);
    const size_t need = mht_mc_domain_work_bytes(nx, nComp, nTarget, G, nDomain, steps, particles);
    MHT_REQUIRE(work_bytes >= need, "%s: the work buffer holds %zu bytes, %zu are needed", who, work_bytes, need);
    // (domFirst, domXY and ownPose live on the device as first does: read back and checked before anything is launched -- the walk
    // stages the domains in arrays of the limits' size and indexes the vertices with domFirst.  There is no radius here: the shared
    // checks get 1)
    std::vector<int32_t> df;
    int rc = mc_seam_checks(who, ctx, nx, transition, nComp, nTarget, steps, particles, dt, 1.0, Phi, Q, first, domFirst, (size_t)nDomain + 1, df);
    if (rc != MHT_OK) return rc;
    MHT_REQUIRE(df[0] == 0 && df[(size_t)nDomain] == nVert, "%s: domFirst runs from 0 to nVert = %d (got %d .. %d)", who, nVert, df[0], df[(size_t)nDomain]);
    for (int d = 0; d < nDomain; ++d)
        MHT_REQUIRE(df[(size_t)d + 1] >= df[(size_t)d] + MC_ZONE_MIN_VERTS, "%s: domain %d has the vertices %d .. %d - 1; %d at least are wanted", who, d, df[(size_t)d],
                    df[(size_t)d + 1], MC_ZONE_MIN_VERTS);
    std::vector<double> xy((size_t)nVert * 2), pose((size_t)G * (size_t)(steps + 1) * 4);
    MHT_HIP_CHECK(hipMemcpyAsync(xy.data(), domXY, xy.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MHT_HIP_CHECK(hipMemcpyAsync(pose.data(), ownPose, pose.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < xy.size(); ++i) MHT_REQUIRE(mc_finite(xy[i]), "%s: domXY must be finite (vertex %zu)", who, i / 2);
    for (size_t i = 0; i < pose.size(); i += 4) {
        const double ux = pose[i + 2], uy = pose[i + 3];
        MHT_REQUIRE(mc_finite(pose[i]) && mc_finite(pose[i + 1]) && mc_finite(ux) && mc_finite(uy), "%s: ownPose must be finite (path %zu, step %zu)", who,
                    i / 4 / (size_t)(steps + 1), i / 4 % (size_t)(steps + 1));
        MHT_REQUIRE(fabs(ux * ux + uy * uy - 1.0) <= MC_DOMAIN_UNIT_TOL, "%s: a heading must be a unit vector, |ux^2 + uy^2 - 1| <= %g (path %zu, step %zu: %.17g, %.17g)",
                    who, MC_DOMAIN_UNIT_TOL, i / 4 / (size_t)(steps + 1), i / 4 % (size_t)(steps + 1), ux, uy);
    }
    rc = mc_dispatch(nx, transition, [&](auto n, auto turning) -> int {
        constexpr int N = decltype(n)::value;
        constexpr bool CT = decltype(turning)::value;
        McModel<N> m;
        MHT_REQUIRE(mc_model<N>(CT ? nullptr : Phi, Q, dt, 1.0, m), "%s: Q is not positive semidefinite", who);
        return mc_domain_run<N, CT>(ctx, nComp, nTarget, G, nDomain, nVert, steps, particles, seed, m, x, P, first, cdf, ownPose, domFirst, domXY, inside, firstAt,
                                    ever, valid, status, (char*)work);
    });
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
