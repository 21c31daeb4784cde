// mht_mc_zone_encounters (include/mht_amd.h): guard zones by Monte Carlo -- the particles of mht_mc_encounters, drawn from every
// target's mixture of components and walked with process noise (linear or constant turn), counted against nZone polygons: inside a
// zone at a step, entering it first at a step (at the step, or on the segment that ends in it), entering it at all (the definition,
// the geometry and the skip of a far zone: mht_mc_zone.h).  Three launches on the context's stream -- factor, walk, fold -- and no
// atomic: every word has one writer, and the counts are integers, so the result is the same bits from run to run whatever the grid.
// The factor and the fold are mht_mc.hip's kernels, launched through mht_mc_seam.h; the walk kernel is this unit's, and stores its
// workgroup's counts to part[chunk][word][target], which the fold sums over the chunks into inside, firstAt and ever.
#include <vector>
#include "mht_common.h"
#include "mht_mc_zone.h"
#include "mht_mc_seam.h"

namespace mht {

constexpr int MC_ZONE_CELLS = MC_ZONE_MAX_ZONES * MC_ROW;      // words of one array, inside or firstAt, in LDS, whatever nZone and K are
constexpr int MC_ZONE_WORDS = 2 * MC_ZONE_CELLS + MC_ZONE_MAX_ZONES;      // inside, firstAt, ever: 4 192 words, 16.8 KB
constexpr int MC_ZONE_PAD = 64 - MC_ZONE_MAX_ZONES;      // words behind ever [32] that lanes 32 .. 63 of the first wavefront add their 0 to

template <int N>
struct McZoneWalkArgs {
    McModel<N> m;
    int32_t nComp, T, nZone, nVert, K, S, chunks, slab;
    uint64_t seed;
    const double* x;
    const double* Lw;
    const int32_t* cstatus;
    const int32_t* first;          // dev [T + 1]
    const double* cdf;
    const int32_t* zoneFirst;      // dev [nZone + 1]
    const double* zoneXY;          // dev [nVert][2]
    uint32_t* part;                // [chunks][2 nZone (K + 1) + nZone][T]: inside [nZone][K + 1], firstAt [nZone][K + 1], then ever [nZone]
    int32_t* tstatus;              // [T]
    int32_t target, chunk;         // (not arguments: the workgroup's target and chunk, put here by its first lane)
};

// What mc_zone_walk hands its predicates to, in a workgroup.  Lane z of a wavefront keeps the wavefront's count of zone z's inside at
// this step, lane 32 + z that of its firstAt; at the end of a particle lane z keeps zone z's ever.
struct McZoneWaveSink {
    uint32_t* cnt;                       // LDS: inside [32][MC_ROW], firstAt [32][MC_ROW], ever [32]: a lane of the first wavefront a row
    uint32_t (*stage)[MC_WAVES][64];     // LDS [2]
    int lane, wave, event;
    uint32_t mine;

    __device__ void path(int, const double*) {}
    __device__ bool any(bool near) { return __ballot(near) != 0ull; }      // (the same in every lane of the wavefront: a scalar branch)
    __device__ void step(int z, int, bool in, bool first) {
        const uint32_t bi = (uint32_t)__popcll(__ballot(in)), bf = (uint32_t)__popcll(__ballot(first));
        mine = lane == z ? bi : (lane == MC_ZONE_MAX_ZONES + z ? bf : mine);
    }
    __device__ void flush(int word) {      // word: the word of this lane at this event
        stage[event & 1][wave][lane] = mine;
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(wave) == 0) {      // (a scalar branch: the first wavefront owns the words)
            uint32_t s = stage[event & 1][0][lane];
#pragma unroll
            for (int w = 1; w < MC_WAVES; ++w) s += stage[event & 1][w][lane];
            cnt[word] += s;
        }
        ++event;
        mine = 0;
    }
    // lane l < 32: inside of zone l; lane 32 + l: firstAt of zone l -- the rows follow each other in cnt, so the word is lane * MC_ROW + k
    __device__ void step_done(int k) { flush(lane * MC_ROW + k); }
    __device__ void ever(int z, bool came) {
        const uint32_t b = (uint32_t)__popcll(__ballot(came));
        mine = lane == z ? b : mine;
    }
    // (lanes 32 .. 63 hold 0 here and add it to the words behind ever's: the array's padding, MC_ZONE_PAD)
    __device__ void particle_done() { flush(2 * MC_ZONE_CELLS + lane); }
};

// ONE WORKGROUP of 256 lanes PER (target, chunk) by mc_chunks(T, S), one lane one particle, looped over the chunk's slab, as
// mc_walk_kernel (mht_mc.hip).  The zones are staged in LDS -- the vertices (16 KB at the limit), zoneFirst and the boxes, which lane z
// takes from zone z's staged vertices -- and read there at addresses that are the same in every lane.  Per (zone, step) a wavefront
// asks by a ballot whether any of its lanes' segment boxes overlaps the zone's box and, if none does, leaves the zone's edge loop out
// by a scalar branch (mht_mc_zone.h: the skip does not move a result).  The counts live in LDS at the limits' size, 16.8 KB, so that a
// lane of the first wavefront owns a row: per (zone, step) a wavefront takes __popcll(__ballot(in)) and __popcll(__ballot(first)), lane
// z keeps the one and lane 32 + z the other; per step every lane puts its figure into a staging row of its wavefront, and behind ONE
// barrier the lanes of the first wavefront add the four rows to their words: one owner per word, no LDS atomic.  The staging is
// double-buffered by the parity of the event, so one barrier per step serves.  EVERY BARRIER is in control flow that is the same over
// the workgroup -- the step loop and the slab loop, never inside the skip and never behind a lane's data; a lane beyond the slab's end
// walks along and counts nowhere.  At its end the workgroup stores its slab to part[chunk][word][t].
template <int N, bool CT>
__global__ void __launch_bounds__(MC_THREADS) mc_zone_walk_kernel(const McZoneWalkArgs<N> a) {
    __shared__ double zxy[MC_ZONE_MAX_VERTS * 2];
    __shared__ double zbox[MC_ZONE_MAX_ZONES * 4];
    __shared__ int32_t zfirst[MC_ZONE_MAX_ZONES + 1];
    __shared__ uint32_t cnt[MC_ZONE_WORDS + MC_ZONE_PAD];
    __shared__ uint32_t stage[2][MC_WAVES][64];
    __shared__ McZoneWalkArgs<N> s;
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
    // (nZone <= 32 and nVert <= 1024, the seam's checks: the staged arrays hold them)
    for (int i = tid; i < 2 * a.nVert; i += MC_THREADS) zxy[i] = a.zoneXY[i];
    for (int i = tid; i <= a.nZone; i += MC_THREADS) zfirst[i] = a.zoneFirst[i];
    for (int i = tid; i < MC_ZONE_WORDS + MC_ZONE_PAD; i += MC_THREADS) cnt[i] = 0;
    if (tid == 0) {
        s.target = t;
        s.chunk = chunk;
    }
    __syncthreads();
    if (tid < s.nZone) mc_zone_box(zxy, zfirst[tid], zfirst[tid + 1], zbox + 4 * tid);
    __syncthreads();
    // (the particle index, the slab's end and the sink's event count start from staged words: vector registers)
    const uint32_t begin = (uint32_t)s.chunk * (uint32_t)s.slab;
    const uint32_t end = begin + (uint32_t)s.slab < (uint32_t)s.S ? begin + (uint32_t)s.slab : (uint32_t)s.S;
    McZoneWaveSink sink = {cnt, stage, tid & 63, tid >> 6, s.chunk - chunk, 0u};
    const McZones zs = {zfirst, zxy, zbox, a.nZone};
    uint32_t base = begin;      // (begin < end: no chunk is empty)
    do {                        // (the same trips in every lane of the workgroup: the barriers)
        const uint32_t p = base + (uint32_t)tid;
        mc_zone_walk<N, CT>(s.m, s.x, s.Lw, s.first, s.cdf, s.nComp, a.K, s.seed, s.target, p, p < end, zs, sink);
        base += MC_THREADS;
    } while (__builtin_amdgcn_readfirstlane((int)(base < end)) != 0);
    __syncthreads();
    // (from the staged copy: nothing of the store stays in a scalar register over the walk)
    const int K1 = s.K + 1, cells = s.nZone * K1;
    const size_t T = (size_t)s.T, at = (size_t)s.chunk * (size_t)(2 * cells + s.nZone), tt = (size_t)s.target;
    for (int i = tid; i < 2 * cells; i += MC_THREADS) {
        const int arr = i / cells, j = i % cells;
        s.part[(at + (size_t)i) * T + tt] = cnt[arr * MC_ZONE_CELLS + j / K1 * MC_ROW + j % K1];
    }
    for (int z = tid; z < s.nZone; z += MC_THREADS) s.part[(at + 2 * (size_t)cells + (size_t)z) * T + tt] = cnt[2 * MC_ZONE_CELLS + z];
}

static int32_t mc_zone_words(int32_t nZone, int32_t K) { return 2 * nZone * (K + 1) + nZone; }

template <int N, bool CT>
static int mc_zone_run(mht_ctx* ctx, int32_t nComp, int32_t T, int32_t nZone, int32_t nVert, int32_t K, int32_t S, uint64_t seed, const McModel<N>& m, const double* x,
                       const double* P, const int32_t* first, const double* cdf, const int32_t* zoneFirst, const double* zoneXY, uint32_t* inside,
                       uint32_t* firstAt, uint32_t* ever, uint32_t* valid, int32_t* status, char* work) {
    const int32_t words = mc_zone_words(nZone, K);
    const McLayout l = mc_layout(N, nComp, T, words, S);
    double* Lw = (double*)(work + l.Lw);
    uint32_t* part = (uint32_t*)(work + l.part);
    int32_t* cs = (int32_t*)(work + l.cstatus);
    int32_t* ts = (int32_t*)(work + l.istatus);
    int rc = mc_launch_factor(ctx, N, nComp, x, P, cdf, Lw, cs);
    if (rc != MHT_OK) return rc;
    const McZoneWalkArgs<N> wa = {m, nComp, T, nZone, nVert, K, S, l.split.chunks, l.split.slab, seed, x, Lw, cs, first, cdf, zoneFirst, zoneXY, part, ts, 0, 0};
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, mc_zone_walk_kernel<N, CT>, dim3((unsigned)T * (unsigned)l.split.chunks), dim3(MC_THREADS), 0, false, wa);
    if (rc != MHT_OK) return rc;
    return mc_launch_fold(ctx, McFoldArgs{T, words, l.split.chunks, S, part, ts, inside, firstAt, ever, nZone * (K + 1), 2 * nZone * (K + 1), valid, status});
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_mc_zone_work_bytes(int32_t nx, int32_t nComp, int32_t nTarget, int32_t nZone, int32_t steps, int32_t particles) {
    if (!mc_sizes_fit(nx, nComp, nTarget, steps, particles) || nZone < 1 || nZone > MC_ZONE_MAX_ZONES) return 0;
    return mc_layout(nx, nComp, nTarget, mc_zone_words(nZone, steps), particles).bytes;
}

extern "C" int mht_mc_zone_encounters(mht_ctx* ctx, int32_t nx, int32_t transition, int32_t nComp, int32_t nTarget, int32_t nZone, int32_t nVert, int32_t steps,
                                      int32_t particles, uint64_t seed, double dt, const double* Phi, const double* Q, const double* x, const double* P,
                                      const int32_t* first, const double* cdf, const int32_t* zoneFirst, const double* zoneXY, uint32_t* inside, uint32_t* firstAt,
                                      uint32_t* ever, uint32_t* valid, int32_t* status, void* work, size_t work_bytes) {
    const char* who = "mht_mc_zone_encounters";
    MHT_REQUIRE(ctx, "%s: null context", who);
    MHT_REQUIRE(nZone >= 1 && nZone <= MC_ZONE_MAX_ZONES, "%s: nZone must be 1 .. %d zones (got %d)", who, MC_ZONE_MAX_ZONES, nZone);
    MHT_REQUIRE(nVert >= MC_ZONE_MIN_VERTS * nZone && nVert <= MC_ZONE_MAX_VERTS, "%s: nVert must be %d per zone at least and %d in all at most (got %d for %d zones)",
                who, MC_ZONE_MIN_VERTS, MC_ZONE_MAX_VERTS, nVert, nZone);
    MHT_REQUIRE((Phi || transition == 1) && Q && x && P && first && cdf && zoneFirst && zoneXY && inside && firstAt && ever && valid && status && work,
                "%s: null array", who);
    const size_t need = mht_mc_zone_work_bytes(nx, nComp, nTarget, nZone, steps, particles);
    MHT_REQUIRE(work_bytes >= need, "%s: the work buffer holds %zu bytes, %zu are needed", who, work_bytes, need);
    // (zoneFirst and zoneXY live on the device as first does: read back and checked before anything is launched -- the walk stages
    // them in arrays of the limits' size and indexes the vertices with zoneFirst.  There is no radius here: the shared checks get 1)
    std::vector<int32_t> zf;
    int rc = mc_seam_checks(who, ctx, nx, transition, nComp, nTarget, steps, particles, dt, 1.0, Phi, Q, first, zoneFirst, (size_t)nZone + 1, zf);
    if (rc != MHT_OK) return rc;
    MHT_REQUIRE(zf[0] == 0 && zf[(size_t)nZone] == nVert, "%s: zoneFirst runs from 0 to nVert = %d (got %d .. %d)", who, nVert, zf[0], zf[(size_t)nZone]);
    for (int z = 0; z < nZone; ++z)
        MHT_REQUIRE(zf[(size_t)z + 1] >= zf[(size_t)z] + MC_ZONE_MIN_VERTS, "%s: zone %d has the vertices %d .. %d - 1; %d at least are wanted", who, z, zf[(size_t)z],
                    zf[(size_t)z + 1], MC_ZONE_MIN_VERTS);
    std::vector<double> xy((size_t)nVert * 2);
    MHT_HIP_CHECK(hipMemcpyAsync(xy.data(), zoneXY, xy.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < xy.size(); ++i) MHT_REQUIRE(mc_finite(xy[i]), "%s: zoneXY must be finite (vertex %zu)", who, i / 2);
    rc = mc_dispatch(nx, transition, [&](auto n, auto turning) -> int {
        constexpr int N = decltype(n)::value;
        constexpr bool CT = decltype(turning)::value;
        McModel<N> m;
        MHT_REQUIRE(mc_model<N>(CT ? nullptr : Phi, Q, dt, 1.0, m), "%s: Q is not positive semidefinite", who);
        return mc_zone_run<N, CT>(ctx, nComp, nTarget, nZone, nVert, steps, particles, seed, m, x, P, first, cdf, zoneFirst, zoneXY, inside, firstAt, ever, valid,
                                  status, (char*)work);
    });
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
