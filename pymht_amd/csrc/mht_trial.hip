// mht_trial_manoeuvres (include/mht_amd.h): G candidate manoeuvres of the own ship against n tracks in one call -- the table of
// candidates x tracks of the encounter figures, and per candidate the worst track (the manoeuvre and the fold: mht_trial.h; the
// figures of a cell: mht_encounter.h).  The trajectories of all n + G entries live in the work buffer, pos [K + 1][2][n + G] and
// S [K + 1][3][n + G], entry-minor: tracks are entries 0 .. n - 1, candidates n .. n + G - 1.  Four launches on the context's stream:
//
// trial_propagate_kernel<N>: ONE TRACK PER LANE through encounter_propagate<N>, as encounter_propagate_kernel does, with the entry
// stride n + G.  The tracks are propagated once, whatever G is.
//
// trial_candidate_kernel: ONE CANDIDATE PER LANE, the closed form of mht_trial.h; the own ship and the turn rate are wave-uniform
// kernel arguments.
//
// trial_cell_kernel: ONE CELL (g, j) PER LANE of the [G][n] table, j fastest.  A workgroup takes a TILE, candidate g and 256 consecutive
// tracks, and strides over the tiles: g is the same in every lane, so the candidate's trajectory is read through wave-uniform loads
// and the tracks' through coalesced ones, as in encounter_pair_kernel.  Every cell of the five figures is written.  The workgroup then
// folds its tile: xor-shuffles inside a wavefront, four wavefronts through 96 bytes of LDS, and lane 0 stores the tile's partial
// into partials [4][G][tiles per row].  No atomic: every partial has one writer.
//
// trial_summary_kernel: ONE WAVEFRONT PER CANDIDATE folds the row of partials, lane l taking tiles l, l + 64, ... in index order, into
// summary [4][G].  The fold's order is total (mht_trial.h), so the grouping does not show in the bits.
#include "mht_common.h"
#include "mht_trial.h"

namespace mht {

static_assert(TRIAL_MAX_CANDIDATES == MHT_TRIAL_MAX_CANDIDATES, "the bound include/mht_amd.h states");

constexpr int TRIAL_THREADS = TRIAL_TILE;
constexpr int TRIAL_WAVE = 64;
constexpr int TRIAL_MAX_BLOCKS = 2048;

template <int N>
struct TrialPropagateArgs {
    EncounterModel<N> m;
    int32_t n, nt, K;
    const double* x;      // [N][n]
    const double* P;      // [N(N+1)/2][n]
    double* xs;           // [N][nt], the staging
    double* Ps;           // [N(N+1)/2][nt]
    double* pos;          // [K + 1][2][nt]
    double* S;            // [K + 1][3][nt]
};

struct TrialCandidateArgs {
    TrialOwn own;
    int32_t n, G, K;
    double dt;
    const double* cand;      // dev [G][3]
    double* pos;
    double* S;
};

struct TrialCellArgs {
    int32_t n, G, K;
    double dt, R;
    const double* pos;
    const double* S;
    double* out;           // [5][G][n]
    double* partials;      // [4][G][tiles per row]
};

struct TrialSummaryArgs {
    int32_t G, chunks;
    const double* partials;
    double* summary;      // [4][G]
};

__device__ __forceinline__ void trial_fold_wave(TrialBest& b) {
#pragma unroll
    for (int m = 1; m < TRIAL_WAVE; m <<= 1) {
        TrialBest o;
        o.pc = __shfl_xor(b.pc, m, TRIAL_WAVE);
        o.dcpa = __shfl_xor(b.dcpa, m, TRIAL_WAVE);
        o.pcj = __shfl_xor(b.pcj, m, TRIAL_WAVE);
        o.dj = __shfl_xor(b.dj, m, TRIAL_WAVE);
        trial_fold(b, o);
    }
}

template <int N>
__global__ void __launch_bounds__(TRIAL_THREADS) trial_propagate_kernel(const TrialPropagateArgs<N> a) {
    for (size_t t = (size_t)blockIdx.x * TRIAL_THREADS + threadIdx.x; t < (size_t)a.n; t += (size_t)gridDim.x * TRIAL_THREADS)
        trial_track<N>(a.m, a.x, a.P, a.n, a.nt, a.K, (int)t, a.xs, a.Ps, a.pos, a.S);
}

__global__ void __launch_bounds__(TRIAL_THREADS) trial_candidate_kernel(const TrialCandidateArgs a) {
    for (size_t g = (size_t)blockIdx.x * TRIAL_THREADS + threadIdx.x; g < (size_t)a.G; g += (size_t)gridDim.x * TRIAL_THREADS) {
        const double* c = a.cand + 3 * g;
        trial_candidate(a.own, c[0], c[1], c[2], a.n + a.G, a.K, a.dt, a.n + (int)g, a.pos, a.S);
    }
}

__global__ void __launch_bounds__(TRIAL_THREADS) trial_cell_kernel(const TrialCellArgs a) {
    __shared__ double fig[2][TRIAL_THREADS / TRIAL_WAVE];
    __shared__ int arg[2][TRIAL_THREADS / TRIAL_WAVE];
    const size_t chunks = ((size_t)a.n + TRIAL_TILE - 1) / TRIAL_TILE;
    const size_t tiles = (size_t)a.G * chunks;
    const int wave = threadIdx.x / TRIAL_WAVE;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // (the same trips in every lane of the workgroup: the barriers)
        const int g = (int)(tile / chunks);
        const size_t chunk = tile % chunks;
        const size_t j = chunk * TRIAL_TILE + threadIdx.x;
        TrialBest b = trial_none();
        if (j < (size_t)a.n) b = trial_cell(a.pos, a.S, a.n, a.G, a.K, a.dt, a.R, g, (int)j, a.out);
        trial_fold_wave(b);
        if (threadIdx.x % TRIAL_WAVE == 0) {
            fig[0][wave] = b.pc;
            fig[1][wave] = b.dcpa;
            arg[0][wave] = b.pcj;
            arg[1][wave] = b.dj;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            TrialBest t = trial_none();
#pragma unroll
            for (int v = 0; v < TRIAL_THREADS / TRIAL_WAVE; ++v) trial_fold(t, TrialBest{fig[0][v], fig[1][v], arg[0][v], arg[1][v]});
            trial_store(t, a.partials + (size_t)g * chunks + chunk, tiles);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(TRIAL_WAVE) trial_summary_kernel(const TrialSummaryArgs a) {
    const size_t chunks = (size_t)a.chunks, tiles = (size_t)a.G * chunks;
    for (int g = blockIdx.x; g < a.G; g += gridDim.x) {
        TrialBest b = trial_none();
        for (size_t c = threadIdx.x; c < chunks; c += TRIAL_WAVE) trial_fold(b, trial_load(a.partials + (size_t)g * chunks + c, tiles));
        trial_fold_wave(b);
        if (threadIdx.x == 0) trial_store(b, a.summary + g, (size_t)a.G);
    }
}

struct TrialLayout {
    size_t pos, S, partials, xs, Ps, cand, doubles;      // offsets in doubles, and the total
};

// The staging is sized for six states whatever nx is: the sizer does not take nx
static TrialLayout trial_layout(int32_t n, int32_t G, int32_t K) {
    const size_t nt = (size_t)n + (size_t)G, steps = (size_t)(K + 1), chunks = ((size_t)n + TRIAL_TILE - 1) / TRIAL_TILE;
    TrialLayout l;
    l.pos = 0;
    l.S = l.pos + 2 * steps * nt;
    l.partials = l.S + 3 * steps * nt;
    l.xs = l.partials + (size_t)TRIAL_SUMMARY * (size_t)G * chunks;
    l.Ps = l.xs + 6 * nt;
    l.cand = l.Ps + 21 * nt;
    l.doubles = l.cand + 3 * (size_t)G;
    return l;
}

static bool trial_sizes_fit(int32_t n, int32_t G, int32_t K) {
    return n > 0 && G >= 1 && G <= TRIAL_MAX_CANDIDATES && K >= 1 && K <= ENCOUNTER_MAX_STEPS && n <= INT32_MAX - TRIAL_MAX_CANDIDATES;
}

template <int N>
static int trial_run(mht_ctx* ctx, int32_t n, int32_t G, int32_t K, double dt, double R, const double* Phi, const double* Q, const double* x,
                     const double* P, const TrialOwn& own, double* out, double* summary, double* work) {
    const TrialLayout l = trial_layout(n, G, K);
    TrialPropagateArgs<N> pa;
    for (int c = 0; c < N * N; ++c) {
        pa.m.Phi[c] = Phi[c];
        pa.m.Q[c] = Q[c];
    }
    pa.n = n;
    pa.nt = n + G;
    pa.K = K;
    pa.x = x;
    pa.P = P;
    pa.xs = work + l.xs;
    pa.Ps = work + l.Ps;
    pa.pos = work + l.pos;
    pa.S = work + l.S;
    const size_t chunks = ((size_t)n + TRIAL_TILE - 1) / TRIAL_TILE;
    const dim3 grid((unsigned)(chunks < (size_t)TRIAL_MAX_BLOCKS ? chunks : (size_t)TRIAL_MAX_BLOCKS));
    int rc = launch_kernel(ctx, K_SMOOTH_SCORE, trial_propagate_kernel<N>, grid, dim3(TRIAL_THREADS), 0, false, pa);
    if (rc != MHT_OK) return rc;
    const TrialCandidateArgs ca = {own, n, G, K, dt, work + l.cand, pa.pos, pa.S};
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, trial_candidate_kernel, dim3((unsigned)((G + TRIAL_THREADS - 1) / TRIAL_THREADS)), dim3(TRIAL_THREADS), 0, false, ca);
    if (rc != MHT_OK) return rc;
    const TrialCellArgs qa = {n, G, K, dt, R, pa.pos, pa.S, out, work + l.partials};
    const size_t tiles = (size_t)G * chunks;
    const dim3 cgrid((unsigned)(tiles < (size_t)TRIAL_MAX_BLOCKS ? tiles : (size_t)TRIAL_MAX_BLOCKS));
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, trial_cell_kernel, cgrid, dim3(TRIAL_THREADS), 0, false, qa);
    if (rc != MHT_OK) return rc;
    const TrialSummaryArgs sa = {G, (int32_t)chunks, work + l.partials, summary};
    return launch_kernel(ctx, K_SMOOTH_SCORE, trial_summary_kernel, dim3((unsigned)(G < TRIAL_MAX_BLOCKS ? G : TRIAL_MAX_BLOCKS)), dim3(TRIAL_WAVE), 0, false, sa);
}

static bool trial_finite(double v) { return v - v == 0.0; }
static bool trial_finite_or_nan(double v) { return v != v || trial_finite(v); }

}  // namespace mht

using namespace mht;

extern "C" size_t mht_trial_work_bytes(int32_t n, int32_t G, int32_t K) {
    if (!trial_sizes_fit(n, G, K)) return 0;
    return (trial_layout(n, G, K).doubles * sizeof(double) + 255) / 256 * 256;
}

extern "C" int mht_trial_manoeuvres(mht_ctx* ctx, int32_t nx, int32_t n, int32_t G, int32_t K, double dt, double R, const double* Phi,
                                    const double* Q, const double* x, const double* P, const double* own, const double* Sown, double w,
                                    const double* cand, double* out, double* summary, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx, "mht_trial_manoeuvres: null context");
    MHT_REQUIRE(nx == 4 || nx == 6, "mht_trial_manoeuvres: nx must be 4 or 6 (got %d)", nx);
    MHT_REQUIRE(K >= 1 && K <= ENCOUNTER_MAX_STEPS, "mht_trial_manoeuvres: K must be 1 .. %d steps (got %d)", ENCOUNTER_MAX_STEPS, K);
    MHT_REQUIRE(G >= 1 && G <= TRIAL_MAX_CANDIDATES, "mht_trial_manoeuvres: G must be 1 .. %d candidates (got %d)", TRIAL_MAX_CANDIDATES, G);
    MHT_REQUIRE(n >= 0 && n <= INT32_MAX - TRIAL_MAX_CANDIDATES, "mht_trial_manoeuvres: bad number of tracks (%d)", n);
    MHT_REQUIRE(R > 0.0 && dt > 0.0 && w > 0.0 && trial_finite(R) && trial_finite(dt) && trial_finite(w),
                "mht_trial_manoeuvres: the radius, the step and the turn rate must be positive and finite (R %g, dt %g, w %g)", R, dt, w);
    if (n == 0) return MHT_OK;
    MHT_REQUIRE(Phi && Q && x && P && own && Sown && cand && out && summary && work, "mht_trial_manoeuvres: null array");
    TrialOwn o;
    for (int c = 0; c < 4; ++c) MHT_REQUIRE(trial_finite_or_nan(own[c]), "mht_trial_manoeuvres: own[%d] is infinite", c);
    for (int c = 0; c < 3; ++c) MHT_REQUIRE(trial_finite_or_nan(Sown[c]), "mht_trial_manoeuvres: Sown[%d] is infinite", c);
    for (int g = 0; g < G; ++g) {
        const double dpsi = cand[3 * g], f = cand[3 * g + 1], t0 = cand[3 * g + 2];
        MHT_REQUIRE(trial_finite_or_nan(dpsi) && trial_finite_or_nan(f) && trial_finite_or_nan(t0) && !(fabs(dpsi) > 3.14159265358979323846) &&
                        !(f < 0.0) && !(t0 < 0.0),
                    "mht_trial_manoeuvres: candidate %d (dpsi %g, f %g, t0 %g): |dpsi| <= pi, f >= 0, t0 >= 0, finite or NaN", g, dpsi, f, t0);
    }
    MHT_REQUIRE(work_bytes >= mht_trial_work_bytes(n, G, K), "mht_trial_manoeuvres: the work buffer holds %zu bytes, %zu are needed", work_bytes,
                mht_trial_work_bytes(n, G, K));
    o.p0[0] = own[0];
    o.p0[1] = own[1];
    o.v0[0] = own[2];
    o.v0[1] = own[3];
    for (int c = 0; c < 3; ++c) o.S[c] = Sown[c];
    o.w = w;
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    // (the candidates come from pageable host memory: the copy has left the caller's array when this returns)
    MHT_HIP_CHECK(hipMemcpyAsync((double*)work + trial_layout(n, G, K).cand, cand, (size_t)3 * (size_t)G * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const int rc = nx == 4 ? trial_run<4>(ctx, n, G, K, dt, R, Phi, Q, x, P, o, out, summary, (double*)work)
                           : trial_run<6>(ctx, n, G, K, dt, R, Phi, Q, x, P, o, out, summary, (double*)work);
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
