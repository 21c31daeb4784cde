// mht_trial_hypotheses (include/mht_amd.h): G candidate manoeuvres of the own ship against the L leaves of the forest -- every live
// hypothesis of every target -- folded per (candidate, target) (the figures, the weights and the order of the sums: mht_trial_hyp.h;
// the manoeuvre: mht_trial.h; the figures of a cell: mht_encounter.h).  The trajectories live in the work buffer as in mht_trial.hip,
// pos [K + 1][2][L + G] and S [K + 1][3][L + G], leaves first.  Five launches on the context's stream:
//
// hyp_weight_kernel: ONE TARGET PER LANE, serial over its leaves: cmin_t, w_l, weight_l and the leaf's target.  None of it depends on g.
//
// hyp_propagate_kernel<N>: ONE LEAF PER LANE through trial_track<N>.  The leaves are propagated once, whatever G is.
//
// hyp_candidate_kernel: ONE CANDIDATE PER LANE, trial_candidate.
//
// hyp_cell_kernel: ONE CELL (g, l) PER LANE, mht_trial.hip's tile: candidate g and 256 consecutive leaves, so that g is the same in
// every lane (the candidate's trajectory through wave-uniform loads, the leaves' through coalesced ones).  A lane stores its cell to the
// table if there is one, and to fig's Sel rows if its leaf is sel[t] (one writer).  It puts (pc, dcpa, w) into LDS, 6 KB; then the lanes
// that head a PIECE -- the part of a target inside the tile -- fold their piece serially in leaf order and store one partial at slot
// tile + target of partials [6][G][tiles + T].  No atomic: every partial has one writer.
//
// hyp_target_kernel: ONE (g, t) PER LANE, t fastest, folds the target's pieces in tile order, divides, and writes fig.
#include "mht_common.h"
#include "mht_trial_hyp.h"

namespace mht {

constexpr int HYP_THREADS = TRIAL_TILE;
constexpr int HYP_MAX_BLOCKS = 2048;

template <int N>
struct HypPropagateArgs {
    EncounterModel<N> m;
    int32_t L, nt, K;
    const double* x;      // [N][L]
    const double* P;      // [N(N+1)/2][L]
    double* xs;           // [N][nt], the staging
    double* Ps;           // [N(N+1)/2][nt]
    double* pos;          // [K + 1][2][nt]
    double* S;            // [K + 1][3][nt]
};

struct HypCandidateArgs {
    TrialOwn own;
    int32_t L, G, K;
    double dt;
    const double* cand;      // dev [G][3]
    double* pos;
    double* S;
};

struct HypWeightArgs {
    int32_t T;
    const double* cnllr;      // [L]
    const int32_t* seg;       // dev [T + 1]
    double* wl;               // [L]
    double* weight;           // [L]
    int32_t* target_of;       // [L]
};

struct HypCellArgs {
    int32_t L, T, G, K;
    double dt, R;
    const double* pos;
    const double* S;
    const double* wl;
    const int32_t* target_of;
    const int32_t* seg;
    const int32_t* sel;
    double* table;         // [5][G][L] or null
    double* fig;           // [8][G][T]
    double* partials;      // [6][G][tiles + T]
};

struct HypTargetArgs {
    int32_t T, G;
    size_t slots;      // tiles + T
    const double* partials;
    const int32_t* seg;
    const int32_t* sel;
    double* fig;
};

__global__ void __launch_bounds__(HYP_THREADS) hyp_weight_kernel(const HypWeightArgs a) {
    for (size_t t = (size_t)blockIdx.x * HYP_THREADS + threadIdx.x; t < (size_t)a.T; t += (size_t)gridDim.x * HYP_THREADS)
        hyp_weights(a.cnllr, a.seg, (int)t, a.wl, a.weight, a.target_of);
}

template <int N>
__global__ void __launch_bounds__(HYP_THREADS) hyp_propagate_kernel(const HypPropagateArgs<N> a) {
    for (size_t l = (size_t)blockIdx.x * HYP_THREADS + threadIdx.x; l < (size_t)a.L; l += (size_t)gridDim.x * HYP_THREADS)
        trial_track<N>(a.m, a.x, a.P, a.L, a.nt, a.K, (int)l, a.xs, a.Ps, a.pos, a.S);
}

__global__ void __launch_bounds__(HYP_THREADS) hyp_candidate_kernel(const HypCandidateArgs a) {
    for (size_t g = (size_t)blockIdx.x * HYP_THREADS + threadIdx.x; g < (size_t)a.G; g += (size_t)gridDim.x * HYP_THREADS) {
        const double* c = a.cand + 3 * g;
        trial_candidate(a.own, c[0], c[1], c[2], a.L + a.G, a.K, a.dt, a.L + (int)g, a.pos, a.S);
    }
}

__global__ void __launch_bounds__(HYP_THREADS) hyp_cell_kernel(const HypCellArgs a) {
    __shared__ double pc[HYP_THREADS], dcpa[HYP_THREADS], w[HYP_THREADS];
    const size_t chunks = ((size_t)a.L + TRIAL_TILE - 1) / TRIAL_TILE;
    const size_t tiles = (size_t)a.G * chunks;
    const size_t slots = chunks + (size_t)a.T;
    const int lane = threadIdx.x;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // (the same trips in every lane of the workgroup: the barriers)
        const int g = (int)(tile / chunks);
        const size_t chunk = tile % chunks;
        const int base = (int)(chunk * TRIAL_TILE);
        const size_t l = (size_t)base + lane;
        int t = -1;
        if (l < (size_t)a.L) {
            double o[ENCOUNTER_FIGURES];
            hyp_cell(a.pos, a.S, a.L, a.G, a.K, a.dt, a.R, g, (int)l, a.table, o);
            t = a.target_of[l];
            if (a.sel[t] == (int)l) hyp_store_selected(o, a.G, a.T, g, t, a.fig);
            pc[lane] = o[3];
            dcpa[lane] = o[1];
            w[lane] = a.wl[l];
        }
        __syncthreads();
        if (t >= 0 && (lane == 0 || a.target_of[l - 1] != t)) {      // the head of a piece
            const HypPart p = hyp_piece(pc, dcpa, w, base, lane, a.seg[t + 1]);
            hyp_store(p, a.partials + (size_t)g * slots + chunk + (size_t)t, (size_t)a.G * slots);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(HYP_THREADS) hyp_target_kernel(const HypTargetArgs a) {
    const size_t cells = (size_t)a.G * (size_t)a.T;
    for (size_t i = (size_t)blockIdx.x * HYP_THREADS + threadIdx.x; i < cells; i += (size_t)gridDim.x * HYP_THREADS)
        hyp_target(a.partials, a.seg, a.sel, a.G, a.T, a.slots, (int)(i / (size_t)a.T), (int)(i % (size_t)a.T), a.fig);
}

struct HypLayout {
    size_t pos, S, partials, xs, Ps, cand, wl, doubles;      // offsets in doubles, and their total
    size_t seg, sel, target_of, ints;                        // offsets in int32 behind the doubles, and their total
};

// The staging is sized for six states whatever nx is: the sizer does not take nx
static HypLayout hyp_layout(int32_t L, int32_t T, int32_t G, int32_t K) {
    const size_t nt = (size_t)L + (size_t)G, steps = (size_t)(K + 1), chunks = ((size_t)L + TRIAL_TILE - 1) / TRIAL_TILE;
    HypLayout l;
    l.pos = 0;
    l.S = l.pos + 2 * steps * nt;
    l.partials = l.S + 3 * steps * nt;
    l.xs = l.partials + (size_t)HYP_PARTIAL * (size_t)G * (chunks + (size_t)T);
    l.Ps = l.xs + 6 * nt;
    l.cand = l.Ps + 21 * nt;
    l.wl = l.cand + 3 * (size_t)G;
    l.doubles = l.wl + (size_t)L;
    l.seg = 0;
    l.sel = l.seg + (size_t)T + 1;
    l.target_of = l.sel + (size_t)T;
    l.ints = l.target_of + (size_t)L;
    return l;
}

static bool hyp_sizes_fit(int32_t L, int32_t T, int32_t G, int32_t K) {
    return L > 0 && T >= 1 && T <= L && G >= 1 && G <= TRIAL_MAX_CANDIDATES && K >= 1 && K <= ENCOUNTER_MAX_STEPS && L <= INT32_MAX - TRIAL_MAX_CANDIDATES;
}

static unsigned hyp_blocks(size_t items) {
    const size_t b = (items + HYP_THREADS - 1) / HYP_THREADS;
    return (unsigned)(b < (size_t)HYP_MAX_BLOCKS ? b : (size_t)HYP_MAX_BLOCKS);
}

template <int N>
static int hyp_run(mht_ctx* ctx, int32_t L, int32_t T, int32_t G, int32_t K, double dt, double R, const double* Phi, const double* Q, const double* x,
                   const double* P, const double* cnllr, const TrialOwn& own, double* table, double* fig, double* weight, double* work) {
    const HypLayout l = hyp_layout(L, T, G, K);
    int32_t* ints = (int32_t*)(work + l.doubles);
    const HypWeightArgs wa = {T, cnllr, ints + l.seg, work + l.wl, weight, ints + l.target_of};
    int rc = launch_kernel(ctx, K_SMOOTH_SCORE, hyp_weight_kernel, dim3(hyp_blocks((size_t)T)), dim3(HYP_THREADS), 0, false, wa);
    if (rc != MHT_OK) return rc;
    HypPropagateArgs<N> pa;
    for (int c = 0; c < N * N; ++c) {
        pa.m.Phi[c] = Phi[c];
        pa.m.Q[c] = Q[c];
    }
    pa.L = L;
    pa.nt = L + G;
    pa.K = K;
    pa.x = x;
    pa.P = P;
    pa.xs = work + l.xs;
    pa.Ps = work + l.Ps;
    pa.pos = work + l.pos;
    pa.S = work + l.S;
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, hyp_propagate_kernel<N>, dim3(hyp_blocks((size_t)L)), dim3(HYP_THREADS), 0, false, pa);
    if (rc != MHT_OK) return rc;
    const HypCandidateArgs ca = {own, L, G, K, dt, work + l.cand, pa.pos, pa.S};
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, hyp_candidate_kernel, dim3(hyp_blocks((size_t)G)), dim3(HYP_THREADS), 0, false, ca);
    if (rc != MHT_OK) return rc;
    const size_t chunks = ((size_t)L + TRIAL_TILE - 1) / TRIAL_TILE, tiles = (size_t)G * chunks;
    const HypCellArgs qa = {L, T, G, K, dt, R, pa.pos, pa.S, work + l.wl, ints + l.target_of, ints + l.seg, ints + l.sel, table, fig, work + l.partials};
    rc = launch_kernel(ctx, K_SMOOTH_SCORE, hyp_cell_kernel, dim3((unsigned)(tiles < (size_t)HYP_MAX_BLOCKS ? tiles : (size_t)HYP_MAX_BLOCKS)), dim3(HYP_THREADS), 0, false, qa);
    if (rc != MHT_OK) return rc;
    const HypTargetArgs ta = {T, G, chunks + (size_t)T, work + l.partials, ints + l.seg, ints + l.sel, fig};
    return launch_kernel(ctx, K_SMOOTH_SCORE, hyp_target_kernel, dim3(hyp_blocks((size_t)G * (size_t)T)), dim3(HYP_THREADS), 0, false, ta);
}

static bool hyp_finite(double v) { return v - v == 0.0; }
static bool hyp_finite_or_nan(double v) { return v != v || hyp_finite(v); }

}  // namespace mht

using namespace mht;

extern "C" size_t mht_trial_hyp_work_bytes(int32_t n_leaves, int32_t n_targets, int32_t G, int32_t K) {
    if (!hyp_sizes_fit(n_leaves, n_targets, G, K)) return 0;
    const HypLayout l = hyp_layout(n_leaves, n_targets, G, K);
    return (l.doubles * sizeof(double) + l.ints * sizeof(int32_t) + 255) / 256 * 256;
}

extern "C" int mht_trial_hypotheses(mht_ctx* ctx, int32_t nx, int32_t L, int32_t T, int32_t G, int32_t K, double dt, double R, const double* Phi,
                                    const double* Q, const double* x, const double* P, const double* cnllr, const int32_t* seg, const int32_t* sel,
                                    const double* own, const double* Sown, double w, const double* cand, double* table, double* fig, double* weight,
                                    void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx, "mht_trial_hypotheses: null context");
    MHT_REQUIRE(nx == 4 || nx == 6, "mht_trial_hypotheses: nx must be 4 or 6 (got %d)", nx);
    MHT_REQUIRE(K >= 1 && K <= ENCOUNTER_MAX_STEPS, "mht_trial_hypotheses: K must be 1 .. %d steps (got %d)", ENCOUNTER_MAX_STEPS, K);
    MHT_REQUIRE(G >= 1 && G <= TRIAL_MAX_CANDIDATES, "mht_trial_hypotheses: G must be 1 .. %d candidates (got %d)", TRIAL_MAX_CANDIDATES, G);
    MHT_REQUIRE(L >= 0 && L <= INT32_MAX - TRIAL_MAX_CANDIDATES, "mht_trial_hypotheses: bad number of leaves (%d)", L);
    MHT_REQUIRE(R > 0.0 && dt > 0.0 && w > 0.0 && hyp_finite(R) && hyp_finite(dt) && hyp_finite(w),
                "mht_trial_hypotheses: the radius, the step and the turn rate must be positive and finite (R %g, dt %g, w %g)", R, dt, w);
    if (L == 0) return MHT_OK;
    MHT_REQUIRE(T >= 1 && T <= L, "mht_trial_hypotheses: T must be 1 .. L = %d targets (got %d)", L, T);
    MHT_REQUIRE(Phi && Q && x && P && cnllr && seg && sel && own && Sown && cand && fig && weight && work, "mht_trial_hypotheses: null array");
    MHT_REQUIRE(seg[0] == 0 && seg[T] == L, "mht_trial_hypotheses: seg runs from 0 to L = %d (got %d .. %d)", L, seg[0], seg[T]);
    for (int t = 0; t < T; ++t) {
        MHT_REQUIRE(seg[t + 1] >= seg[t], "mht_trial_hypotheses: seg decreases at target %d (%d, then %d)", t, seg[t], seg[t + 1]);
        MHT_REQUIRE(sel[t] == -1 || (sel[t] >= seg[t] && sel[t] < seg[t + 1]), "mht_trial_hypotheses: sel[%d] = %d is neither -1 nor a leaf of %d .. %d", t, sel[t],
                    seg[t], seg[t + 1] - 1);
    }
    TrialOwn o;
    for (int c = 0; c < 4; ++c) MHT_REQUIRE(hyp_finite_or_nan(own[c]), "mht_trial_hypotheses: own[%d] is infinite", c);
    for (int c = 0; c < 3; ++c) MHT_REQUIRE(hyp_finite_or_nan(Sown[c]), "mht_trial_hypotheses: Sown[%d] is infinite", c);
    for (int g = 0; g < G; ++g) {
        const double dpsi = cand[3 * g], f = cand[3 * g + 1], t0 = cand[3 * g + 2];
        MHT_REQUIRE(hyp_finite_or_nan(dpsi) && hyp_finite_or_nan(f) && hyp_finite_or_nan(t0) && !(fabs(dpsi) > 3.14159265358979323846) && !(f < 0.0) &&
                        !(t0 < 0.0),
                    "mht_trial_hypotheses: candidate %d (dpsi %g, f %g, t0 %g): |dpsi| <= pi, f >= 0, t0 >= 0, finite or NaN", g, dpsi, f, t0);
    }
    MHT_REQUIRE(work_bytes >= mht_trial_hyp_work_bytes(L, T, G, K), "mht_trial_hypotheses: the work buffer holds %zu bytes, %zu are needed", work_bytes,
                mht_trial_hyp_work_bytes(L, T, G, K));
    o.p0[0] = own[0];
    o.p0[1] = own[1];
    o.v0[0] = own[2];
    o.v0[1] = own[3];
    for (int c = 0; c < 3; ++c) o.S[c] = Sown[c];
    o.w = w;
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    // (the small arrays come from pageable host memory: the copies have left the caller's arrays when this returns)
    const HypLayout l = hyp_layout(L, T, G, K);
    int32_t* ints = (int32_t*)((double*)work + l.doubles);
    MHT_HIP_CHECK(hipMemcpyAsync((double*)work + l.cand, cand, (size_t)3 * (size_t)G * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MHT_HIP_CHECK(hipMemcpyAsync(ints + l.seg, seg, ((size_t)T + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    MHT_HIP_CHECK(hipMemcpyAsync(ints + l.sel, sel, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const int rc = nx == 4 ? hyp_run<4>(ctx, L, T, G, K, dt, R, Phi, Q, x, P, cnllr, o, table, fig, weight, (double*)work)
                           : hyp_run<6>(ctx, L, T, G, K, dt, R, Phi, Q, x, P, cnllr, o, table, fig, weight, (double*)work);
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
