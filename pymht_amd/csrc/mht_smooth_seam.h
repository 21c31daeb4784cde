// Host side shared by the seams over a batch of track histories (mht_smooth.hip, mht_smooth_em.hip, mht_smooth_score.hip,
// mht_smooth_score_grid.hip, mht_smooth_trace.hip, mht_smooth_filter.hip, mht_imm.hip, mht_imm_smooth.hip): the batch every seam is
// handed, the checks of its model and of the batch, the step policy made of an mht_model_x, the smoothers' workspace, and the tail every
// seam ends in -- the lengths to the workspace's front, one launch, a wait.
#pragma once
#include "mht_common.h"
#include "mht_smooth_walk.h"

namespace mht {

struct TrackBatch {      // what every seam is handed besides its model; a unit's own batch derives from it and adds its outputs
    int32_t n, L_max;
    const int32_t* len;
    const double *x_init, *P_init, *z;
    const uint8_t* has_z;
    void* work;
    size_t work_bytes;
};

struct SmoothBatch : TrackBatch {
    double *xs, *Ps;
};

// ---- the model, checked per kind: a null ctx or model first, then nx, transition, the matrices, the sizes; MHT_E_INVALID each

static int check_linear(const char* seam, const mht_ctx* ctx, const mht_model_x* m, int32_t n_tracks, int32_t L_max) {
    MHT_REQUIRE(ctx && m, "%s: null argument", seam);
    MHT_REQUIRE(m->nx == 4 || m->nx == 6, "%s: nx must be 4 or 6 (got %d)", seam, m->nx);
    MHT_REQUIRE(m->transition == 0, "%s: a state-dependent transition (%d) is no linear model", seam, m->transition);
    MHT_REQUIRE(m->A && m->Q && m->C && m->R, "%s: null model matrix", seam);
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "%s: bad size (n_tracks %d, L_max %d)", seam, n_tracks, L_max);
    return MHT_OK;
}

static int check_ct(const char* seam, const mht_ctx* ctx, const mht_model_x* m, int32_t n_tracks, int32_t L_max) {
    MHT_REQUIRE(ctx && m, "%s: null argument", seam);
    MHT_REQUIRE(m->nx == 6, "%s: the constant-turn model has 6 states (got nx = %d)", seam, m->nx);
    MHT_REQUIRE(m->transition == 1, "%s: transition must be 1 (got %d; a linear model belongs to the seam without _ct)", seam, m->transition);
    MHT_REQUIRE(m->Q && m->C && m->R, "%s: null model matrix", seam);
    MHT_REQUIRE(m->period > 0.0, "%s: the model's period must be positive (got %g)", seam, m->period);
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "%s: bad size (n_tracks %d, L_max %d)", seam, n_tracks, L_max);
    return MHT_OK;
}

static int check_ais(const char* seam, const mht_ctx* ctx, const mht_model_x* m, int32_t n_tracks, int32_t L_max, int32_t n_legs) {
    MHT_REQUIRE(ctx && m, "%s: null argument", seam);
    MHT_REQUIRE(m->nx == 4, "%s: AIS messages report four states (got nx = %d)", seam, m->nx);
    MHT_REQUIRE(m->transition == 0, "%s: a state-dependent transition (%d) is no AIS-aware model", seam, m->transition);
    MHT_REQUIRE(m->A && m->Q && m->C && m->R, "%s: null model matrix", seam);
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1 && n_legs >= 0, "%s: bad size (n_tracks %d, L_max %d, n_legs %d)", seam, n_tracks, L_max, n_legs);
    return MHT_OK;
}

// ---- the step policy of a checked model

// mht_model_x's float32 matrices in float64 (exact): Q, C, R, and A where the model has one
template <int N, typename Model>
static void widen(const mht_model_x* m, Model& out, double* A = nullptr) {
    if (A)
        for (int i = 0; i < N * N; ++i) A[i] = (double)m->A[i];
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j) out.Q[sym_idx(N, i, j)] = (double)m->Q[i * N + j];
    for (int i = 0; i < 2 * N; ++i) out.C[i] = (double)m->C[i];
    out.R[0] = (double)m->R[0]; out.R[1] = (double)m->R[1]; out.R[2] = (double)m->R[3];
}

template <int N>
static LinearSteps<N> linear_steps(const mht_model_x* m) {
    LinearSteps<N> steps = {};
    widen<N>(m, steps.model, steps.model.A);
    return steps;
}

static ConstantTurnSteps ct_steps(const mht_model_x* m) {
    ConstantTurnSteps steps = {};
    widen<6>(m, steps.model);
    steps.model.T = m->period;
    return steps;
}

// *complete: none of the per-node arrays is missing, nor the leg table where it has entries
static AisSteps ais_steps(const mht_model_x* m, const uint8_t* kind, const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs,
                          int32_t n_legs, bool* complete) {
    AisSteps steps = {};
    widen<4>(m, steps.model, steps.model.A);
    steps.kind = kind; steps.ais_z = ais_z; steps.ais_r = ais_r; steps.leg = leg; steps.legs = legs;
    *complete = kind && ais_z && ais_r && leg && (legs || n_legs == 0);
    return steps;
}

// ---- a non-empty batch, checked behind its model; nothing has been launched or written where one of these fails

static int check_lengths(const char* seam, const TrackBatch& b) {
    for (int32_t t = 0; t < b.n; ++t)
        MHT_REQUIRE(b.len[t] >= 1 && b.len[t] <= b.L_max, "%s: track %d has length %d (1 .. L_max = %d)", seam, t, b.len[t], b.L_max);
    return MHT_OK;
}

// short_code: what the seam documents for a workspace that is too small -- MHT_E_CAPACITY for mht_smooth_tracks*, MHT_E_INVALID for the rest
static int check_workspace(const char* seam, const TrackBatch& b, size_t need, const char* sizer, int short_code) {
    if (b.work_bytes >= need) return MHT_OK;
    set_error("%s: the workspace has %zu bytes, %zu are needed (%s)", seam, b.work_bytes, need, sizer);
    return short_code;
}

// The three in the order most seams make them; own_arrays: none of the arrays the unit takes next to the batch's is missing
static int check_batch(const char* seam, const TrackBatch& b, bool own_arrays, size_t need, const char* sizer, int short_code) {
    MHT_REQUIRE(b.len && b.x_init && b.P_init && b.z && b.has_z && own_arrays && b.work, "%s: null array", seam);
    const int rc = check_lengths(seam, b);
    return rc != MHT_OK ? rc : check_workspace(seam, b, need, sizer, short_code);
}

// ---- the tail

// The lengths to the workspace's front, queued on the context's stream.  The copy reads the caller's host array: whatever fails behind
// it, the stream is waited for before the error goes back (wait_and_return)
static int queue_lengths(mht_ctx* ctx, const TrackBatch& b) {
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    MHT_HIP_CHECK(hipMemcpyAsync(b.work, b.len, (size_t)b.n * 4, hipMemcpyHostToDevice, ctx->stream));
    return MHT_OK;
}

static int wait_and_return(mht_ctx* ctx, int rc) {
    if (rc != MHT_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}

static size_t smooth_len_bytes(int32_t n_tracks) { return (((size_t)n_tracks * 4 + 255) / 256) * 256; }

// A checked batch, run: the lengths, then `table` (host, or null: the IMM's modes, the grid's candidates) behind them in the workspace,
// then launch() -- launch_kernel's return --, then the wait
template <typename Launch>
static int run_over_lengths(mht_ctx* ctx, const char* seam, const TrackBatch& b, const double* table, size_t table_doubles, Launch launch) {
    int rc = queue_lengths(ctx, b);
    if (rc != MHT_OK) return rc;
    if (table) {
        const hipError_t e = hipMemcpyAsync(static_cast<char*>(b.work) + smooth_len_bytes(b.n), table, table_doubles * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            set_error("%s: copying to the workspace: %s", seam, hipGetErrorString(e));
            rc = MHT_E_HIP;
        }
    }
    return wait_and_return(ctx, rc == MHT_OK ? launch() : rc);
}

// ---- the smoothers' workspace: the lengths, then the filtered slots of every node

static size_t smooth_work_bytes(int32_t nx, int32_t slots, int32_t n_tracks, int32_t L_max) {
    return smooth_len_bytes(n_tracks) + (size_t)L_max * (size_t)slots * (size_t)(nx + nx * (nx + 1) / 2) * (size_t)n_tracks * 8;
}

// The arguments of a walk over a checked batch: the lengths at the front of the workspace, the filtered means and covariances behind
// them; returns the first byte behind those
template <int N, typename Steps>
static char* smooth_args(const Steps& steps, const SmoothBatch& b, SmoothArgs<N, Steps>& a) {
    a = {};
    a.steps = steps;
    a.n = b.n; a.L_max = b.L_max;
    a.x_init = b.x_init; a.P_init = b.P_init; a.z = b.z; a.has_z = b.has_z; a.xs = b.xs; a.Ps = b.Ps;
    char* q = static_cast<char*>(b.work);
    a.len = reinterpret_cast<const int32_t*>(q); q += smooth_len_bytes(b.n);
    a.xf = reinterpret_cast<double*>(q); q += (size_t)b.L_max * Steps::SLOTS * N * (size_t)b.n * 8;
    a.Pf = reinterpret_cast<double*>(q); q += (size_t)b.L_max * Steps::SLOTS * (N * (N + 1) / 2) * (size_t)b.n * 8;
    return q;
}

// One forward-only score launch over a checked linear batch whose lengths are in the workspace (mht_smooth_score.hip), queued on the
// context's stream and not waited for: ll [n] <- each track's log-likelihood under the call's (x_init, P_init, Q, R) (theta null) or
// under its own theta [N + 2 NS + 3][n] in the EM workspace's layout.  What mht_smooth_tracks_em_ll puts in front of each EM walk.
int score_linear_launch(mht_ctx* ctx, const mht_model_x* model, const TrackBatch& b, const double* theta, double* ll);

}  // namespace mht
