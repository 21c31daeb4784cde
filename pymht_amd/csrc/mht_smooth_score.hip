// mht_score_tracks, mht_score_tracks_ct, mht_score_tracks_ais (include/mht_amd.h): how well the smoothers' models explain a batch of
// track histories -- per track the log-likelihood, the normalised innovation squared summed over its plots, and their number.  The
// forward-only sibling of mht_smooth.hip: one walk (smooth_score_walk, mht_smooth_score.h) with that unit's step policies, ONE TRACK PER
// LANE, everything in memory track-minor, no lane touching anything of another -- a track's figures do not depend on where in the batch
// it sits.  Nothing is kept per node: no filtered slot, no xs, no Ps; the workspace holds the lengths and nothing else, and a lane
// writes three to five numbers at the end of its walk.  Without a backward step nothing but (x, P), one prediction and one gain is
// live at a time: the kernels sit far below the smoothers' registers (tests/test_smooth_score_resources.py), no LDS, no scratch.
//
// A further instance per state count reads x0, P0, Q and R PER TRACK from the EM workspace's theta (mht_smooth_em.h): the launch
// mht_smooth_tracks_em_ll (mht_smooth_em.hip) puts in front of each of its walks for the trace of log-likelihoods (score_linear_launch).
#include "mht_common.h"
#include "mht_smooth_score.h"
#include "mht_smooth_seam.h"

namespace mht {

template <int N, typename Steps>
__global__ void __launch_bounds__(64) smooth_score_kernel(const ScoreArgs<N, Steps> a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < a.n) smooth_score_walk<N>(a, t);
}

template <int N>
__global__ void __launch_bounds__(64) smooth_score_theta_kernel(const ScoreArgs<N, LinearSteps<N>> a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < a.n) smooth_score_walk_theta<N>(a, t);
}

static size_t score_work_bytes(int32_t n_tracks) { return smooth_len_bytes(n_tracks); }      // the lengths

struct ScoreBatch {      // what every score seam is handed besides its model
    int32_t n, L_max;
    const int32_t* len;
    const double *x_init, *P_init, *z;
    const uint8_t* has_z;
    double *ll, *nis;
    int32_t* nobs;
    void* work;
    size_t work_bytes;
};

template <int N, typename Steps>
static void score_args(const Steps& steps, const ScoreBatch& b, ScoreArgs<N, Steps>& a) {
    a = {};
    a.steps = steps;
    a.n = b.n; a.L_max = b.L_max;
    a.len = static_cast<const int32_t*>(b.work);
    a.x_init = b.x_init; a.P_init = b.P_init; a.z = b.z; a.has_z = b.has_z;
    a.ll = b.ll; a.nis = b.nis; a.nobs = b.nobs;
}

// An empty batch is done; any other is checked, then the lengths go to the workspace; then one launch and a wait
template <int N, typename Steps>
static int run_score(mht_ctx* ctx, const char* seam, const Steps& steps, bool extras, const ScoreBatch& b, double* nis_ais, int32_t* nais) {
    if (b.n == 0) return MHT_OK;
    MHT_REQUIRE(b.len && b.x_init && b.P_init && b.z && b.has_z && extras && b.ll && b.nis && b.nobs && b.work, "%s: null array", seam);
    for (int32_t t = 0; t < b.n; ++t)
        MHT_REQUIRE(b.len[t] >= 1 && b.len[t] <= b.L_max, "%s: track %d has length %d (1 .. L_max = %d)", seam, t, b.len[t], b.L_max);
    MHT_REQUIRE(b.work_bytes >= score_work_bytes(b.n), "%s: the workspace has %zu bytes, %zu are needed (mht_score_work_bytes)", seam, b.work_bytes,
                score_work_bytes(b.n));
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    ScoreArgs<N, Steps> a;
    score_args<N>(steps, b, a);
    a.nis_ais = nis_ais; a.nais = nais;
    MHT_HIP_CHECK(hipMemcpyAsync(b.work, b.len, (size_t)b.n * 4, hipMemcpyHostToDevice, ctx->stream));
    const int rc = launch_kernel(ctx, K_SMOOTH_SCORE, smooth_score_kernel<N, Steps>, dim3((b.n + 63) / 64), dim3(64), 0, false, a);
    if (rc != MHT_OK) {      // (the copy of the lengths reads the caller's array: it is waited for before the error goes back)
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}

template <int N>
static int run_score_linear(mht_ctx* ctx, const mht_model_x* model, const ScoreBatch& b) {
    LinearSteps<N> steps = {};
    widen<N>(model, steps.model, steps.model.A);
    return run_score<N>(ctx, "mht_score_tracks", steps, true, b, nullptr, nullptr);
}

template <int N>
static int em_score_launch(mht_ctx* ctx, const mht_model_x* model, const SmoothBatch& b, const double* theta, double* ll) {
    LinearSteps<N> steps = {};
    widen<N>(model, steps.model, steps.model.A);
    ScoreArgs<N, LinearSteps<N>> a;
    score_args<N>(steps, ScoreBatch{b.n, b.L_max, b.len, b.x_init, b.P_init, b.z, b.has_z, ll, nullptr, nullptr, b.work, b.work_bytes}, a);
    a.theta = theta;
    return launch_kernel(ctx, K_SMOOTH_SCORE, theta ? smooth_score_theta_kernel<N> : smooth_score_kernel<N, LinearSteps<N>>, dim3((b.n + 63) / 64),
                         dim3(64), 0, false, a);
}

int score_linear_launch(mht_ctx* ctx, const mht_model_x* model, const SmoothBatch& b, const double* theta, double* ll) {
    return model->nx == 4 ? em_score_launch<4>(ctx, model, b, theta, ll) : em_score_launch<6>(ctx, model, b, theta, ll);
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_score_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max) {
    if ((nx != 4 && nx != 6) || n_tracks < 0 || L_max < 0) return 0;
    return score_work_bytes(n_tracks);
}

extern "C" int mht_score_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                                const double* P_init, const double* z, const uint8_t* has_z, double* ll_out, double* nis_out, int32_t* nobs_out,
                                void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_score_tracks: null argument");
    MHT_REQUIRE(model->nx == 4 || model->nx == 6, "mht_score_tracks: nx must be 4 or 6 (got %d)", model->nx);
    MHT_REQUIRE(model->transition == 0, "mht_score_tracks: a state-dependent transition (%d) has no linear filter to score", model->transition);
    MHT_REQUIRE(model->A && model->Q && model->C && model->R, "mht_score_tracks: null model matrix");
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "mht_score_tracks: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    const ScoreBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, ll_out, nis_out, nobs_out, work, work_bytes};
    return model->nx == 4 ? run_score_linear<4>(ctx, model, b) : run_score_linear<6>(ctx, model, b);
}

extern "C" int mht_score_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                                   const double* P_init, const double* z, const uint8_t* has_z, double* ll_out, double* nis_out,
                                   int32_t* nobs_out, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_score_tracks_ct: null argument");
    MHT_REQUIRE(model->nx == 6, "mht_score_tracks_ct: the constant-turn model has 6 states (got nx = %d)", model->nx);
    MHT_REQUIRE(model->transition == 1, "mht_score_tracks_ct: transition must be 1 (got %d; a linear model belongs to mht_score_tracks)", model->transition);
    MHT_REQUIRE(model->Q && model->C && model->R, "mht_score_tracks_ct: null model matrix");
    MHT_REQUIRE(model->period > 0.0, "mht_score_tracks_ct: the model's period must be positive (got %g)", model->period);
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "mht_score_tracks_ct: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    ConstantTurnSteps steps = {};
    widen<6>(model, steps.model);
    steps.model.T = model->period;
    const ScoreBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, ll_out, nis_out, nobs_out, work, work_bytes};
    return run_score<6>(ctx, "mht_score_tracks_ct", steps, true, b, nullptr, nullptr);
}

extern "C" int mht_score_tracks_ais(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                    const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                                    const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, int32_t n_legs,
                                    double* ll_out, double* nis_out, int32_t* nobs_out, double* nis_ais_out, int32_t* nais_out, void* work,
                                    size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_score_tracks_ais: null argument");
    MHT_REQUIRE(model->nx == 4, "mht_score_tracks_ais: AIS messages report four states (got nx = %d)", model->nx);
    MHT_REQUIRE(model->transition == 0, "mht_score_tracks_ais: a state-dependent transition (%d) has no AIS-aware filter to score", model->transition);
    MHT_REQUIRE(model->A && model->Q && model->C && model->R, "mht_score_tracks_ais: null model matrix");
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1 && n_legs >= 0, "mht_score_tracks_ais: bad size (n_tracks %d, L_max %d, n_legs %d)", n_tracks, L_max, n_legs);
    AisSteps steps = {};
    widen<4>(model, steps.model, steps.model.A);
    steps.kind = kind; steps.ais_z = ais_z; steps.ais_r = ais_r; steps.leg = leg; steps.legs = legs;
    const ScoreBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, ll_out, nis_out, nobs_out, work, work_bytes};
    return run_score<4>(ctx, "mht_score_tracks_ais", steps, kind && ais_z && ais_r && leg && (legs || n_legs == 0) && nis_ais_out && nais_out, b,
                        nis_ais_out, nais_out);
}
