// mht_score_tracks, mht_score_tracks_ct, mht_score_tracks_ais (include/mht_amd.h): how well the smoothers' models explain a batch of
// track histories -- per track the log-likelihood, the normalised innovation squared summed over its plots, and their number.  The
// forward half of mht_smooth.hip: one walk (smooth_score_walk, mht_smooth_score.h) with that unit's step policies, lanes and layout; the
// host path is mht_smooth_seam.h's.  Nothing is kept per node: no filtered slot, no xs, no Ps; the workspace holds the lengths and
// nothing else, and a lane writes three to five numbers at the end of its walk.  Without a backward step nothing but (x, P), one prediction and one gain is
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

struct ScoreBatch : TrackBatch {
    double *ll, *nis;
    int32_t* nobs;
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
    const int rc = check_batch(seam, b, extras && b.ll && b.nis && b.nobs, score_work_bytes(b.n), "mht_score_work_bytes", MHT_E_INVALID);
    if (rc != MHT_OK) return rc;
    ScoreArgs<N, Steps> a;
    score_args<N>(steps, b, a);
    a.nis_ais = nis_ais; a.nais = nais;
    return run_over_lengths(ctx, seam, b, nullptr, 0, [&] {
        return launch_kernel(ctx, K_SMOOTH_SCORE, smooth_score_kernel<N, Steps>, dim3((b.n + 63) / 64), dim3(64), 0, false, a);
    });
}

template <int N>
static int em_score_launch(mht_ctx* ctx, const mht_model_x* model, const TrackBatch& b, const double* theta, double* ll) {
    ScoreArgs<N, LinearSteps<N>> a;
    score_args<N>(linear_steps<N>(model), ScoreBatch{b, ll, nullptr, nullptr}, a);
    a.theta = theta;
    return launch_kernel(ctx, K_SMOOTH_SCORE, theta ? smooth_score_theta_kernel<N> : smooth_score_kernel<N, LinearSteps<N>>, dim3((b.n + 63) / 64),
                         dim3(64), 0, false, a);
}

int score_linear_launch(mht_ctx* ctx, const mht_model_x* model, const TrackBatch& b, const double* theta, double* ll) {
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
    const char* seam = "mht_score_tracks";
    const int rc = check_linear(seam, ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const ScoreBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, ll_out, nis_out, nobs_out};
    return model->nx == 4 ? run_score<4>(ctx, seam, linear_steps<4>(model), true, b, nullptr, nullptr)
                          : run_score<6>(ctx, seam, linear_steps<6>(model), true, b, nullptr, nullptr);
}

extern "C" int mht_score_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                                   const double* P_init, const double* z, const uint8_t* has_z, double* ll_out, double* nis_out,
                                   int32_t* nobs_out, void* work, size_t work_bytes) {
    const int rc = check_ct("mht_score_tracks_ct", ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const ScoreBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, ll_out, nis_out, nobs_out};
    return run_score<6>(ctx, "mht_score_tracks_ct", ct_steps(model), true, b, nullptr, nullptr);
}

extern "C" int mht_score_tracks_ais(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                    const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                                    const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, int32_t n_legs,
                                    double* ll_out, double* nis_out, int32_t* nobs_out, double* nis_ais_out, int32_t* nais_out, void* work,
                                    size_t work_bytes) {
    const int rc = check_ais("mht_score_tracks_ais", ctx, model, n_tracks, L_max, n_legs);
    if (rc != MHT_OK) return rc;
    bool extras;
    const AisSteps steps = ais_steps(model, kind, ais_z, ais_r, leg, legs, n_legs, &extras);
    const ScoreBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, ll_out, nis_out, nobs_out};
    return run_score<4>(ctx, "mht_score_tracks_ais", steps, extras && nis_ais_out && nais_out, b, nis_ais_out, nais_out);
}
