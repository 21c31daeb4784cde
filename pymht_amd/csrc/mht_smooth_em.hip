// mht_smooth_tracks_em (include/mht_amd.h): the linear smoother of mht_smooth.hip with Q, R and the initial state re-estimated per track by
// expectation-maximisation before the smoothing walk, opt-in (em=5 in the Python API): what the reference's pykalman call does.  One
// track per lane and track-minor memory as there.  The same lane walks its track n_iter + 1 times, one launch per walk
// (mht_smooth_em.h says why, and what lives in registers and what in the workspace); Q and R are per lane, A and C stay wave-uniform.
// Its workspace is the linear smoother's plus theta, the sums and one parked state per track.
//
// mht_smooth_tracks_em_ll is the same call with the log-likelihood of every track under every theta_i handed out: one forward-only score
// launch (mht_smooth_score.hip, score_linear_launch) in front of each walk, on the same stream; smooth_em_kernel does not know of it.
#include "mht_common.h"
#include "mht_smooth_em.h"
#include "mht_smooth_seam.h"

namespace mht {

template <int N, bool LAST>
__global__ void __launch_bounds__(64) smooth_em_kernel(const SmoothEmArgs<N> a, const int first) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < a.s.n) smooth_em_pass<N, LAST>(a, t, first != 0);
}

static size_t smooth_em_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max) {      // + theta, sq and pn of mht_smooth_em.h
    return smooth_work_bytes(nx, 1, n_tracks, L_max) + (size_t)smooth_em_track_doubles(nx) * (size_t)n_tracks * 8;
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_smooth_em_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max) {
    if ((nx != 4 && nx != 6) || n_tracks < 0 || L_max < 0) return 0;
    return smooth_em_work_bytes(nx, n_tracks, L_max);
}

// n_iter + 1 launches of one walk each on the stream (mht_smooth_em.h says why not one), then a wait.  ll_trace [n_iter + 1][n], if
// asked for: in front of walk i, which runs under theta_i, one score launch under the same theta writes row i -- the call's arguments
// for the first, the workspace's theta behind it.
template <int N>
static int run_em(mht_ctx* ctx, const char* seam, const mht_model_x* model, const SmoothBatch& b, int32_t n_iter, double* Q_out, double* R_out,
                  double* ll_trace, KernelSlot slot) {
    constexpr int NS = N * (N + 1) / 2;
    if (b.n == 0) return MHT_OK;
    const int rc = check_batch(seam, "mht_smooth_em_work_bytes", N, 1, b, Q_out && R_out);
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    LinearSteps<N> steps = {};
    widen<N>(model, steps.model, steps.model.A);
    SmoothEmArgs<N> a = {};
    char* q = smooth_args<N>(steps, b, a.s);
    a.theta = reinterpret_cast<double*>(q); q += (size_t)(N + 2 * NS + 3) * (size_t)b.n * 8;
    a.sq = reinterpret_cast<double*>(q); q += (size_t)(NS + 4) * (size_t)b.n * 8;
    a.pn = reinterpret_cast<double*>(q);      // [NS + N][n]: with it the workspace holds smooth_em_track_doubles(N) per track
    a.Q_out = Q_out; a.R_out = R_out;
    MHT_HIP_CHECK(hipMemcpyAsync(b.work, b.len, (size_t)b.n * 4, hipMemcpyHostToDevice, ctx->stream));
    for (int32_t it = 0; it <= n_iter; ++it) {
        int lrc = ll_trace ? score_linear_launch(ctx, model, b, it == 0 ? nullptr : a.theta, ll_trace + (size_t)it * (size_t)b.n) : MHT_OK;
        if (lrc == MHT_OK)
            lrc = launch_kernel(ctx, slot, it == n_iter ? smooth_em_kernel<N, true> : smooth_em_kernel<N, false>, dim3((b.n + 63) / 64), dim3(64), 0,
                                false, a, it == 0 ? 1 : 0);
        if (lrc != MHT_OK) {      // (the walks already queued read and write the caller's arrays: they are waited for before the error goes back)
            (void)hipStreamSynchronize(ctx->stream);
            return lrc;
        }
    }
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}

// The checks of both EM seams in front of the batch's own
static int run_em_seam(const char* seam, mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                       const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_iter, double* xs, double* Ps,
                       double* Q_out, double* R_out, double* ll_trace, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "%s: null argument", seam);
    MHT_REQUIRE(model->nx == 4 || model->nx == 6, "%s: nx must be 4 or 6 (got %d)", seam, model->nx);
    MHT_REQUIRE(model->transition == 0, "%s: a state-dependent transition (%d) has no linear smoother to learn under", seam, model->transition);
    MHT_REQUIRE(model->A && model->Q && model->C && model->R, "%s: null model matrix", seam);
    MHT_REQUIRE(n_iter >= 0 && n_iter <= SMOOTH_EM_MAX_ITER, "%s: n_iter must be 0 .. %d (got %d)", seam, SMOOTH_EM_MAX_ITER, n_iter);
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "%s: bad size (n_tracks %d, L_max %d)", seam, n_tracks, L_max);
    const size_t need = smooth_em_work_bytes(model->nx, n_tracks, L_max);
    MHT_REQUIRE(n_tracks == 0 || work_bytes >= need, "%s: the workspace has %zu bytes, %zu are needed (mht_smooth_em_work_bytes)", seam, work_bytes, need);
    const SmoothBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, xs, Ps, work, work_bytes};
    return model->nx == 4 ? run_em<4>(ctx, seam, model, b, n_iter, Q_out, R_out, ll_trace, K_SMOOTH_EM4)
                          : run_em<6>(ctx, seam, model, b, n_iter, Q_out, R_out, ll_trace, K_SMOOTH_EM6);
}

extern "C" int mht_smooth_tracks_em(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                    const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_iter,
                                    double* xs, double* Ps, double* Q_out, double* R_out, void* work, size_t work_bytes) {
    return run_em_seam("mht_smooth_tracks_em", ctx, model, n_tracks, L_max, len, x_init, P_init, z, has_z, n_iter, xs, Ps, Q_out, R_out, nullptr, work,
                       work_bytes);
}

extern "C" int mht_smooth_tracks_em_ll(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                       const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_iter,
                                       double* xs, double* Ps, double* Q_out, double* R_out, void* work, size_t work_bytes, double* ll_trace) {
    MHT_REQUIRE(ll_trace || n_tracks == 0, "mht_smooth_tracks_em_ll: null ll_trace (mht_smooth_tracks_em is the call without one)");
    return run_em_seam("mht_smooth_tracks_em_ll", ctx, model, n_tracks, L_max, len, x_init, P_init, z, has_z, n_iter, xs, Ps, Q_out, R_out, ll_trace,
                       work, work_bytes);
}
