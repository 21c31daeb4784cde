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
static int run_em(mht_ctx* ctx, const mht_model_x* model, const SmoothBatch& b, int32_t n_iter, double* Q_out, double* R_out, double* ll_trace,
                  KernelSlot slot) {
    constexpr int NS = N * (N + 1) / 2;
    SmoothEmArgs<N> a = {};
    char* q = smooth_args<N>(linear_steps<N>(model), b, a.s);
    a.theta = reinterpret_cast<double*>(q); q += (size_t)(N + 2 * NS + 3) * (size_t)b.n * 8;
    a.sq = reinterpret_cast<double*>(q); q += (size_t)(NS + 4) * (size_t)b.n * 8;
    a.pn = reinterpret_cast<double*>(q);      // [NS + N][n]: with it the workspace holds smooth_em_track_doubles(N) per track
    a.Q_out = Q_out; a.R_out = R_out;
    int rc = queue_lengths(ctx, b);
    if (rc != MHT_OK) return rc;
    for (int32_t it = 0; it <= n_iter && rc == MHT_OK; ++it) {
        if (ll_trace) rc = score_linear_launch(ctx, model, b, it == 0 ? nullptr : a.theta, ll_trace + (size_t)it * (size_t)b.n);
        if (rc == MHT_OK)
            rc = launch_kernel(ctx, slot, it == n_iter ? smooth_em_kernel<N, true> : smooth_em_kernel<N, false>, dim3((b.n + 63) / 64), dim3(64), 0,
                               false, a, it == 0 ? 1 : 0);
    }
    return wait_and_return(ctx, rc);      // (the walks already queued read and write the caller's arrays)
}

// Both EM seams: the linear model's checks and n_iter's; an empty batch is done; the workspace is checked in front of the batch's arrays
static int run_em_seam(const char* seam, mht_ctx* ctx, const mht_model_x* model, const SmoothBatch& b, int32_t n_iter, double* Q_out, double* R_out,
                       double* ll_trace) {
    int rc = check_linear(seam, ctx, model, b.n, b.L_max);
    if (rc != MHT_OK) return rc;
    MHT_REQUIRE(n_iter >= 0 && n_iter <= SMOOTH_EM_MAX_ITER, "%s: n_iter must be 0 .. %d (got %d)", seam, SMOOTH_EM_MAX_ITER, n_iter);
    if (b.n == 0) return MHT_OK;
    rc = check_workspace(seam, b, smooth_em_work_bytes(model->nx, b.n, b.L_max), "mht_smooth_em_work_bytes", MHT_E_INVALID);
    if (rc != MHT_OK) return rc;
    MHT_REQUIRE(b.len && b.x_init && b.P_init && b.z && b.has_z && Q_out && R_out && b.xs && b.work, "%s: null array", seam);
    rc = check_lengths(seam, b);
    if (rc != MHT_OK) return rc;
    return model->nx == 4 ? run_em<4>(ctx, model, b, n_iter, Q_out, R_out, ll_trace, K_SMOOTH_EM4)
                          : run_em<6>(ctx, model, b, n_iter, Q_out, R_out, ll_trace, K_SMOOTH_EM6);
}

extern "C" int mht_smooth_tracks_em(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                    const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_iter,
                                    double* xs, double* Ps, double* Q_out, double* R_out, void* work, size_t work_bytes) {
    const SmoothBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, xs, Ps};
    return run_em_seam("mht_smooth_tracks_em", ctx, model, b, n_iter, Q_out, R_out, nullptr);
}

extern "C" int mht_smooth_tracks_em_ll(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                       const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_iter,
                                       double* xs, double* Ps, double* Q_out, double* R_out, void* work, size_t work_bytes, double* ll_trace) {
    MHT_REQUIRE(ll_trace || n_tracks == 0, "mht_smooth_tracks_em_ll: null ll_trace (mht_smooth_tracks_em is the call without one)");
    const SmoothBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, xs, Ps};
    return run_em_seam("mht_smooth_tracks_em_ll", ctx, model, b, n_iter, Q_out, R_out, ll_trace);
}
