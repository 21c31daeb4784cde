// mht_trace_tracks, mht_trace_tracks_ct, mht_trace_tracks_ais (include/mht_amd.h): the per-node innovation sequence of a batch of track
// histories -- v_k, S_k, nis_k and ll_k at every node with a plot, and the same for every AIS message -- where mht_score_tracks*
// (mht_smooth_score.hip) hands out their sums.  One walk (smooth_trace_walk, mht_smooth_trace.h) with the smoothers' step policies; the
// lanes and the layout are mht_smooth.hip's, the host path mht_smooth_seam.h's.  The workspace holds the lengths and nothing
// else; the outputs are [node][element][track], so the 7 (16) stores a lane makes per node are contiguous over a wavefront, and a lane
// writes EVERY row of its track, NaN where there is nothing to say: the caller's memory need not be initialised.  Like the score
// kernels, nothing but (x, P), one prediction and one gain is live at a time, and the node's figures are stored in front of the gain:
// no LDS, no scratch (tests/test_smooth_trace_resources.py).
//
// A unit of its own: the score and grid units keep their kernels, and their compiled resources, as they are.
#include "mht_common.h"
#include "mht_smooth_trace.h"
#include "mht_smooth_seam.h"

namespace mht {

template <int N, typename Steps>
__global__ void __launch_bounds__(64) smooth_trace_kernel(const TraceArgs<N, Steps> a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < a.n) smooth_trace_walk<N>(a, t);
}

static size_t trace_work_bytes(int32_t n_tracks) { return smooth_len_bytes(n_tracks); }      // the lengths

struct TraceBatch : TrackBatch {
    double* radar;
};

// An empty batch is done; any other is checked, then the lengths go to the workspace; then one launch and a wait
template <int N, typename Steps>
static int run_trace(mht_ctx* ctx, const char* seam, const Steps& steps, bool extras, const TraceBatch& b, double* ais) {
    if (b.n == 0) return MHT_OK;
    const int rc = check_batch(seam, b, extras && b.radar, trace_work_bytes(b.n), "mht_trace_work_bytes", MHT_E_INVALID);
    if (rc != MHT_OK) return rc;
    TraceArgs<N, Steps> a = {};
    a.steps = steps;
    a.n = b.n; a.L_max = b.L_max;
    a.len = static_cast<const int32_t*>(b.work);
    a.x_init = b.x_init; a.P_init = b.P_init; a.z = b.z; a.has_z = b.has_z;
    a.radar = b.radar; a.ais = ais;
    return run_over_lengths(ctx, seam, b, nullptr, 0, [&] {
        return launch_kernel(ctx, K_SMOOTH_SCORE, smooth_trace_kernel<N, Steps>, dim3((b.n + 63) / 64), dim3(64), 0, false, a);
    });
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_trace_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max) {
    if ((nx != 4 && nx != 6) || n_tracks < 0 || L_max < 0) return 0;
    return trace_work_bytes(n_tracks);
}

extern "C" int mht_trace_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                                const double* P_init, const double* z, const uint8_t* has_z, double* radar_out, void* work, size_t work_bytes) {
    const char* seam = "mht_trace_tracks";
    const int rc = check_linear(seam, ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const TraceBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, radar_out};
    return model->nx == 4 ? run_trace<4>(ctx, seam, linear_steps<4>(model), true, b, nullptr)
                          : run_trace<6>(ctx, seam, linear_steps<6>(model), true, b, nullptr);
}

extern "C" int mht_trace_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                                   const double* P_init, const double* z, const uint8_t* has_z, double* radar_out, void* work, size_t work_bytes) {
    const int rc = check_ct("mht_trace_tracks_ct", ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const TraceBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, radar_out};
    return run_trace<6>(ctx, "mht_trace_tracks_ct", ct_steps(model), true, b, nullptr);
}

extern "C" int mht_trace_tracks_ais(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                    const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                                    const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, int32_t n_legs,
                                    double* radar_out, double* ais_out, void* work, size_t work_bytes) {
    const int rc = check_ais("mht_trace_tracks_ais", ctx, model, n_tracks, L_max, n_legs);
    if (rc != MHT_OK) return rc;
    bool extras;
    const AisSteps steps = ais_steps(model, kind, ais_z, ais_r, leg, legs, n_legs, &extras);
    const TraceBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, radar_out};
    return run_trace<4>(ctx, "mht_trace_tracks_ais", steps, extras && ais_out, b, ais_out);
}
