// mht_filter_tracks, mht_filter_tracks_ct, mht_filter_tracks_ais (include/mht_amd.h): the filtered state and covariance of every node of
// a batch of track histories -- what mht_smooth_tracks* computes going forward and keeps in its workspace, and mht_score_tracks* and
// mht_trace_tracks* compute and discard.  The fifth sibling next to smooth, EM, score and trace: one walk (smooth_filter_walk,
// mht_smooth_filter.h) with the smoothers' step policies, ONE TRACK PER LANE, everything in memory track-minor, no lane touching anything
// of another -- a track's figures do not depend on where in the batch it sits.  The workspace holds the lengths and nothing else; the
// outputs are [node][element][track], so the N + N (N + 1) / 2 stores a lane makes per node (14 at four states, 27 at six) are contiguous
// over a wavefront, and a lane writes EVERY row of its track, NaN behind its end: the caller's memory need not be initialised.  It is
// the score walk with those stores in place of its sums: nothing but (x, P), one prediction and one gain is live at a time; no LDS, no
// scratch (tests/test_filter_resources.py).
//
// A unit of its own: the smoother, score, grid and trace units keep their kernels, and their compiled resources, as they are.
#include "mht_common.h"
#include "mht_smooth_filter.h"
#include "mht_smooth_seam.h"

namespace mht {

template <int N, typename Steps>
__global__ void __launch_bounds__(64) smooth_filter_kernel(const FilterArgs<N, Steps> a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < a.n) smooth_filter_walk<N>(a, t);
}

static size_t filter_work_bytes(int32_t n_tracks) { return smooth_len_bytes(n_tracks); }      // the lengths

struct FilterBatch {      // what every filter seam is handed besides its model
    int32_t n, L_max;
    const int32_t* len;
    const double *x_init, *P_init, *z;
    const uint8_t* has_z;
    double *xf, *Pf;
    void* work;
    size_t work_bytes;
};

// An empty batch is done; any other is checked, then the lengths go to the workspace; then one launch and a wait
template <int N, typename Steps>
static int run_filter(mht_ctx* ctx, const char* seam, const Steps& steps, bool extras, const FilterBatch& b) {
    if (b.n == 0) return MHT_OK;
    MHT_REQUIRE(b.len && b.x_init && b.P_init && b.z && b.has_z && extras && b.xf && b.Pf && b.work, "%s: null array", seam);
    for (int32_t t = 0; t < b.n; ++t)
        MHT_REQUIRE(b.len[t] >= 1 && b.len[t] <= b.L_max, "%s: track %d has length %d (1 .. L_max = %d)", seam, t, b.len[t], b.L_max);
    MHT_REQUIRE(b.work_bytes >= filter_work_bytes(b.n), "%s: the workspace has %zu bytes, %zu are needed (mht_filter_work_bytes)", seam, b.work_bytes,
                filter_work_bytes(b.n));
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    FilterArgs<N, Steps> a = {};
    a.steps = steps;
    a.n = b.n; a.L_max = b.L_max;
    a.len = static_cast<const int32_t*>(b.work);
    a.x_init = b.x_init; a.P_init = b.P_init; a.z = b.z; a.has_z = b.has_z;
    a.xf = b.xf; a.Pf = b.Pf;
    MHT_HIP_CHECK(hipMemcpyAsync(b.work, b.len, (size_t)b.n * 4, hipMemcpyHostToDevice, ctx->stream));
    const int rc = launch_kernel(ctx, K_SMOOTH_SCORE, smooth_filter_kernel<N, Steps>, dim3((b.n + 63) / 64), dim3(64), 0, false, a);
    if (rc != MHT_OK) {      // (the copy of the lengths reads the caller's array: it is waited for before the error goes back)
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}

template <int N>
static int run_filter_linear(mht_ctx* ctx, const mht_model_x* model, const FilterBatch& b) {
    LinearSteps<N> steps = {};
    widen<N>(model, steps.model, steps.model.A);
    return run_filter<N>(ctx, "mht_filter_tracks", steps, true, b);
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_filter_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max) {
    if ((nx != 4 && nx != 6) || n_tracks < 0 || L_max < 0) return 0;
    return filter_work_bytes(n_tracks);
}

extern "C" int mht_filter_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                                 const double* P_init, const double* z, const uint8_t* has_z, double* xf, double* Pf, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_filter_tracks: null argument");
    MHT_REQUIRE(model->nx == 4 || model->nx == 6, "mht_filter_tracks: nx must be 4 or 6 (got %d)", model->nx);
    MHT_REQUIRE(model->transition == 0, "mht_filter_tracks: a state-dependent transition (%d) has no linear filter to run", model->transition);
    MHT_REQUIRE(model->A && model->Q && model->C && model->R, "mht_filter_tracks: null model matrix");
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "mht_filter_tracks: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    const FilterBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, xf, Pf, work, work_bytes};
    return model->nx == 4 ? run_filter_linear<4>(ctx, model, b) : run_filter_linear<6>(ctx, model, b);
}

extern "C" int mht_filter_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                                    const double* P_init, const double* z, const uint8_t* has_z, double* xf, double* Pf, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_filter_tracks_ct: null argument");
    MHT_REQUIRE(model->nx == 6, "mht_filter_tracks_ct: the constant-turn model has 6 states (got nx = %d)", model->nx);
    MHT_REQUIRE(model->transition == 1, "mht_filter_tracks_ct: transition must be 1 (got %d; a linear model belongs to mht_filter_tracks)", model->transition);
    MHT_REQUIRE(model->Q && model->C && model->R, "mht_filter_tracks_ct: null model matrix");
    MHT_REQUIRE(model->period > 0.0, "mht_filter_tracks_ct: the model's period must be positive (got %g)", model->period);
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "mht_filter_tracks_ct: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    ConstantTurnSteps steps = {};
    widen<6>(model, steps.model);
    steps.model.T = model->period;
    const FilterBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, xf, Pf, work, work_bytes};
    return run_filter<6>(ctx, "mht_filter_tracks_ct", steps, true, b);
}

extern "C" int mht_filter_tracks_ais(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                     const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                                     const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, int32_t n_legs,
                                     double* xf, double* Pf, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_filter_tracks_ais: null argument");
    MHT_REQUIRE(model->nx == 4, "mht_filter_tracks_ais: AIS messages report four states (got nx = %d)", model->nx);
    MHT_REQUIRE(model->transition == 0, "mht_filter_tracks_ais: a state-dependent transition (%d) has no AIS-aware filter to run", model->transition);
    MHT_REQUIRE(model->A && model->Q && model->C && model->R, "mht_filter_tracks_ais: null model matrix");
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1 && n_legs >= 0, "mht_filter_tracks_ais: bad size (n_tracks %d, L_max %d, n_legs %d)", n_tracks, L_max, n_legs);
    AisSteps steps = {};
    widen<4>(model, steps.model, steps.model.A);
    steps.kind = kind; steps.ais_z = ais_z; steps.ais_r = ais_r; steps.leg = leg; steps.legs = legs;
    const FilterBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, xf, Pf, work, work_bytes};
    return run_filter<4>(ctx, "mht_filter_tracks_ais", steps, kind && ais_z && ais_r && leg && (legs || n_legs == 0), b);
}
