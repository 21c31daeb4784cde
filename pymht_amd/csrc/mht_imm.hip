// mht_imm_tracks, mht_imm_tracks_ct (include/mht_amd.h): an interacting-multiple-model filter over a batch of track histories -- per
// node the posterior probability of each of r <= 4 noise levels and one combined state and covariance, per track the log-likelihood of
// its plots under the mixture.  The sixth sibling next to smooth, EM, score, trace and filter, and the first whose lanes are not alone:
// ONE (TRACK, MODE) PER LANE, the four lanes of a quad being the modes of one track, sixteen tracks to a wavefront.  Modes in a loop
// inside one lane would hold r states at once (108 doubles at six states and four modes, before any temporary); a mode per lane is the
// filter kernel's size plus the mixing, and what a mode needs of the others it reads from their registers (quad_read), one element at a
// time (imm_moments, mht_imm.h).
//
// Every branch of the walk but the select on cbar_j > 0 depends on the track only -- its length, whether a node has a plot -- so the
// lanes of a quad stay together, and a cross-lane read only ever names a lane < r of the lane's own quad: lanes whose mode is >= r or
// whose track is >= n leave before the walk.  Everything in memory is track-minor; the combined state is computed by every lane of a
// quad from the same operands in the same order and stored by mode 0, sixteen consecutive doubles a wavefront and element.  The
// workspace holds the lengths, the mode table [r][NS + 3], Pi and mu0; no LDS, no scratch (tests/test_imm_resources.py).
#include "mht_imm_quad.h"

namespace mht {

template <int N, typename Steps>
__global__ void __launch_bounds__(64) imm_kernel(const ImmArgs<N, Steps> a) {
    const int j = threadIdx.x & 3, t = blockIdx.x * 16 + (threadIdx.x >> 2);
    if (j >= a.r || t >= a.n) return;
    QuadLanes<N, Steps> L;
    L.j = j;
    imm_walk<N, Steps>(a, t, L);
}

// An empty batch is done; any other is checked, the lengths, the packed modes, Pi and mu0 go to the workspace; then one launch and a wait
template <int N, typename Steps>
static int run_imm(mht_ctx* ctx, const char* seam, const Steps& steps, const ImmBatch& b) {
    MHT_REQUIRE(b.r >= 1 && b.r <= IMM_MAX_MODES, "%s: n_modes must be 1 .. %d (got %d)", seam, IMM_MAX_MODES, b.r);
    if (b.n == 0) return MHT_OK;
    MHT_REQUIRE(b.len && b.x_init && b.P_init && b.z && b.has_z && b.Q && b.R && b.Pi && b.mu0 && b.mu && b.x && b.P && b.ll && b.nobs && b.work,
                "%s: null array", seam);
    for (int32_t t = 0; t < b.n; ++t)
        MHT_REQUIRE(b.len[t] >= 1 && b.len[t] <= b.L_max, "%s: track %d has length %d (1 .. L_max = %d)", seam, t, b.len[t], b.L_max);
    const size_t need = imm_work_bytes(N, b.n, b.r);
    MHT_REQUIRE(b.work_bytes >= need, "%s: the workspace has %zu bytes, %zu are needed (mht_imm_work_bytes)", seam, b.work_bytes, need);
    const int rcc = check_chain(seam, b);
    if (rcc != MHT_OK) return rcc;
    const std::vector<double> table = imm_table<N>(b);
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    char* w = static_cast<char*>(b.work);
    const ImmArgs<N, Steps> a = imm_args<N>(steps, b);
    int rc = MHT_OK;
    // (the copies read the caller's array and `table`: whatever fails from here on, the stream is waited for before the error goes back)
    hipError_t e = hipMemcpyAsync(w, b.len, (size_t)b.n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w + smooth_len_bytes(b.n), table.data(), table.size() * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        set_error("%s: copying to the workspace: %s", seam, hipGetErrorString(e));
        rc = MHT_E_HIP;
    } else {
        rc = launch_kernel(ctx, K_SMOOTH_SCORE, imm_kernel<N, Steps>, dim3((b.n + 15) / 16), dim3(64), 0, false, a);
    }
    if (rc != MHT_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}

template <int N>
static int run_imm_linear(mht_ctx* ctx, const mht_model_x* model, const ImmBatch& b) {
    LinearSteps<N> steps = {};
    widen<N>(model, steps.model, steps.model.A);      // (Q and R too: every lane overwrites them with its mode's)
    return run_imm<N>(ctx, "mht_imm_tracks", steps, b);
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_imm_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max, int32_t n_modes) {
    if ((nx != 4 && nx != 6) || n_tracks <= 0 || L_max < 0 || n_modes < 1 || n_modes > IMM_MAX_MODES) return 0;
    return imm_work_bytes(nx, n_tracks, n_modes);
}

extern "C" int mht_imm_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                              const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes, const double* Q, const double* R,
                              const double* Pi, const double* mu0, double* mu, double* x, double* P, double* ll, int32_t* nobs, void* work,
                              size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_imm_tracks: null argument");
    MHT_REQUIRE(model->nx == 4 || model->nx == 6, "mht_imm_tracks: nx must be 4 or 6 (got %d)", model->nx);
    MHT_REQUIRE(model->transition == 0, "mht_imm_tracks: a state-dependent transition (%d) has no linear filter to run", model->transition);
    MHT_REQUIRE(model->A && model->Q && model->C && model->R, "mht_imm_tracks: null model matrix");
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "mht_imm_tracks: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    const ImmBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, n_modes, Q, R, Pi, mu0, mu, x, P, ll, nobs, work, work_bytes};
    return model->nx == 4 ? run_imm_linear<4>(ctx, model, b) : run_imm_linear<6>(ctx, model, b);
}

extern "C" int mht_imm_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                                 const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes, const double* Q, const double* R,
                                 const double* Pi, const double* mu0, double* mu, double* x, double* P, double* ll, int32_t* nobs, void* work,
                                 size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_imm_tracks_ct: null argument");
    MHT_REQUIRE(model->nx == 6, "mht_imm_tracks_ct: the constant-turn model has 6 states (got nx = %d)", model->nx);
    MHT_REQUIRE(model->transition == 1, "mht_imm_tracks_ct: transition must be 1 (got %d; a linear model belongs to mht_imm_tracks)", model->transition);
    MHT_REQUIRE(model->Q && model->C && model->R, "mht_imm_tracks_ct: null model matrix");
    MHT_REQUIRE(model->period > 0.0, "mht_imm_tracks_ct: the model's period must be positive (got %g)", model->period);
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "mht_imm_tracks_ct: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    ConstantTurnSteps steps = {};
    widen<6>(model, steps.model);
    steps.model.T = model->period;
    const ImmBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, n_modes, Q, R, Pi, mu0, mu, x, P, ll, nobs, work, work_bytes};
    return run_imm<6>(ctx, "mht_imm_tracks_ct", steps, b);
}
