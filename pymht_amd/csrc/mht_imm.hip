// mht_imm_tracks, mht_imm_tracks_ct (include/mht_amd.h): an interacting-multiple-model filter over a batch of track histories -- per
// node the posterior probability of each of r <= 4 noise levels and one combined state and covariance, per track the log-likelihood of
// its plots under the mixture.  The one family whose lanes are not alone:
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
    int rc = check_batch(seam, b, b.Q && b.R && b.Pi && b.mu0 && b.mu && b.x && b.P && b.ll && b.nobs, imm_work_bytes(N, b.n, b.r), "mht_imm_work_bytes",
                         MHT_E_INVALID);
    if (rc == MHT_OK) rc = check_chain(seam, b);
    if (rc != MHT_OK) return rc;
    const std::vector<double> table = imm_table<N>(b);
    const ImmArgs<N, Steps> a = imm_args<N>(steps, b);
    return run_over_lengths(ctx, seam, b, table.data(), table.size(), [&] {
        return launch_kernel(ctx, K_SMOOTH_SCORE, imm_kernel<N, Steps>, dim3((b.n + 15) / 16), dim3(64), 0, false, a);
    });
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_imm_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max, int32_t n_modes) {
    if ((nx != 4 && nx != 6) || n_tracks <= 0 || L_max < 0 || n_modes < 1 || n_modes > IMM_MAX_MODES) return 0;
    return imm_work_bytes(nx, n_tracks, n_modes);
}

// (the steps carry the model's Q and R too: every lane overwrites them with its mode's)
extern "C" int mht_imm_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                              const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes, const double* Q, const double* R,
                              const double* Pi, const double* mu0, double* mu, double* x, double* P, double* ll, int32_t* nobs, void* work,
                              size_t work_bytes) {
    const char* seam = "mht_imm_tracks";
    const int rc = check_linear(seam, ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const ImmBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, n_modes, Q, R, Pi, mu0, mu, x, P, ll, nobs};
    return model->nx == 4 ? run_imm<4>(ctx, seam, linear_steps<4>(model), b) : run_imm<6>(ctx, seam, linear_steps<6>(model), b);
}

extern "C" int mht_imm_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                                 const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes, const double* Q, const double* R,
                                 const double* Pi, const double* mu0, double* mu, double* x, double* P, double* ll, int32_t* nobs, void* work,
                                 size_t work_bytes) {
    const int rc = check_ct("mht_imm_tracks_ct", ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const ImmBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, n_modes, Q, R, Pi, mu0, mu, x, P, ll, nobs};
    return run_imm<6>(ctx, "mht_imm_tracks_ct", ct_steps(model), b);
}
