// mht_imm_smooth_tracks, mht_imm_smooth_tracks_ct (include/mht_amd.h): the fixed-interval IMM smoother over a batch of track histories
// -- per node the probability of each of r <= 4 noise levels in hindsight and one smoothed state and covariance.  The walk and the
// recursion are mht_imm_smooth.h's; the lanes are mht_imm.hip's: ONE (TRACK, MODE) PER LANE, the four lanes of a quad being the modes of
// one track, what a mode needs of the others read from their registers (quad_read, mht_imm_quad.h).
//
// One launch: a lane walks its track forward and then backward, as the lanes of mht_smooth.hip do, and the last node's rows never
// leave the registers in between.  Going forward every mode stores its own row [xf | Pf packed | mu] per node in the workspace,
// track-minor; going backward it loads only the rows it stored itself, so nothing is read that another lane wrote.  Every branch but
// the selects depends on the track only, so the lanes of a quad stay together; lanes whose mode is >= r or whose track is >= n leave
// before the walk.  These kernels live in their own translation unit: tests/test_imm_resources.py counts the kernels of mht_imm.hip.
// No LDS, no scratch (tests/test_imm_smooth_resources.py).
#include "mht_imm_quad.h"
#include "mht_imm_smooth.h"

namespace mht {

template <int N, typename Steps>
__global__ void __launch_bounds__(64) imm_smooth_kernel(const ImmSmoothArgs<N, Steps> b) {
    const int j = threadIdx.x & 3, t = blockIdx.x * 16 + (threadIdx.x >> 2);
    if (j >= b.f.r || t >= b.f.n) return;
    QuadLanes<N, Steps> L;
    L.j = j;
    imm_smooth_walk<N, Steps>(b, t, L);
}

static size_t imm_smooth_rows_bytes(int32_t nx, int32_t n_tracks, int32_t L_max, int32_t r) {
    const size_t row = (size_t)nx + (size_t)nx * (nx + 1) / 2 + 1;
    return (((size_t)L_max * (size_t)r * row * (size_t)n_tracks * 8 + 255) / 256) * 256;
}

// An empty batch is done; any other is checked as run_imm checks it, the lengths and the table go to the workspace; one launch and a wait
template <int N, typename Steps>
static int run_imm_smooth(mht_ctx* ctx, const char* seam, const Steps& steps, const ImmBatch& b, double* muf) {
    MHT_REQUIRE(b.r >= 1 && b.r <= IMM_MAX_MODES, "%s: n_modes must be 1 .. %d (got %d)", seam, IMM_MAX_MODES, b.r);
    if (b.n == 0) return MHT_OK;
    MHT_REQUIRE(b.len && b.x_init && b.P_init && b.z && b.has_z && b.Q && b.R && b.Pi && b.mu0 && b.mu && b.x && b.P && b.work, "%s: null array", seam);
    MHT_REQUIRE((b.ll == nullptr) == (b.nobs == nullptr), "%s: ll and nobs are handed over together, or both left out", seam);
    const size_t front = imm_work_bytes(N, b.n, b.r);
    int rc = check_lengths(seam, b);
    if (rc == MHT_OK) rc = check_workspace(seam, b, front + imm_smooth_rows_bytes(N, b.n, b.L_max, b.r), "mht_imm_smooth_work_bytes", MHT_E_INVALID);
    if (rc == MHT_OK) rc = check_chain(seam, b);
    if (rc != MHT_OK) return rc;
    const std::vector<double> table = imm_table<N>(b);
    ImmSmoothArgs<N, Steps> a = {};
    a.f = imm_args<N>(steps, b);
    a.muf = muf;
    a.rows = reinterpret_cast<double*>(static_cast<char*>(b.work) + front);
    return run_over_lengths(ctx, seam, b, table.data(), table.size(), [&] {
        return launch_kernel(ctx, K_SMOOTH_SCORE, imm_smooth_kernel<N, Steps>, dim3((b.n + 15) / 16), dim3(64), 0, false, a);
    });
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_imm_smooth_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max, int32_t n_modes) {
    if ((nx != 4 && nx != 6) || n_tracks <= 0 || L_max < 0 || n_modes < 1 || n_modes > IMM_MAX_MODES) return 0;
    return imm_work_bytes(nx, n_tracks, n_modes) + imm_smooth_rows_bytes(nx, n_tracks, L_max, n_modes);
}

// (the steps carry the model's Q and R too: every lane overwrites them with its mode's)
extern "C" int mht_imm_smooth_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                     const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes,
                                     const double* Q, const double* R, const double* Pi, const double* mu0, double* mus, double* xs, double* Ps,
                                     double* muf, double* ll, int32_t* nobs, void* work, size_t work_bytes) {
    const char* seam = "mht_imm_smooth_tracks";
    const int rc = check_linear(seam, ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const ImmBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, n_modes, Q, R, Pi, mu0, mus, xs, Ps, ll, nobs};
    return model->nx == 4 ? run_imm_smooth<4>(ctx, seam, linear_steps<4>(model), b, muf) : run_imm_smooth<6>(ctx, seam, linear_steps<6>(model), b, muf);
}

extern "C" int mht_imm_smooth_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                        const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes,
                                        const double* Q, const double* R, const double* Pi, const double* mu0, double* mus, double* xs, double* Ps,
                                        double* muf, double* ll, int32_t* nobs, void* work, size_t work_bytes) {
    const int rc = check_ct("mht_imm_smooth_tracks_ct", ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const ImmBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, n_modes, Q, R, Pi, mu0, mus, xs, Ps, ll, nobs};
    return run_imm_smooth<6>(ctx, "mht_imm_smooth_tracks_ct", ct_steps(model), b, muf);
}
