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
    for (int32_t t = 0; t < b.n; ++t)
        MHT_REQUIRE(b.len[t] >= 1 && b.len[t] <= b.L_max, "%s: track %d has length %d (1 .. L_max = %d)", seam, t, b.len[t], b.L_max);
    const size_t front = imm_work_bytes(N, b.n, b.r), need = front + imm_smooth_rows_bytes(N, b.n, b.L_max, b.r);
    MHT_REQUIRE(b.work_bytes >= need, "%s: the workspace has %zu bytes, %zu are needed (mht_imm_smooth_work_bytes)", seam, b.work_bytes, need);
    const int rcc = check_chain(seam, b);
    if (rcc != MHT_OK) return rcc;
    const std::vector<double> table = imm_table<N>(b);
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    char* w = static_cast<char*>(b.work);
    ImmSmoothArgs<N, Steps> a = {};
    a.f = imm_args<N>(steps, b);
    a.muf = muf;
    a.rows = reinterpret_cast<double*>(w + front);
    int rc = MHT_OK;
    // (the copies read the caller's array and `table`: whatever fails from here on, the stream is waited for before the error goes back)
    hipError_t e = hipMemcpyAsync(w, b.len, (size_t)b.n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w + smooth_len_bytes(b.n), table.data(), table.size() * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        set_error("%s: copying to the workspace: %s", seam, hipGetErrorString(e));
        rc = MHT_E_HIP;
    } else {
        rc = launch_kernel(ctx, K_SMOOTH_SCORE, imm_smooth_kernel<N, Steps>, dim3((b.n + 15) / 16), dim3(64), 0, false, a);
    }
    if (rc != MHT_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}

template <int N>
static int run_imm_smooth_linear(mht_ctx* ctx, const mht_model_x* model, const ImmBatch& b, double* muf) {
    LinearSteps<N> steps = {};
    widen<N>(model, steps.model, steps.model.A);      // (Q and R too: every lane overwrites them with its mode's)
    return run_imm_smooth<N>(ctx, "mht_imm_smooth_tracks", steps, b, muf);
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_imm_smooth_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max, int32_t n_modes) {
    if ((nx != 4 && nx != 6) || n_tracks <= 0 || L_max < 0 || n_modes < 1 || n_modes > IMM_MAX_MODES) return 0;
    return imm_work_bytes(nx, n_tracks, n_modes) + imm_smooth_rows_bytes(nx, n_tracks, L_max, n_modes);
}

extern "C" int mht_imm_smooth_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                     const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes,
                                     const double* Q, const double* R, const double* Pi, const double* mu0, double* mus, double* xs, double* Ps,
                                     double* muf, double* ll, int32_t* nobs, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_imm_smooth_tracks: null argument");
    MHT_REQUIRE(model->nx == 4 || model->nx == 6, "mht_imm_smooth_tracks: nx must be 4 or 6 (got %d)", model->nx);
    MHT_REQUIRE(model->transition == 0, "mht_imm_smooth_tracks: a state-dependent transition (%d) has no linear smoother to run", model->transition);
    MHT_REQUIRE(model->A && model->Q && model->C && model->R, "mht_imm_smooth_tracks: null model matrix");
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "mht_imm_smooth_tracks: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    const ImmBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, n_modes, Q, R, Pi, mu0, mus, xs, Ps, ll, nobs, work, work_bytes};
    return model->nx == 4 ? run_imm_smooth_linear<4>(ctx, model, b, muf) : run_imm_smooth_linear<6>(ctx, model, b, muf);
}

extern "C" int mht_imm_smooth_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                        const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_modes,
                                        const double* Q, const double* R, const double* Pi, const double* mu0, double* mus, double* xs, double* Ps,
                                        double* muf, double* ll, int32_t* nobs, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_imm_smooth_tracks_ct: null argument");
    MHT_REQUIRE(model->nx == 6, "mht_imm_smooth_tracks_ct: the constant-turn model has 6 states (got nx = %d)", model->nx);
    MHT_REQUIRE(model->transition == 1, "mht_imm_smooth_tracks_ct: transition must be 1 (got %d; a linear model belongs to mht_imm_smooth_tracks)",
                model->transition);
    MHT_REQUIRE(model->Q && model->C && model->R, "mht_imm_smooth_tracks_ct: null model matrix");
    MHT_REQUIRE(model->period > 0.0, "mht_imm_smooth_tracks_ct: the model's period must be positive (got %g)", model->period);
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "mht_imm_smooth_tracks_ct: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    ConstantTurnSteps steps = {};
    widen<6>(model, steps.model);
    steps.model.T = model->period;
    const ImmBatch b = {n_tracks, L_max, len, x_init, P_init, z, has_z, n_modes, Q, R, Pi, mu0, mus, xs, Ps, ll, nobs, work, work_bytes};
    return run_imm_smooth<6>(ctx, "mht_imm_smooth_tracks_ct", steps, b, muf);
}
