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
#include <cmath>
#include <vector>

#include "mht_common.h"
#include "mht_imm.h"
#include "mht_smooth_seam.h"

namespace mht {

// v as lane I of the caller's quad holds it.  Two ways, timed in profiles/imm_cost.txt: a DPP quad_perm broadcast on the two halves of
// the double (the default: no LDS crossbar, no address), or __shfl at the quad's lane (-DMHT_IMM_QUAD_SHFL).
template <int I>
__device__ __forceinline__ double quad_read_at(double v) {
#if defined(MHT_IMM_QUAD_SHFL)
    return __shfl(v, (int)((threadIdx.x & ~3u) | I), 64);
#else
    constexpr int ctrl = I * 0x55;      // quad_perm:[I, I, I, I]
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, ctrl, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(lo, lo, ctrl, 0xf, 0xf, false));
#endif
}

__device__ __forceinline__ double quad_read(double v, int i) {      // (i is a constant wherever the walk's loops are unrolled)
    switch (i) {
        case 0: return quad_read_at<0>(v);
        case 1: return quad_read_at<1>(v);
        case 2: return quad_read_at<2>(v);
        default: return quad_read_at<3>(v);
    }
}

template <int N, typename Steps>
struct QuadLanes {      // the Lanes policy of a kernel: the lane's own mode, the others through the quad
    ImmLane<N, Steps> own;
    int j;
    __device__ __forceinline__ static constexpr int count() { return 1; }
    __device__ __forceinline__ int mode(int) const { return j; }
    __device__ __forceinline__ ImmLane<N, Steps>& lane(int) { return own; }
    __device__ __forceinline__ double get(int, int i, int e) const { return quad_read(own.s[e], i); }
};

template <int N, typename Steps>
__global__ void __launch_bounds__(64) imm_kernel(const ImmArgs<N, Steps> a) {
    const int j = threadIdx.x & 3, t = blockIdx.x * 16 + (threadIdx.x >> 2);
    if (j >= a.r || t >= a.n) return;
    QuadLanes<N, Steps> L;
    L.j = j;
    imm_walk<N, Steps>(a, t, L);
}

static size_t imm_table_bytes(int32_t nx, int32_t r) {      // the mode table, Pi, mu0
    return (((size_t)r * (smooth_score_grid_row(nx) + r + 1) * 8 + 255) / 256) * 256;
}

static size_t imm_work_bytes(int32_t nx, int32_t n_tracks, int32_t r) { return smooth_len_bytes(n_tracks) + imm_table_bytes(nx, r); }

struct ImmBatch {      // what both seams are handed besides their model
    int32_t n, L_max;
    const int32_t* len;
    const double *x_init, *P_init, *z;
    const uint8_t* has_z;
    int32_t r;
    const double *Q, *R, *Pi, *mu0;
    double *mu, *x, *P, *ll;
    int32_t* nobs;
    void* work;
    size_t work_bytes;
};

// A distribution over the modes: entries in [0, 1] that add up to 1
static int check_distribution(const char* seam, const char* what, int row, const double* p, int32_t r) {
    double sum = 0.0;
    for (int32_t i = 0; i < r; ++i) {
        MHT_REQUIRE(p[i] >= 0.0 && p[i] <= 1.0, "%s: %s[%d][%d] = %g is no probability", seam, what, row, i, p[i]);
        sum += p[i];
    }
    MHT_REQUIRE(std::fabs(sum - 1.0) <= 1e-9, "%s: %s[%d] adds up to %.17g, not to 1", seam, what, row, sum);
    return MHT_OK;
}

// An empty batch is done; any other is checked, the lengths, the packed modes, Pi and mu0 go to the workspace; then one launch and a wait
template <int N, typename Steps>
static int run_imm(mht_ctx* ctx, const char* seam, const Steps& steps, const ImmBatch& b) {
    constexpr int NS = N * (N + 1) / 2;
    MHT_REQUIRE(b.r >= 1 && b.r <= IMM_MAX_MODES, "%s: n_modes must be 1 .. %d (got %d)", seam, IMM_MAX_MODES, b.r);
    if (b.n == 0) return MHT_OK;
    MHT_REQUIRE(b.len && b.x_init && b.P_init && b.z && b.has_z && b.Q && b.R && b.Pi && b.mu0 && b.mu && b.x && b.P && b.ll && b.nobs && b.work,
                "%s: null array", seam);
    for (int32_t t = 0; t < b.n; ++t)
        MHT_REQUIRE(b.len[t] >= 1 && b.len[t] <= b.L_max, "%s: track %d has length %d (1 .. L_max = %d)", seam, t, b.len[t], b.L_max);
    const size_t need = imm_work_bytes(N, b.n, b.r);
    MHT_REQUIRE(b.work_bytes >= need, "%s: the workspace has %zu bytes, %zu are needed (mht_imm_work_bytes)", seam, b.work_bytes, need);
    for (int32_t i = 0; i < b.r; ++i) {
        const int rc = check_distribution(seam, "Pi", i, b.Pi + (size_t)i * b.r, b.r);
        if (rc != MHT_OK) return rc;
    }
    const int rc0 = check_distribution(seam, "mu0", 0, b.mu0, b.r);
    if (rc0 != MHT_OK) return rc0;
    const size_t row = NS + 3;
    std::vector<double> table((size_t)b.r * (row + b.r + 1));
    for (int32_t g = 0; g < b.r; ++g) {
        double* out = table.data() + (size_t)g * row;
        const double *Q = b.Q + (size_t)g * N * N, *R = b.R + (size_t)g * 4;
        for (int i = 0; i < N; ++i)
            for (int j = i; j < N; ++j) out[sym_idx(N, i, j)] = Q[i * N + j];
        out[NS] = R[0]; out[NS + 1] = R[1]; out[NS + 2] = R[3];
    }
    for (int32_t i = 0; i < b.r * b.r; ++i) table[(size_t)b.r * row + i] = b.Pi[i];
    for (int32_t i = 0; i < b.r; ++i) table[(size_t)b.r * (row + b.r) + i] = b.mu0[i];
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    char* w = static_cast<char*>(b.work);
    ImmArgs<N, Steps> a = {};
    a.steps = steps;
    a.n = b.n; a.L_max = b.L_max; a.r = b.r;
    a.len = reinterpret_cast<const int32_t*>(w);
    a.x_init = b.x_init; a.P_init = b.P_init; a.z = b.z; a.has_z = b.has_z;
    a.modes = reinterpret_cast<const double*>(w + smooth_len_bytes(b.n));
    a.Pi = a.modes + (size_t)b.r * row;
    a.mu0 = a.Pi + (size_t)b.r * b.r;
    a.mu = b.mu; a.x = b.x; a.P = b.P; a.ll = b.ll; a.nobs = b.nobs;
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
