// mht_smooth_tracks: fixed-interval Rauch-Tung-Striebel smoothing of a batch of track histories (include/mht_amd.h; the arithmetic is
// mht_smooth_math.h).  What the reference does per track with pykalman at the end of a run (Target.getSmoothTrack, pyTarget.py:580-609,
// behind every exported <Track>, pyTarget.py:745-802), for ALL tracks of an export in one launch.
//
// Mapping: ONE TRACK PER LANE.  A track is a serial chain of small matrix steps and the tracks are independent, so a lane walks its track
// forward (filter) and then backward (smoother) with every matrix in registers, and everything the lanes touch in memory is laid out
// track-minor -- [node][element][track] -- so that one load or store instruction of a wavefront covers 64 consecutive doubles.  The forward
// pass leaves the filtered mean and covariance (packed symmetric) of every node in the caller's workspace; the backward pass reads them
// back (each lane its own column: no synchronisation) and recomputes the prediction from them, which costs one 6 x 6 x 6 product less than it
// sounds because G needs A Pf anyway.  Tracks have different lengths: a lane stops at its own, so a wavefront runs as long as its longest
// track and shorter lanes idle -- callers that care put tracks of similar length next to each other (pymht_amd.smoothing sorts by length);
// no lane reads or writes anything of another, so the result of a track does not depend on where in the batch it sits.
// Registers: one wavefront per workgroup and __launch_bounds__(64) give a lane the whole 512-entry file; the six-state covariance
// kernel needs most of a backward step's matrices live at once (Pf, A Pf, U, G, Ps - Pp) and must not spill (tests/test_smooth_resources.py).
// A batch is a few dozen wavefronts, far fewer than the device has SIMDs: occupancy is not what bounds it, the chain's latency is.
//
// mht_smooth_tracks_ct: the same walk (smooth_walk below: same mapping, same layouts, same workspace) for the constant-turn model, whose
// transition A_k = Phi(T, w) is rebuilt per lane and per node from the filtered turn rate (mht_smooth_ct_math.h).  The backward pass
// RECOMPUTES sin / cos from the xf_k[4] it reads back anyway instead of keeping sw, cw, c, s in the workspace: the same function of the
// same bits gives the A_k the forward pass predicted with, the workspace stays that of the linear six-state smoother (27 doubles a
// node, not 31, and four loads fewer on the chain), and float64 sin / cos cost about 30 registers and no scratch, which the kernel has
// to spare because A_k is four numbers and not a matrix (tests/test_smooth_ct_resources.py).  What the recomputation costs in time is
// measured by tools/smooth_cost.py --ct (profiles/smooth_ct_cost.txt).
#include "mht_common.h"
#include "mht_smooth_ct_math.h"

namespace mht {

template <int N, typename Model = SmoothModel<N>>
struct SmoothArgs {
    Model model;
    int32_t n, L_max;
    const int32_t* len;       // [n] (in the workspace)
    const double* x_init;     // [N][n]
    const double* P_init;     // [N*N][n]
    const double* z;          // [L_max][2][n]
    const uint8_t* has_z;     // [L_max][n]
    double* xs;               // [L_max][N][n]
    double* Ps;               // [L_max][N(N+1)/2][n] or null
    double* xf;               // workspace [L_max][N][n]
    double* Pf;               // workspace [L_max][N(N+1)/2][n]
};

// What differs between the models: the prediction from a filtered state and the backward step (smooth_update takes either model)
template <int N>
struct LinearSteps {
    static __device__ __forceinline__ void predict(const SmoothModel<N>& m, const double* xf, const double* Pf, double* xp, double* AP, double* Pp) {
        smooth_predict<N>(m, xf, Pf, xp, AP, Pp);
    }
    template <bool COV>
    static __device__ __forceinline__ void backward(const SmoothModel<N>& m, const double* xf, const double* Pf, double* xs, double* Ps) {
        smooth_backward<N, COV>(m, xf, Pf, xs, Ps);
    }
};
struct ConstantTurnSteps {
    static __device__ __forceinline__ void predict(const SmoothCtModel& m, const double* xf, const double* Pf, double* xp, double* AP, double* Pp) {
        smooth_ct_predict(m, ct_transition(m.T, xf[4]), xf, Pf, xp, AP, Pp);
    }
    template <bool COV>
    static __device__ __forceinline__ void backward(const SmoothCtModel& m, const double* xf, const double* Pf, double* xs, double* Ps) {
        smooth_ct_backward<COV>(m, xf, Pf, xs, Ps);
    }
};

// One lane's track, forward and backward
template <int N, bool COV, typename Steps, typename Model>
__device__ __forceinline__ void smooth_walk(const SmoothArgs<N, Model>& a) {
    constexpr int NS = N * (N + 1) / 2;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.n) return;
    const size_t n = (size_t)a.n;
    const int len = a.len[t];      // 1 <= len <= L_max: checked by the host before the launch
    double x[N], P[NS];
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = a.x_init[(size_t)i * n + t];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) P[sym_idx(N, i, j)] = a.P_init[(size_t)(i * N + j) * n + t];
    // forward: node 0 is the initial state; node k >= 1 predicts and, with a measurement, updates
    for (int k = 0; k < len; ++k) {
        if (k > 0) {
            double xp[N], AP[N * N], Pp[NS];
            Steps::predict(a.model, x, P, xp, AP, Pp);
#pragma unroll
            for (int i = 0; i < N; ++i) x[i] = xp[i];
#pragma unroll
            for (int e = 0; e < NS; ++e) P[e] = Pp[e];
            if (a.has_z[(size_t)k * n + t]) smooth_update<N>(a.model, a.z[((size_t)k * 2) * n + t], a.z[((size_t)k * 2 + 1) * n + t], x, P);
        }
        if (k < len - 1) {      // (the last node's filtered state is its smoothed state: it stays in registers)
#pragma unroll
            for (int i = 0; i < N; ++i) a.xf[((size_t)k * N + i) * n + t] = x[i];
#pragma unroll
            for (int e = 0; e < NS; ++e) a.Pf[((size_t)k * NS + e) * n + t] = P[e];
        }
    }
    // backward: (x, P) is the smoothed state of node k + 1 on entry of a step and of node k afterwards
    for (int k = len - 1; k >= 0; --k) {
        if (k < len - 1) {
            double xf[N], Pf[NS];
#pragma unroll
            for (int i = 0; i < N; ++i) xf[i] = a.xf[((size_t)k * N + i) * n + t];
#pragma unroll
            for (int e = 0; e < NS; ++e) Pf[e] = a.Pf[((size_t)k * NS + e) * n + t];
            Steps::template backward<COV>(a.model, xf, Pf, x, P);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) a.xs[((size_t)k * N + i) * n + t] = x[i];
        if (COV) {
#pragma unroll
            for (int e = 0; e < NS; ++e) a.Ps[((size_t)k * NS + e) * n + t] = P[e];
        }
    }
}

template <int N, bool COV>
__global__ void __launch_bounds__(64) smooth_rts_kernel(const SmoothArgs<N> a) {
    smooth_walk<N, COV, LinearSteps<N>>(a);
}

template <bool COV>
__global__ void __launch_bounds__(64) smooth_rts_ct_kernel(const SmoothArgs<6, SmoothCtModel> a) {
    smooth_walk<6, COV, ConstantTurnSteps>(a);
}

static size_t smooth_len_bytes(int32_t n_tracks) { return (((size_t)n_tracks * 4 + 255) / 256) * 256; }

static size_t smooth_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max) {
    return smooth_len_bytes(n_tracks) + (size_t)L_max * (size_t)(nx + nx * (nx + 1) / 2) * (size_t)n_tracks * 8;
}

// The lengths go to the front of the workspace, the filtered means and covariances behind them; then one launch and a wait
template <int N, typename Model, typename Launch>
static int run_smooth(mht_ctx* ctx, SmoothArgs<N, Model>& a, int32_t n, int32_t L_max, const int32_t* len, const double* x_init, const double* P_init,
                      const double* z, const uint8_t* has_z, double* xs, double* Ps, void* work, Launch launch) {
    a.n = n; a.L_max = L_max;
    a.x_init = x_init; a.P_init = P_init; a.z = z; a.has_z = has_z; a.xs = xs; a.Ps = Ps;
    char* q = static_cast<char*>(work);
    a.len = reinterpret_cast<const int32_t*>(q); q += smooth_len_bytes(n);
    a.xf = reinterpret_cast<double*>(q); q += (size_t)L_max * N * (size_t)n * 8;
    a.Pf = reinterpret_cast<double*>(q);
    MHT_HIP_CHECK(hipMemcpyAsync(work, len, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    launch(dim3((n + 63) / 64), dim3(64));
    MHT_HIP_CHECK(hipGetLastError());
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}

template <int N>
static int run_linear(mht_ctx* ctx, const mht_model_x* m, int32_t n, int32_t L_max, const int32_t* len, const double* x_init, const double* P_init,
                      const double* z, const uint8_t* has_z, double* xs, double* Ps, void* work) {
    SmoothArgs<N> a = {};
    for (int i = 0; i < N * N; ++i) a.model.A[i] = (double)m->A[i];
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j) a.model.Q[sym_idx(N, i, j)] = (double)m->Q[i * N + j];
    for (int i = 0; i < 2 * N; ++i) a.model.C[i] = (double)m->C[i];
    a.model.R[0] = (double)m->R[0]; a.model.R[1] = (double)m->R[1]; a.model.R[2] = (double)m->R[3];
    return run_smooth(ctx, a, n, L_max, len, x_init, P_init, z, has_z, xs, Ps, work, [&](dim3 grid, dim3 block) {
        if (Ps) hipLaunchKernelGGL((smooth_rts_kernel<N, true>), grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL((smooth_rts_kernel<N, false>), grid, block, 0, ctx->stream, a);
    });
}

static int run_ct(mht_ctx* ctx, const mht_model_x* m, int32_t n, int32_t L_max, const int32_t* len, const double* x_init, const double* P_init,
                  const double* z, const uint8_t* has_z, double* xs, double* Ps, void* work) {
    SmoothArgs<6, SmoothCtModel> a = {};
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) a.model.Q[sym_idx(6, i, j)] = (double)m->Q[i * 6 + j];
    for (int i = 0; i < 12; ++i) a.model.C[i] = (double)m->C[i];
    a.model.R[0] = (double)m->R[0]; a.model.R[1] = (double)m->R[1]; a.model.R[2] = (double)m->R[3];
    a.model.T = m->period;
    return run_smooth(ctx, a, n, L_max, len, x_init, P_init, z, has_z, xs, Ps, work, [&](dim3 grid, dim3 block) {
        if (Ps) hipLaunchKernelGGL((smooth_rts_ct_kernel<true>), grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL((smooth_rts_ct_kernel<false>), grid, block, 0, ctx->stream, a);
    });
}

// What both seams ask of a non-empty batch behind their own model checks
static int check_batch(const char* seam, const char* sizer, int32_t nx, int32_t n_tracks, int32_t L_max, const int32_t* len, const double* x_init,
                       const double* P_init, const double* z, const uint8_t* has_z, const double* xs, const void* work, size_t work_bytes) {
    MHT_REQUIRE(len && x_init && P_init && z && has_z && xs && work, "%s: null array", seam);
    for (int32_t t = 0; t < n_tracks; ++t)
        MHT_REQUIRE(len[t] >= 1 && len[t] <= L_max, "%s: track %d has length %d (1 .. L_max = %d)", seam, t, len[t], L_max);
    const size_t need = smooth_work_bytes(nx, n_tracks, L_max);
    if (work_bytes < need) {
        set_error("%s: the workspace has %zu bytes, %zu are needed (%s)", seam, work_bytes, need, sizer);
        return MHT_E_CAPACITY;
    }
    return MHT_OK;
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_smooth_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max) {
    if ((nx != 4 && nx != 6) || n_tracks < 0 || L_max < 0) return 0;
    return smooth_work_bytes(nx, n_tracks, L_max);
}

extern "C" int mht_smooth_tracks(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                 const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* xs, double* Ps,
                                 void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_smooth_tracks: null argument");
    MHT_REQUIRE(model->nx == 4 || model->nx == 6, "mht_smooth_tracks: nx must be 4 or 6 (got %d)", model->nx);
    MHT_REQUIRE(model->transition == 0, "mht_smooth_tracks: a state-dependent transition (%d) has no linear smoother", model->transition);
    MHT_REQUIRE(model->A && model->Q && model->C && model->R, "mht_smooth_tracks: null model matrix");
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "mht_smooth_tracks: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    if (n_tracks == 0) return MHT_OK;
    const int rc = check_batch("mht_smooth_tracks", "mht_smooth_work_bytes", model->nx, n_tracks, L_max, len, x_init, P_init, z, has_z, xs, work, work_bytes);
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    if (model->nx == 4) return run_linear<4>(ctx, model, n_tracks, L_max, len, x_init, P_init, z, has_z, xs, Ps, work);
    return run_linear<6>(ctx, model, n_tracks, L_max, len, x_init, P_init, z, has_z, xs, Ps, work);
}

extern "C" size_t mht_smooth_ct_work_bytes(int32_t n_tracks, int32_t L_max) {
    if (n_tracks < 0 || L_max < 0) return 0;
    return smooth_work_bytes(6, n_tracks, L_max);
}

extern "C" int mht_smooth_tracks_ct(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                    const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* xs, double* Ps,
                                    void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_smooth_tracks_ct: null argument");
    MHT_REQUIRE(model->nx == 6, "mht_smooth_tracks_ct: the constant-turn model has 6 states (got nx = %d)", model->nx);
    MHT_REQUIRE(model->transition == 1, "mht_smooth_tracks_ct: transition must be 1 (got %d; a linear model belongs to mht_smooth_tracks)", model->transition);
    MHT_REQUIRE(model->Q && model->C && model->R, "mht_smooth_tracks_ct: null model matrix");
    MHT_REQUIRE(model->period > 0.0, "mht_smooth_tracks_ct: the model's period must be positive (got %g)", model->period);
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1, "mht_smooth_tracks_ct: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    if (n_tracks == 0) return MHT_OK;
    const int rc = check_batch("mht_smooth_tracks_ct", "mht_smooth_ct_work_bytes", 6, n_tracks, L_max, len, x_init, P_init, z, has_z, xs, work, work_bytes);
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    return run_ct(ctx, model, n_tracks, L_max, len, x_init, P_init, z, has_z, xs, Ps, work);
}
