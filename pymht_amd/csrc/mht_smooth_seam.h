// Host side shared by the smoother seams (mht_smooth.hip, mht_smooth_em.hip): the model widened, the workspace's layout and size, the
// checks every seam makes of a batch, and the arguments of a walk over it.
#pragma once
#include "mht_common.h"
#include "mht_smooth_walk.h"

namespace mht {

// mht_model_x's float32 matrices in float64 (exact): Q, C, R, and A where the model has one
template <int N, typename Model>
static void widen(const mht_model_x* m, Model& out, double* A = nullptr) {
    if (A)
        for (int i = 0; i < N * N; ++i) A[i] = (double)m->A[i];
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j) out.Q[sym_idx(N, i, j)] = (double)m->Q[i * N + j];
    for (int i = 0; i < 2 * N; ++i) out.C[i] = (double)m->C[i];
    out.R[0] = (double)m->R[0]; out.R[1] = (double)m->R[1]; out.R[2] = (double)m->R[3];
}

static size_t smooth_len_bytes(int32_t n_tracks) { return (((size_t)n_tracks * 4 + 255) / 256) * 256; }

static size_t smooth_work_bytes(int32_t nx, int32_t slots, int32_t n_tracks, int32_t L_max) {
    return smooth_len_bytes(n_tracks) + (size_t)L_max * (size_t)slots * (size_t)(nx + nx * (nx + 1) / 2) * (size_t)n_tracks * 8;
}

struct SmoothBatch {      // what every seam is handed besides its model
    int32_t n, L_max;
    const int32_t* len;
    const double *x_init, *P_init, *z;
    const uint8_t* has_z;
    double *xs, *Ps;
    void* work;
    size_t work_bytes;
};

// What the seams ask of a non-empty batch behind their own model checks
static int check_batch(const char* seam, const char* sizer, int32_t nx, int32_t slots, const SmoothBatch& b, bool extras) {
    MHT_REQUIRE(b.len && b.x_init && b.P_init && b.z && b.has_z && extras && b.xs && b.work, "%s: null array", seam);
    for (int32_t t = 0; t < b.n; ++t)
        MHT_REQUIRE(b.len[t] >= 1 && b.len[t] <= b.L_max, "%s: track %d has length %d (1 .. L_max = %d)", seam, t, b.len[t], b.L_max);
    const size_t need = smooth_work_bytes(nx, slots, b.n, b.L_max);
    if (b.work_bytes < need) {
        set_error("%s: the workspace has %zu bytes, %zu are needed (%s)", seam, b.work_bytes, need, sizer);
        return MHT_E_CAPACITY;
    }
    return MHT_OK;
}

// The arguments of a walk over a checked batch: the lengths at the front of the workspace, the filtered means and covariances behind
// them; returns the first byte behind those
template <int N, typename Steps>
static char* smooth_args(const Steps& steps, const SmoothBatch& b, SmoothArgs<N, Steps>& a) {
    a = {};
    a.steps = steps;
    a.n = b.n; a.L_max = b.L_max;
    a.x_init = b.x_init; a.P_init = b.P_init; a.z = b.z; a.has_z = b.has_z; a.xs = b.xs; a.Ps = b.Ps;
    char* q = static_cast<char*>(b.work);
    a.len = reinterpret_cast<const int32_t*>(q); q += smooth_len_bytes(b.n);
    a.xf = reinterpret_cast<double*>(q); q += (size_t)b.L_max * Steps::SLOTS * N * (size_t)b.n * 8;
    a.Pf = reinterpret_cast<double*>(q); q += (size_t)b.L_max * Steps::SLOTS * (N * (N + 1) / 2) * (size_t)b.n * 8;
    return q;
}

// One forward-only score launch over a checked linear batch whose lengths are in the workspace (mht_smooth_score.hip), queued on the
// context's stream and not waited for: ll [n] <- each track's log-likelihood under the call's (x_init, P_init, Q, R) (theta null) or
// under its own theta [N + 2 NS + 3][n] in the EM workspace's layout.  What mht_smooth_tracks_em_ll puts in front of each EM walk.
int score_linear_launch(mht_ctx* ctx, const mht_model_x* model, const SmoothBatch& b, const double* theta, double* ll);

}  // namespace mht
