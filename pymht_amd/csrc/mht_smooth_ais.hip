// mht_smooth_tracks_ais: fixed-interval Rauch-Tung-Striebel smoothing of a batch of AIS-aided track histories with the model the forest
// filtered them with (include/mht_amd.h; the arithmetic is mht_smooth_ais_math.h on top of mht_smooth_math.h).  Four states, opt-in:
// nothing routes here unless the caller asks (ais=True in the Python API).
//
// Mapping: the smoother's (mht_smooth.hip), because a batch of independent serial chains has no better one.  ONE TRACK PER LANE, one
// wavefront per workgroup and __launch_bounds__(64); a lane walks its track forward and then backward with every matrix in registers and
// stops at its own length; every per-lane array is track-minor -- [node][element][track] -- so one load or store of a wavefront covers
// 64 consecutive values; no lane touches another's data, so there is no LDS, no atomic and no barrier, and a track's result does not
// depend on its place in the batch.
//
// What a node is comes from two bytes a lane reads per node: has_z (a radar update, as in mht_smooth_tracks) and kind (>= 2: the node took
// an AIS message and steps over two legs instead of one period).  Lanes of a wavefront disagree about it, so a wavefront with AIS nodes
// in some lanes runs both paths; the plain path is the linear kernel's, call for call.
//
// The legs' matrices are NOT wave-uniform: (dT1, dT2) belongs to the message.  They come from a small table of one entry per distinct
// (dT1, dT2) of the batch, 52 doubles each, which a lane indexes with leg[node][track]: a GATHER, the one access here that does not
// coalesce.  That is accepted: messages are made at a few instants inside a radar period, so the table is a handful of entries (a few
// hundred bytes to a few KiB) that stay in cache, neighbouring lanes mostly point at the same entry, and an entry is read once per leg
// and pass -- against a step's several hundred dependent float64 operations.  tools/smooth_cost.py --ais measures what it costs.
//
// Workspace: the lengths, then TWO filtered slots per node, [node][slot][element][track]: slot 0 the filtered state at the scan's time
// (what the linear smoother keeps), slot 1 the filtered state at the message's time, written for AIS nodes only.
#include "mht_common.h"
#include "mht_smooth_ais_math.h"

namespace mht {

struct SmoothAisArgs {
    SmoothModel<4> model;     // the plain step's A, Q and the radar update's C, R
    int32_t n, L_max;
    const int32_t* len;       // [n] (in the workspace)
    const double* x_init;     // [4][n]
    const double* P_init;     // [16][n]
    const double* z;          // [L_max][2][n]
    const uint8_t* has_z;     // [L_max][n]
    const uint8_t* kind;      // [L_max][n]
    const double* ais_z;      // [L_max][4][n]
    const double* ais_r;      // [L_max][n]
    const int32_t* leg;       // [L_max][n]
    const double* legs;       // [n_legs][52]
    double* xs;               // [L_max][4][n]
    double* Ps;               // [L_max][10][n] or null
    double* xf;               // workspace [L_max][2][4][n]
    double* Pf;               // workspace [L_max][2][10][n]
};

// One lane's track, forward and backward
template <bool COV>
__global__ void __launch_bounds__(64) smooth_ais_kernel(const SmoothAisArgs a) {
    constexpr int N = 4, NS = 10;
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
    // forward: node 0 is the initial state; node k >= 1 steps one period or over its two legs and, with a plot, updates
    for (int k = 0; k < len; ++k) {
        if (k > 0) {
            if (a.kind[(size_t)k * n + t] >= 2) {
                const double* entry = a.legs + (size_t)a.leg[(size_t)k * n + t] * SMOOTH_AIS_LEG_DOUBLES;
                double m[N], xm[N], Pm[NS];
#pragma unroll
                for (int i = 0; i < N; ++i) m[i] = a.ais_z[((size_t)k * N + i) * n + t];
                smooth_ais_forward(entry, m, a.ais_r[(size_t)k * n + t], x, P, xm, Pm);
#pragma unroll
                for (int i = 0; i < N; ++i) a.xf[(((size_t)k * 2 + 1) * N + i) * n + t] = xm[i];
#pragma unroll
                for (int e = 0; e < NS; ++e) a.Pf[(((size_t)k * 2 + 1) * NS + e) * n + t] = Pm[e];
            } else {
                double xp[N], AP[N * N], Pp[NS];
                smooth_predict<N>(a.model, x, P, xp, AP, Pp);
#pragma unroll
                for (int i = 0; i < N; ++i) x[i] = xp[i];
#pragma unroll
                for (int e = 0; e < NS; ++e) P[e] = Pp[e];
            }
            if (a.has_z[(size_t)k * n + t]) smooth_update<N>(a.model, a.z[((size_t)k * 2) * n + t], a.z[((size_t)k * 2 + 1) * n + t], x, P);
        }
        if (k < len - 1) {      // (the last node's filtered state is its smoothed state: it stays in registers)
#pragma unroll
            for (int i = 0; i < N; ++i) a.xf[(((size_t)k * 2) * N + i) * n + t] = x[i];
#pragma unroll
            for (int e = 0; e < NS; ++e) a.Pf[(((size_t)k * 2) * NS + e) * n + t] = P[e];
        }
    }
    // backward: (x, P) is the smoothed state of node k + 1 on entry of a step and of node k afterwards
    for (int k = len - 1; k >= 0; --k) {
        if (k < len - 1) {
            double xf[N], Pf[NS];
#pragma unroll
            for (int i = 0; i < N; ++i) xf[i] = a.xf[(((size_t)k * 2) * N + i) * n + t];
#pragma unroll
            for (int e = 0; e < NS; ++e) Pf[e] = a.Pf[(((size_t)k * 2) * NS + e) * n + t];
            if (a.kind[(size_t)(k + 1) * n + t] >= 2) {
                const double* entry = a.legs + (size_t)a.leg[(size_t)(k + 1) * n + t] * SMOOTH_AIS_LEG_DOUBLES;
                double xm[N], Pm[NS];
#pragma unroll
                for (int i = 0; i < N; ++i) xm[i] = a.xf[(((size_t)(k + 1) * 2 + 1) * N + i) * n + t];
#pragma unroll
                for (int e = 0; e < NS; ++e) Pm[e] = a.Pf[(((size_t)(k + 1) * 2 + 1) * NS + e) * n + t];
                smooth_ais_backward<COV>(entry, xm, Pm, xf, Pf, x, P);
            } else {
                smooth_backward<N, COV>(a.model, xf, Pf, x, P);
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i) a.xs[((size_t)k * N + i) * n + t] = x[i];
        if (COV) {
#pragma unroll
            for (int e = 0; e < NS; ++e) a.Ps[((size_t)k * NS + e) * n + t] = P[e];
        }
    }
}

static size_t smooth_ais_len_bytes(int32_t n_tracks) { return (((size_t)n_tracks * 4 + 255) / 256) * 256; }

static size_t smooth_ais_work_bytes(int32_t n_tracks, int32_t L_max) {
    return smooth_ais_len_bytes(n_tracks) + (size_t)L_max * 2 * (4 + 10) * (size_t)n_tracks * 8;
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_smooth_ais_work_bytes(int32_t n_tracks, int32_t L_max) {
    if (n_tracks < 0 || L_max < 0) return 0;
    return smooth_ais_work_bytes(n_tracks, L_max);
}

extern "C" int mht_smooth_tracks_ais(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                     const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                                     const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, int32_t n_legs,
                                     double* xs, double* Ps, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx && model, "mht_smooth_tracks_ais: null argument");
    MHT_REQUIRE(model->nx == 4, "mht_smooth_tracks_ais: AIS messages report four states (got nx = %d)", model->nx);
    MHT_REQUIRE(model->transition == 0, "mht_smooth_tracks_ais: a state-dependent transition (%d) has no AIS-aware smoother", model->transition);
    MHT_REQUIRE(model->A && model->Q && model->C && model->R, "mht_smooth_tracks_ais: null model matrix");
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 1 && n_legs >= 0, "mht_smooth_tracks_ais: bad size (n_tracks %d, L_max %d, n_legs %d)", n_tracks, L_max, n_legs);
    if (n_tracks == 0) return MHT_OK;
    MHT_REQUIRE(len && x_init && P_init && z && has_z && kind && ais_z && ais_r && leg && (legs || n_legs == 0) && xs && work,
                "mht_smooth_tracks_ais: null array");
    for (int32_t t = 0; t < n_tracks; ++t)
        MHT_REQUIRE(len[t] >= 1 && len[t] <= L_max, "mht_smooth_tracks_ais: track %d has length %d (1 .. L_max = %d)", t, len[t], L_max);
    const size_t need = smooth_ais_work_bytes(n_tracks, L_max);
    if (work_bytes < need) {
        set_error("mht_smooth_tracks_ais: the workspace has %zu bytes, %zu are needed (mht_smooth_ais_work_bytes)", work_bytes, need);
        return MHT_E_CAPACITY;
    }
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    SmoothAisArgs a = {};
    for (int i = 0; i < 16; ++i) a.model.A[i] = (double)model->A[i];
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j) a.model.Q[sym_idx(4, i, j)] = (double)model->Q[i * 4 + j];
    for (int i = 0; i < 8; ++i) a.model.C[i] = (double)model->C[i];
    a.model.R[0] = (double)model->R[0]; a.model.R[1] = (double)model->R[1]; a.model.R[2] = (double)model->R[3];
    a.n = n_tracks; a.L_max = L_max;
    a.x_init = x_init; a.P_init = P_init; a.z = z; a.has_z = has_z; a.kind = kind; a.ais_z = ais_z; a.ais_r = ais_r; a.leg = leg; a.legs = legs;
    a.xs = xs; a.Ps = Ps;
    // the lengths go to the front of the workspace, the filtered means and covariances behind them; then one launch and a wait
    char* q = static_cast<char*>(work);
    a.len = reinterpret_cast<const int32_t*>(q); q += smooth_ais_len_bytes(n_tracks);
    a.xf = reinterpret_cast<double*>(q); q += (size_t)L_max * 2 * 4 * (size_t)n_tracks * 8;
    a.Pf = reinterpret_cast<double*>(q);
    MHT_HIP_CHECK(hipMemcpyAsync(work, len, (size_t)n_tracks * 4, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((n_tracks + 63) / 64), block(64);
    if (Ps) hipLaunchKernelGGL((smooth_ais_kernel<true>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((smooth_ais_kernel<false>), grid, block, 0, ctx->stream, a);
    MHT_HIP_CHECK(hipGetLastError());
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
