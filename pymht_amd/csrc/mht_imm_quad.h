// What the translation units that run a (track, mode) per lane share (mht_imm.hip, mht_imm_smooth.hip): the Lanes policy of a kernel --
// the lane's own mode, the others through the quad -- and the host side of their seams: the batch they are handed, the check of a
// distribution over the modes, the table [modes | Pi | mu0] at the front of the workspace and its size.
#pragma once
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

static size_t imm_table_bytes(int32_t nx, int32_t r) {      // the mode table, Pi, mu0
    return (((size_t)r * (smooth_score_grid_row(nx) + r + 1) * 8 + 255) / 256) * 256;
}

static size_t imm_work_bytes(int32_t nx, int32_t n_tracks, int32_t r) { return smooth_len_bytes(n_tracks) + imm_table_bytes(nx, r); }

struct ImmBatch : TrackBatch {      // with the modes and the outputs
    int32_t r;
    const double *Q, *R, *Pi, *mu0;
    double *mu, *x, *P, *ll;
    int32_t* nobs;
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

// Pi's rows and mu0, checked
static int check_chain(const char* seam, const ImmBatch& b) {
    for (int32_t i = 0; i < b.r; ++i) {
        const int rc = check_distribution(seam, "Pi", i, b.Pi + (size_t)i * b.r, b.r);
        if (rc != MHT_OK) return rc;
    }
    return check_distribution(seam, "mu0", 0, b.mu0, b.r);
}

// What goes behind the lengths in the workspace: the modes [r][NS + 3] (Q packed, R00, R01, R11), Pi [r][r], mu0 [r]
template <int N>
static std::vector<double> imm_table(const ImmBatch& b) {
    constexpr int NS = N * (N + 1) / 2;
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
    return table;
}

// The arguments of a walk over a checked batch whose lengths and table sit at the front of the workspace
template <int N, typename Steps>
static ImmArgs<N, Steps> imm_args(const Steps& steps, const ImmBatch& b) {
    char* w = static_cast<char*>(b.work);
    ImmArgs<N, Steps> a = {};
    a.steps = steps;
    a.n = b.n; a.L_max = b.L_max; a.r = b.r;
    a.len = reinterpret_cast<const int32_t*>(w);
    a.x_init = b.x_init; a.P_init = b.P_init; a.z = b.z; a.has_z = b.has_z;
    a.modes = reinterpret_cast<const double*>(w + smooth_len_bytes(b.n));
    a.Pi = a.modes + (size_t)b.r * (N * (N + 1) / 2 + 3);
    a.mu0 = a.Pi + (size_t)b.r * b.r;
    a.mu = b.mu; a.x = b.x; a.P = b.P; a.ll = b.ll; a.nobs = b.nobs;
    return a;
}

}  // namespace mht
