// mht_nees_nodes (include/mht_amd.h): the estimation error and its NEES at every node of a batch of filtered or smoothed track histories
// against ground truth -- per cell one factorisation of P and one forward substitution (nees_eval, mht_nees.h), which give the position,
// position-and-velocity and full-state NEES together.  The inputs are read where mht_filter_tracks* and mht_smooth_tracks* wrote them,
// in their track-minor layouts.
//
// Mapping: ONE CELL PER LANE, the cells numbered k * n + t with the track index fastest, so that the 64 lanes of a wavefront read 64
// consecutive doubles with every load of x, P and truth and write 64 consecutive doubles with every store (a wavefront that straddles
// the end of a row reads two runs).  The cells do not depend on each other: no LDS, no atomic, no barrier, and every matrix in registers
// (tests/test_nees_resources.py).  A STREAMING kernel: a cell reads 2 N + N (N + 1) / 2 doubles and a flag and writes N + 3 doubles --
// 201 bytes at four states, 337 at six -- against a few dozen dependent float64 operations, so workgroups of 256 lanes, at most 2048
// of them, stride over the cells: enough wavefronts in flight to cover the loads' latency, and no tail of small launches.
#include "mht_common.h"
#include "mht_nees.h"

namespace mht {

constexpr int NEES_THREADS = 256;
constexpr int NEES_MAX_BLOCKS = 2048;

template <int N>
__global__ void __launch_bounds__(NEES_THREADS) nees_kernel(const NeesArgs a) {
    const size_t cells = (size_t)a.L_max * (size_t)a.n;
    for (size_t c = (size_t)blockIdx.x * NEES_THREADS + threadIdx.x; c < cells; c += (size_t)gridDim.x * NEES_THREADS)
        nees_cell<N>(a, (int)(c / (size_t)a.n), (int)(c % (size_t)a.n));
}

}  // namespace mht

using namespace mht;

extern "C" int mht_nees_nodes(mht_ctx* ctx, int32_t nx, int32_t n_tracks, int32_t L_max, int32_t D, const double* x, const double* P,
                              const double* truth, const uint8_t* present, double* out) {
    MHT_REQUIRE(ctx, "mht_nees_nodes: null context");
    MHT_REQUIRE(nx == 4 || nx == 6, "mht_nees_nodes: nx must be 4 or 6 (got %d)", nx);
    MHT_REQUIRE(D == 2 || D == 4 || D == nx, "mht_nees_nodes: D must be 2, 4 or nx = %d (got %d)", nx, D);
    MHT_REQUIRE(n_tracks >= 0 && L_max >= 0, "mht_nees_nodes: bad size (n_tracks %d, L_max %d)", n_tracks, L_max);
    if (n_tracks == 0 || L_max == 0) return MHT_OK;
    MHT_REQUIRE(x && P && truth && present && out, "mht_nees_nodes: null array");
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    const NeesArgs a = {n_tracks, L_max, D, x, P, truth, present, out};
    const size_t cells = (size_t)L_max * (size_t)n_tracks, blocks = (cells + NEES_THREADS - 1) / NEES_THREADS;
    const dim3 grid((unsigned)(blocks < (size_t)NEES_MAX_BLOCKS ? blocks : (size_t)NEES_MAX_BLOCKS));
    const int rc = nx == 4 ? launch_kernel(ctx, K_SMOOTH_SCORE, nees_kernel<4>, grid, dim3(NEES_THREADS), 0, false, a)
                           : launch_kernel(ctx, K_SMOOTH_SCORE, nees_kernel<6>, grid, dim3(NEES_THREADS), 0, false, a);
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
