// mht_encounters (include/mht_amd.h): which tracks come close to each other over the next minutes -- per pair of entries the closest
// point of approach, the smallest Mahalanobis distance and the largest probability of being within a safety radius, over a horizon of
// K steps of the tracker's own model (the figures: mht_encounter.h).  Two launches on the context's stream:
//
// encounter_propagate_kernel<N>: ONE ENTRY PER LANE, x, P and the product Phi P in registers, Phi and Q wave-uniform kernel arguments;
// per step it stores the position and its packed 2 x 2 covariance into the work buffer, pos [K + 1][2][n] and S [K + 1][3][n],
// track-minor, so the 64 lanes of a wavefront write 64 consecutive doubles with every store.
//
// encounter_pair_kernel: ONE CELL (i, j) PER LANE of the [first][n] table, j fastest.  A workgroup of 256 lanes takes a TILE, row i and
// 256 consecutive columns, and strides over the tiles: i is the same in every lane of the workgroup, so row i's trajectory is read
// through wave-uniform loads (ten doubles a step, one address for the wavefront) and column j's through coalesced ones; the cells do
// not depend on each other -- no LDS, no atomic, no barrier.  A tile left of the diagonal only writes its NaN.  The kernel is bound by
// float64 transcendentals, not by memory: a cell whose pc_k is not zero by the rule evaluates 64 nodes of sin, cos, exp and two erfc
// per step, against 80 bytes loaded.  Every cell of every figure is written; the five stores of a wavefront are contiguous runs.
#include "mht_common.h"
#include "mht_encounter.h"

namespace mht {

constexpr int ENCOUNTER_THREADS = 256;
constexpr int ENCOUNTER_MAX_BLOCKS = 2048;

template <int N>
struct EncounterPropagateArgs {
    EncounterModel<N> m;
    int32_t n, K;
    const double* x;      // [N][n]
    const double* P;      // [N(N+1)/2][n]
    double* pos;          // [K + 1][2][n]
    double* S;            // [K + 1][3][n]
};

struct EncounterPairArgs {
    int32_t n, first, K;
    double dt, R;
    const double* pos;
    const double* S;
    double* out;          // [5][first][n]
};

template <int N>
__global__ void __launch_bounds__(ENCOUNTER_THREADS) encounter_propagate_kernel(const EncounterPropagateArgs<N> a) {
    for (size_t t = (size_t)blockIdx.x * ENCOUNTER_THREADS + threadIdx.x; t < (size_t)a.n; t += (size_t)gridDim.x * ENCOUNTER_THREADS)
        encounter_propagate<N>(a.m, a.x, a.P, a.n, a.K, (int)t, a.pos, a.S);
}

__global__ void __launch_bounds__(ENCOUNTER_THREADS) encounter_pair_kernel(const EncounterPairArgs a) {
    const size_t chunks = ((size_t)a.n + ENCOUNTER_THREADS - 1) / ENCOUNTER_THREADS;
    const size_t tiles = (size_t)a.first * chunks;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int i = (int)(tile / chunks);
        const size_t j = (tile % chunks) * ENCOUNTER_THREADS + threadIdx.x;
        if (j < (size_t)a.n) encounter_cell(a.pos, a.S, a.n, a.first, a.K, a.dt, a.R, i, (int)j, a.out);
    }
}

static size_t encounter_doubles(int32_t n, int32_t K) { return (size_t)5 * (size_t)(K + 1) * (size_t)n; }

template <int N>
static int encounter_run(mht_ctx* ctx, int32_t n, int32_t first, int32_t K, double dt, double R, const double* Phi, const double* Q,
                         const double* x, const double* P, double* out, double* work) {
    EncounterPropagateArgs<N> pa;
    for (int c = 0; c < N * N; ++c) {
        pa.m.Phi[c] = Phi[c];
        pa.m.Q[c] = Q[c];
    }
    pa.n = n;
    pa.K = K;
    pa.x = x;
    pa.P = P;
    pa.pos = work;
    pa.S = work + (size_t)2 * (size_t)(K + 1) * (size_t)n;
    const size_t blocks = ((size_t)n + ENCOUNTER_THREADS - 1) / ENCOUNTER_THREADS;
    const dim3 grid((unsigned)(blocks < (size_t)ENCOUNTER_MAX_BLOCKS ? blocks : (size_t)ENCOUNTER_MAX_BLOCKS));
    int rc = launch_kernel(ctx, K_SMOOTH_SCORE, encounter_propagate_kernel<N>, grid, dim3(ENCOUNTER_THREADS), 0, false, pa);
    if (rc != MHT_OK) return rc;
    const EncounterPairArgs qa = {n, first, K, dt, R, pa.pos, pa.S, out};
    const size_t tiles = (size_t)first * blocks;
    const dim3 pgrid((unsigned)(tiles < (size_t)ENCOUNTER_MAX_BLOCKS ? tiles : (size_t)ENCOUNTER_MAX_BLOCKS));
    return launch_kernel(ctx, K_SMOOTH_SCORE, encounter_pair_kernel, pgrid, dim3(ENCOUNTER_THREADS), 0, false, qa);
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_encounter_work_bytes(int32_t n, int32_t K) {
    if (n <= 0 || K < 1 || K > ENCOUNTER_MAX_STEPS) return 0;
    return (encounter_doubles(n, K) * sizeof(double) + 255) / 256 * 256;
}

extern "C" int mht_encounters(mht_ctx* ctx, int32_t nx, int32_t n, int32_t first, int32_t K, double dt, double R, const double* Phi,
                              const double* Q, const double* x, const double* P, double* out, void* work, size_t work_bytes) {
    MHT_REQUIRE(ctx, "mht_encounters: null context");
    MHT_REQUIRE(nx == 4 || nx == 6, "mht_encounters: nx must be 4 or 6 (got %d)", nx);
    MHT_REQUIRE(K >= 1 && K <= ENCOUNTER_MAX_STEPS, "mht_encounters: K must be 1 .. %d steps (got %d)", ENCOUNTER_MAX_STEPS, K);
    MHT_REQUIRE(R > 0.0 && dt > 0.0, "mht_encounters: the radius and the step must be positive (R %g, dt %g)", R, dt);
    MHT_REQUIRE(n >= 0 && first >= 0 && first <= n, "mht_encounters: bad size (n %d, first %d: 0 <= first <= n)", n, first);
    if (n == 0 || first == 0) return MHT_OK;
    MHT_REQUIRE(Phi && Q && x && P && out && work, "mht_encounters: null array");
    MHT_REQUIRE(work_bytes >= mht_encounter_work_bytes(n, K), "mht_encounters: the work buffer holds %zu bytes, %zu are needed", work_bytes,
                mht_encounter_work_bytes(n, K));
    MHT_HIP_CHECK(hipSetDevice(ctx->device));
    const int rc = nx == 4 ? encounter_run<4>(ctx, n, first, K, dt, R, Phi, Q, x, P, out, (double*)work)
                           : encounter_run<6>(ctx, n, first, K, dt, R, Phi, Q, x, P, out, (double*)work);
    if (rc != MHT_OK) return rc;
    MHT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHT_OK;
}
