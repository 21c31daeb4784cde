// mht_score_tracks_grid, mht_score_tracks_ct_grid (include/mht_amd.h): the score seams of mht_smooth_score.hip under a grid of candidate
// (Q, R) in one launch -- the likelihood surface the noise levels are tuned over.  One (track, candidate) per lane: blockIdx.x walks the
// tracks 64 to a workgroup as the score kernels do, blockIdx.y is the candidate, so a wavefront's candidate is one and its row of the
// table (mht_smooth_score_grid.h) is read through a wavefront-uniform address.  A batch of a few hundred tracks is a handful of
// wavefronts; the candidates are what fills the chip.  The workspace holds the lengths and the table; no LDS, no scratch; no lane
// touches anything of another (nobs, which no candidate changes, is written by candidate 0's lanes).
#include <vector>

#include "mht_common.h"
#include "mht_smooth_score_grid.h"
#include "mht_smooth_seam.h"

namespace mht {

constexpr int32_t SCORE_GRID_MAX_CAND = 4096;

template <int N, typename Steps>
__global__ void __launch_bounds__(64) smooth_score_grid_kernel(const ScoreGridArgs<N, Steps> a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < a.s.n) smooth_score_grid_walk<N>(a, t, (int)blockIdx.y);
}

static size_t score_grid_table_bytes(int32_t nx, int32_t n_cand) {
    return (((size_t)n_cand * smooth_score_grid_row(nx) * 8 + 255) / 256) * 256;
}

static size_t score_grid_work_bytes(int32_t nx, int32_t n_tracks, int32_t n_cand) {      // the lengths, then the table
    return smooth_len_bytes(n_tracks) + score_grid_table_bytes(nx, n_cand);
}

struct ScoreGridBatch : TrackBatch {
    int32_t n_cand;
    const double *Q_cand, *R_cand;
    double *ll, *nis;
    int32_t* nobs;
};

// run_score (mht_smooth_score.hip) with the table behind the lengths: an empty batch is done; any other is checked, the lengths and
// the packed candidates go to the workspace; then one launch and a wait
template <int N, typename Steps>
static int run_score_grid(mht_ctx* ctx, const char* seam, const Steps& steps, const ScoreGridBatch& b) {
    constexpr int NS = N * (N + 1) / 2;
    MHT_REQUIRE(b.n_cand >= 1 && b.n_cand <= SCORE_GRID_MAX_CAND, "%s: n_cand must be 1 .. %d (got %d)", seam, SCORE_GRID_MAX_CAND, b.n_cand);
    if (b.n == 0) return MHT_OK;
    const int rc = check_batch(seam, b, b.Q_cand && b.R_cand && b.ll && b.nis && b.nobs, score_grid_work_bytes(N, b.n, b.n_cand),
                               "mht_score_grid_work_bytes", MHT_E_INVALID);
    if (rc != MHT_OK) return rc;
    std::vector<double> table((size_t)b.n_cand * (NS + 3));
    for (int32_t g = 0; g < b.n_cand; ++g) {
        double* row = table.data() + (size_t)g * (NS + 3);
        const double *Q = b.Q_cand + (size_t)g * N * N, *R = b.R_cand + (size_t)g * 4;
        for (int i = 0; i < N; ++i)
            for (int j = i; j < N; ++j) row[sym_idx(N, i, j)] = Q[i * N + j];
        row[NS] = R[0]; row[NS + 1] = R[1]; row[NS + 2] = R[3];
    }
    char* w = static_cast<char*>(b.work);
    ScoreGridArgs<N, Steps> a = {};
    a.s.steps = steps;
    a.s.n = b.n; a.s.L_max = b.L_max;
    a.s.len = reinterpret_cast<const int32_t*>(w);
    a.s.x_init = b.x_init; a.s.P_init = b.P_init; a.s.z = b.z; a.s.has_z = b.has_z;
    a.s.ll = b.ll; a.s.nis = b.nis; a.s.nobs = b.nobs;
    a.cand = reinterpret_cast<const double*>(w + smooth_len_bytes(b.n));
    a.n_cand = b.n_cand;
    return run_over_lengths(ctx, seam, b, table.data(), table.size(), [&] {
        return launch_kernel(ctx, K_SMOOTH_SCORE, smooth_score_grid_kernel<N, Steps>, dim3((b.n + 63) / 64, b.n_cand), dim3(64), 0, false, a);
    });
}

}  // namespace mht

using namespace mht;

extern "C" size_t mht_score_grid_work_bytes(int32_t nx, int32_t n_tracks, int32_t L_max, int32_t n_cand) {
    if ((nx != 4 && nx != 6) || n_tracks < 0 || L_max < 0 || n_cand < 1 || n_cand > SCORE_GRID_MAX_CAND) return 0;
    return score_grid_work_bytes(nx, n_tracks, n_cand);
}

// (the steps carry the model's Q and R too: every walk overwrites them with its candidate's)
extern "C" int mht_score_tracks_grid(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                     const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_cand,
                                     const double* Q_cand, const double* R_cand, double* ll_out, double* nis_out, int32_t* nobs_out, void* work,
                                     size_t work_bytes) {
    const char* seam = "mht_score_tracks_grid";
    const int rc = check_linear(seam, ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const ScoreGridBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, n_cand, Q_cand, R_cand, ll_out, nis_out, nobs_out};
    return model->nx == 4 ? run_score_grid<4>(ctx, seam, linear_steps<4>(model), b) : run_score_grid<6>(ctx, seam, linear_steps<6>(model), b);
}

extern "C" int mht_score_tracks_ct_grid(mht_ctx* ctx, const mht_model_x* model, int32_t n_tracks, int32_t L_max, const int32_t* len,
                                        const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t n_cand,
                                        const double* Q_cand, const double* R_cand, double* ll_out, double* nis_out, int32_t* nobs_out,
                                        void* work, size_t work_bytes) {
    const int rc = check_ct("mht_score_tracks_ct_grid", ctx, model, n_tracks, L_max);
    if (rc != MHT_OK) return rc;
    const ScoreGridBatch b = {{n_tracks, L_max, len, x_init, P_init, z, has_z, work, work_bytes}, n_cand, Q_cand, R_cand, ll_out, nis_out, nobs_out};
    return run_score_grid<6>(ctx, "mht_score_tracks_ct_grid", ct_steps(model), b);
}
