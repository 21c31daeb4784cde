// TEST-ONLY host build of csrc/mht_trial.h: trial_track, trial_candidate, trial_cell and the fold themselves -- what a lane of the
// kernels of mht_trial.hip runs per track, per candidate and per cell -- compiled for the CPU and run over a batch in the seam's own
// layouts, with the lanes of a tile and the tiles of a row as loops, so that the candidate path, the table, its indexing, the NaN rules
// and the summary are checked against tests/trial_ref.py without a GPU (tests/test_trial_cpu.py).
#include <cmath>
#include <cstdint>
#include <cstddef>
using std::fma;
using std::sqrt;
using std::fabs;
using std::fmin;
using std::fmax;
using std::exp;
using std::erfc;
using std::sin;
using std::cos;
using std::asin;
#include "../../pymht_amd/csrc/mht_trial.h"

using namespace mht;

static bool finite_or_nan(double v) { return v != v || v - v == 0.0; }

template <int N>
static void tracks(int32_t n, int32_t G, int32_t K, const double* Phi, const double* Q, const double* x, const double* P, double* xs, double* Ps,
                   double* pos, double* S) {
    EncounterModel<N> m;
    for (int c = 0; c < N * N; ++c) {
        m.Phi[c] = Phi[c];
        m.Q[c] = Q[c];
    }
    for (int t = 0; t < n; ++t) trial_track<N>(m, x, P, n, n + G, K, t, xs, Ps, pos, S);
}

// The doubles of the twin's work buffer: pos [K + 1][2][n + G], S [K + 1][3][n + G], partials [4][G][tiles per row], and the staging
// xs [6][n + G], Ps [21][n + G]
extern "C" int64_t trial_host_work_doubles(int32_t n, int32_t G, int32_t K) {
    const int64_t nt = (int64_t)n + G, chunks = ((int64_t)n + TRIAL_TILE - 1) / TRIAL_TILE;
    return 5 * (int64_t)(K + 1) * nt + TRIAL_SUMMARY * (int64_t)G * chunks + 27 * nt;
}

// The seam's arguments on host arrays: x [nx][n], P [nx (nx + 1) / 2][n], own [4], Sown [3], cand [G][3], out [5][G][n], summary [4][G],
// work as above.  Returns 0, or -1 where the seam refuses (nothing written).
extern "C" int trial_manoeuvres_host(int32_t nx, int32_t n, int32_t G, int32_t K, double dt, double R, const double* Phi, const double* Q,
                                     const double* x, const double* P, const double* own, const double* Sown, double w, const double* cand,
                                     double* out, double* summary, double* work) {
    if ((nx != 4 && nx != 6) || K < 1 || K > ENCOUNTER_MAX_STEPS || G < 1 || G > TRIAL_MAX_CANDIDATES || n < 0) return -1;
    if (!(R > 0.0) || !(dt > 0.0) || !(w > 0.0) || R - R != 0.0 || dt - dt != 0.0 || w - w != 0.0) return -1;
    if (n == 0) return 0;
    for (int c = 0; c < 4; ++c)
        if (!finite_or_nan(own[c])) return -1;
    for (int c = 0; c < 3; ++c)
        if (!finite_or_nan(Sown[c])) return -1;
    for (int c = 0; c < 3 * G; ++c)
        if (!finite_or_nan(cand[c])) return -1;
    for (int g = 0; g < G; ++g)
        if (fabs(cand[3 * g]) > 3.14159265358979323846 || cand[3 * g + 1] < 0.0 || cand[3 * g + 2] < 0.0) return -1;
    const size_t nt = (size_t)n + (size_t)G, steps = (size_t)(K + 1), chunks = ((size_t)n + TRIAL_TILE - 1) / TRIAL_TILE;
    double* pos = work;
    double* S = pos + 2 * steps * nt;
    double* partials = S + 3 * steps * nt;
    double* xs = partials + (size_t)TRIAL_SUMMARY * (size_t)G * chunks;
    double* Ps = xs + 6 * nt;
    if (nx == 4) tracks<4>(n, G, K, Phi, Q, x, P, xs, Ps, pos, S);
    else tracks<6>(n, G, K, Phi, Q, x, P, xs, Ps, pos, S);
    const TrialOwn o = {{own[0], own[1]}, {own[2], own[3]}, {Sown[0], Sown[1], Sown[2]}, w};
    for (int g = 0; g < G; ++g) trial_candidate(o, cand[3 * g], cand[3 * g + 1], cand[3 * g + 2], n + G, K, dt, n + g, pos, S);
    const size_t tiles = (size_t)G * chunks;
    for (size_t tile = 0; tile < tiles; ++tile) {      // a workgroup's tile: the lanes in turn
        const int g = (int)(tile / chunks);
        const size_t chunk = tile % chunks;
        TrialBest t = trial_none();
        for (int lane = 0; lane < TRIAL_TILE; ++lane) {
            const size_t j = chunk * TRIAL_TILE + lane;
            TrialBest b = trial_none();
            if (j < (size_t)n) b = trial_cell(pos, S, n, G, K, dt, R, g, (int)j, out);
            trial_fold(t, b);
        }
        trial_store(t, partials + (size_t)g * chunks + chunk, tiles);
    }
    for (int g = 0; g < G; ++g) {      // a wavefront's candidate: the tiles of its row in index order
        TrialBest b = trial_none();
        for (size_t c = 0; c < chunks; ++c) trial_fold(b, trial_load(partials + (size_t)g * chunks + c, tiles));
        trial_store(b, summary + g, (size_t)G);
    }
    return 0;
}

// The fold of m figures in the order given and in the reverse order: fig [m][2] (pc, dcpa) -> res [2][4] as trial_store writes them.
// The two must be the same bits: the fold's order is total.
extern "C" void trial_fold_host(int32_t m, const double* fig, double* res) {
    TrialBest a = trial_none(), b = trial_none();
    for (int j = 0; j < m; ++j) trial_fold(a, trial_cell_best(fig[2 * j], fig[2 * j + 1], j));
    for (int j = m - 1; j >= 0; --j) trial_fold(b, trial_cell_best(fig[2 * j], fig[2 * j + 1], j));
    trial_store(a, res, 1);
    trial_store(b, res + 4, 1);
}
