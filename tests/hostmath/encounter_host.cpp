// TEST-ONLY host build of csrc/mht_encounter.h: encounter_propagate and encounter_cell themselves -- what a lane of the kernels of
// mht_encounter.hip runs per entry and per cell -- compiled for the CPU and run over a batch in the seam's own track-minor layouts, so
// that the figures, their indexing and their NaN rules are checked against tests/encounter_ref.py without a GPU
// (tests/test_encounter_cpu.py).
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
#include "../../pymht_amd/csrc/mht_encounter.h"

using namespace mht;

template <int N>
static void run(int32_t n, int32_t first, int32_t K, double dt, double R, const double* Phi, const double* Q, const double* x,
                const double* P, double* out, double* work) {
    EncounterModel<N> m;
    for (int c = 0; c < N * N; ++c) {
        m.Phi[c] = Phi[c];
        m.Q[c] = Q[c];
    }
    double* pos = work;
    double* S = work + (size_t)2 * (size_t)(K + 1) * (size_t)n;
    for (int t = 0; t < n; ++t) encounter_propagate<N>(m, x, P, n, K, t, pos, S);
    for (int i = 0; i < first; ++i)
        for (int j = 0; j < n; ++j) encounter_cell(pos, S, n, first, K, dt, R, i, j, out);
}

// The seam's arguments on host arrays: x [nx][n], P [nx (nx + 1) / 2][n], out [5][first][n], work [5 (K + 1) n] doubles (on return
// pos [K + 1][2][n] and behind it S [K + 1][3][n]).  Returns 0, or -1 where the seam refuses (nothing written).
extern "C" int encounters_host(int32_t nx, int32_t n, int32_t first, int32_t K, double dt, double R, const double* Phi, const double* Q,
                               const double* x, const double* P, double* out, double* work) {
    if ((nx != 4 && nx != 6) || K < 1 || K > ENCOUNTER_MAX_STEPS || !(R > 0.0) || !(dt > 0.0) || n < 0 || first < 0 || first > n) return -1;
    if (nx == 4) run<4>(n, first, K, dt, R, Phi, Q, x, P, out, work);
    else run<6>(n, first, K, dt, R, Phi, Q, x, P, out, work);
    return 0;
}

// encounter_pc on m cases: d [m][2], Sigma [m][3] (xx, xy, yy; positive definite), R [m] -> pc [m]
extern "C" void encounter_pc_host(int32_t m, const double* d, const double* Sigma, const double* R, double* pc) {
    for (int c = 0; c < m; ++c) {
        const double a = Sigma[3 * c], b = Sigma[3 * c + 1], cc = Sigma[3 * c + 2];
        pc[c] = encounter_pc(d[2 * c], d[2 * c + 1], a, b, cc, a * cc - b * b, R[c]);
    }
}

// The rule's table, for the test that holds it to 20 digits: x [32], w [32]
extern "C" void encounter_rule_host(double* x, double* w) {
    for (int q = 0; q < 32; ++q) {
        x[q] = EncounterRule::x[q];
        w[q] = EncounterRule::w[q];
    }
}
