// TEST-ONLY host build of csrc/mht_smooth_em.h: smooth_em_walk itself -- the n_iter + 1 walks a lane of smooth_em_kernel runs, one launch
// each, with the math headers under them -- compiled for the CPU and run one track at a time (n = 1, t = 0: the track-minor layout is
// then plain [node][element]), so that the EM walk, its workspace indexing and its arithmetic are checked against tests/smooth_em_ref.py
// without a GPU (tests/test_smooth_em_cpu.py).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
using std::fma;
using std::sqrt;
using std::fabs;
using std::sin;
using std::cos;
#include "../../pymht_amd/csrc/mht_smooth_em.h"

using namespace mht;

template <int N>
static void run(const double* A, const double* Q, const double* C, const double* R, int32_t L, const double* x_init, const double* P_init,
                const double* z, const uint8_t* has_z, int32_t n_iter, double* xs, double* Ps, double* Q_out, double* R_out) {
    constexpr int NS = N * (N + 1) / 2;
    LinearSteps<N> steps;
    std::copy(A, A + N * N, steps.model.A);
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j) steps.model.Q[sym_idx(N, i, j)] = Q[i * N + j];
    std::copy(C, C + 2 * N, steps.model.C);
    steps.model.R[0] = R[0]; steps.model.R[1] = R[1]; steps.model.R[2] = R[3];
    std::vector<double> xf((size_t)L * N), Pf((size_t)L * NS), track(smooth_em_track_doubles(N));
    SmoothEmArgs<N> a = {};
    a.s = {steps, 1, L, &L, x_init, P_init, z, has_z, xs, Ps, xf.data(), Pf.data()};
    a.theta = track.data();
    a.sq = a.theta + N + 2 * NS + 3;
    a.pn = a.sq + NS + 4;
    a.Q_out = Q_out; a.R_out = R_out;
    smooth_em_walk<N>(a, 0, n_iter);
}

// nx = 4 or 6; A [nx][nx], Q [nx][nx], C [2][nx], R [4] row-major float64; one track of L nodes: x_init [nx], P_init [nx][nx], z [L][2],
// has_z [L]; xs [L][nx], Ps [L][nx (nx + 1) / 2] packed or null, Q_out [nx (nx + 1) / 2] packed, R_out [3]
extern "C" void smooth_em_host(int32_t nx, const double* A, const double* Q, const double* C, const double* R, int32_t L, const double* x_init,
                               const double* P_init, const double* z, const uint8_t* has_z, int32_t n_iter, double* xs, double* Ps,
                               double* Q_out, double* R_out) {
    if (nx == 4) run<4>(A, Q, C, R, L, x_init, P_init, z, has_z, n_iter, xs, Ps, Q_out, R_out);
    else run<6>(A, Q, C, R, L, x_init, P_init, z, has_z, n_iter, xs, Ps, Q_out, R_out);
}
