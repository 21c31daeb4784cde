// TEST-ONLY host build of csrc/mht_smooth_filter.h: smooth_filter_walk itself -- the code a lane of the kernels of mht_smooth_filter.hip
// runs, with the walk and math headers under it -- compiled for the CPU and run one track at a time (n = 1, t = 0: the track-minor
// layout is then plain [node][element]), so that the filter walk, its indexing and its arithmetic are checked against
// tests/filter_ref.py, and its last node against tests/hostmath/smooth_host.cpp, without a GPU (tests/test_filter_cpu.py).  The host's
// libm stands in for the device's sin / cos.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
using std::fma;
using std::sqrt;
using std::fabs;
using std::sin;
using std::cos;
#include "../../pymht_amd/csrc/mht_smooth_filter.h"

using namespace mht;

template <int N, typename Model>
static void fill(Model& m, const double* Q, const double* C, const double* R) {
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j) m.Q[sym_idx(N, i, j)] = Q[i * N + j];
    for (int i = 0; i < 2 * N; ++i) m.C[i] = C[i];
    m.R[0] = R[0]; m.R[1] = R[1]; m.R[2] = R[3];
}

// xf [L_max][N], Pf [L_max][N (N + 1) / 2]: every cell is written by the walk
template <int N, typename Steps>
static void walk(const Steps& steps, int32_t L, int32_t L_max, const double* x_init, const double* P_init, const double* z, const uint8_t* has_z,
                 double* xf, double* Pf) {
    const FilterArgs<N, Steps> a = {steps, 1, L_max, &L, x_init, P_init, z, has_z, xf, Pf};
    smooth_filter_walk<N>(a, 0);
}

// nx = 4 or 6; A [nx][nx], Q [nx][nx], C [2][nx], R [4] row-major float64; one track of L nodes in arrays of L_max rows: x_init [nx],
// P_init [nx][nx], z [L_max][2], has_z [L_max]
extern "C" void filter_lin_host(int32_t nx, const double* A, const double* Q, const double* C, const double* R, int32_t L, int32_t L_max,
                                const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, double* xf, double* Pf) {
    if (nx == 4) {
        LinearSteps<4> s;
        std::copy(A, A + 16, s.model.A);
        fill<4>(s.model, Q, C, R);
        walk<4>(s, L, L_max, x_init, P_init, z, has_z, xf, Pf);
    } else {
        LinearSteps<6> s;
        std::copy(A, A + 36, s.model.A);
        fill<6>(s.model, Q, C, R);
        walk<6>(s, L, L_max, x_init, P_init, z, has_z, xf, Pf);
    }
}

extern "C" void filter_ct_host(double T, const double* Q, const double* C, const double* R, int32_t L, int32_t L_max, const double* x_init,
                               const double* P_init, const double* z, const uint8_t* has_z, double* xf, double* Pf) {
    ConstantTurnSteps s;
    fill<6>(s.model, Q, C, R);
    s.model.T = T;
    walk<6>(s, L, L_max, x_init, P_init, z, has_z, xf, Pf);
}

extern "C" void filter_ais_host(const double* A, const double* Q, const double* C, const double* R, int32_t L, int32_t L_max,
                                const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind,
                                const double* ais_z, const double* ais_r, const int32_t* leg, const double* legs, double* xf, double* Pf) {
    AisSteps s;
    std::copy(A, A + 16, s.model.A);
    fill<4>(s.model, Q, C, R);
    s.kind = kind; s.ais_z = ais_z; s.ais_r = ais_r; s.leg = leg; s.legs = legs;
    walk<4>(s, L, L_max, x_init, P_init, z, has_z, xf, Pf);
}
