// TEST-ONLY host build of csrc/mht_smooth_score.h: smooth_score_walk and smooth_score_walk_theta themselves -- the code a lane of the
// kernels of mht_smooth_score.hip runs, with the math headers under it -- compiled for the CPU and run one track at a time (n = 1,
// t = 0: the track-minor layout is then plain [node][element]), so that the score walk, its indexing and its arithmetic are checked
// against tests/smooth_score_ref.py without a GPU (tests/test_smooth_score_cpu.py).  The host's libm stands in for the device's
// sin / cos / log.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>
using std::fma;
using std::sqrt;
using std::fabs;
using std::sin;
using std::cos;
using std::log;
#include "../../pymht_amd/csrc/mht_smooth_score.h"

using namespace mht;

template <int N, typename Model>
static void fill(Model& m, const double* Q, const double* C, const double* R) {
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j) m.Q[sym_idx(N, i, j)] = Q[i * N + j];
    for (int i = 0; i < 2 * N; ++i) m.C[i] = C[i];
    m.R[0] = R[0]; m.R[1] = R[1]; m.R[2] = R[3];
}

// out [5]: ll, nis, nObs, nisAis, nAis
template <int N, typename Steps>
static void walk(const Steps& steps, int32_t L, const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, const double* theta,
                 double* out) {
    double ll = -7.0, nis = -7.0, nis_ais = -7.0;
    int32_t nobs = -7, nais = -7;
    const ScoreArgs<N, Steps> a = {steps, 1, L, &L, x_init, P_init, z, has_z, theta, &ll, &nis, &nobs, &nis_ais, &nais};
    if constexpr (std::is_same<Steps, LinearSteps<N>>::value) {
        if (theta) smooth_score_walk_theta<N>(a, 0);
        else smooth_score_walk<N>(a, 0);
    } else {
        smooth_score_walk<N>(a, 0);
    }
    out[0] = ll; out[1] = nis; out[2] = (double)nobs; out[3] = nis_ais; out[4] = (double)nais;
}

// nx = 4 or 6; A [nx][nx], Q [nx][nx], C [2][nx], R [4] row-major float64; one track of L nodes: x_init [nx], P_init [nx][nx], z [L][2],
// has_z [L].  theta: null, or [nx + 2 nx (nx + 1) / 2 + 3] -- x0, P0 packed, Q packed, R (r00, r01, r11) -- which then stands in for
// x_init, P_init, Q and R
extern "C" void smooth_score_lin_host(int32_t nx, const double* A, const double* Q, const double* C, const double* R, int32_t L, const double* x_init,
                                      const double* P_init, const double* z, const uint8_t* has_z, const double* theta, double* out) {
    if (nx == 4) {
        LinearSteps<4> s;
        std::copy(A, A + 16, s.model.A);
        fill<4>(s.model, Q, C, R);
        walk<4>(s, L, x_init, P_init, z, has_z, theta, out);
    } else {
        LinearSteps<6> s;
        std::copy(A, A + 36, s.model.A);
        fill<6>(s.model, Q, C, R);
        walk<6>(s, L, x_init, P_init, z, has_z, theta, out);
    }
}

extern "C" void smooth_score_ct_host(double T, const double* Q, const double* C, const double* R, int32_t L, const double* x_init, const double* P_init,
                                     const double* z, const uint8_t* has_z, double* out) {
    ConstantTurnSteps s;
    fill<6>(s.model, Q, C, R);
    s.model.T = T;
    walk<6>(s, L, x_init, P_init, z, has_z, nullptr, out);
}

extern "C" void smooth_score_ais_host(const double* A, const double* Q, const double* C, const double* R, int32_t L, const double* x_init,
                                      const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind, const double* ais_z,
                                      const double* ais_r, const int32_t* leg, const double* legs, double* out) {
    AisSteps s;
    std::copy(A, A + 16, s.model.A);
    fill<4>(s.model, Q, C, R);
    s.kind = kind; s.ais_z = ais_z; s.ais_r = ais_r; s.leg = leg; s.legs = legs;
    walk<4>(s, L, x_init, P_init, z, has_z, nullptr, out);
}
