// TEST-ONLY host build of csrc/mht_imm_smooth.h: imm_smooth_walk itself -- the code the lanes of the kernels of mht_imm_smooth.hip run,
// with the walk and math headers under it -- compiled for the CPU and run one track at a time (n = 1, t = 0: the track-minor layout is
// then plain [node][element]) with the modes IN LOCK STEP, as tests/hostmath/imm_host.cpp runs the filter: this Lanes policy holds all
// r modes and reads an array, and every phase of the walk runs for every mode before the next begins.  The same code, not a copy:
// checked against tests/imm_smooth_ref.py without a GPU (tests/test_imm_smooth_cpu.py).  The host's libm stands in for the device's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
using std::fma;
using std::sqrt;
using std::fabs;
using std::sin;
using std::cos;
using std::log;
using std::exp;
using std::fmax;
#include "../../pymht_amd/csrc/mht_imm_smooth.h"

using namespace mht;

template <int N, typename Steps>
struct HostLanes {
    ImmLane<N, Steps> all[IMM_MAX_MODES];
    int r;
    int count() const { return r; }
    int mode(int q) const { return q; }
    ImmLane<N, Steps>& lane(int q) { return all[q]; }
    double get(int, int i, int e) const { return all[i].s[e]; }
};

template <int N, typename Model>
static void fill(Model& m, const double* C) {
    for (int e = 0; e < N * (N + 1) / 2; ++e) m.Q[e] = 0.0;      // (the modes carry Q and R)
    for (int i = 0; i < 2 * N; ++i) m.C[i] = C[i];
    m.R[0] = m.R[1] = m.R[2] = 0.0;
}

// Q [r][N][N], R [r][2][2], Pi [r][r], mu0 [r]; mus, muf [L_max][r], xs [L_max][N], Ps [L_max][N (N + 1) / 2], out [2]: ll, nObs
template <int N, typename Steps>
static void walk(const Steps& steps, int32_t L, int32_t L_max, const double* x_init, const double* P_init, const double* z, const uint8_t* has_z,
                 int32_t r, const double* Q, const double* R, const double* Pi, const double* mu0, double* mus, double* xs, double* Ps, double* muf,
                 double* out) {
    constexpr int NS = N * (N + 1) / 2;
    std::vector<double> table((size_t)r * (NS + 3));
    for (int g = 0; g < r; ++g) {
        for (int i = 0; i < N; ++i)
            for (int j = i; j < N; ++j) table[(size_t)g * (NS + 3) + sym_idx(N, i, j)] = Q[(size_t)g * N * N + i * N + j];
        table[(size_t)g * (NS + 3) + NS] = R[g * 4]; table[(size_t)g * (NS + 3) + NS + 1] = R[g * 4 + 1]; table[(size_t)g * (NS + 3) + NS + 2] = R[g * 4 + 3];
    }
    std::vector<double> rows((size_t)L_max * r * (N + NS + 1));
    int32_t nobs = 0;
    ImmSmoothArgs<N, Steps> b;
    b.f = {steps, 1, L_max, r, &L, x_init, P_init, z, has_z, table.data(), Pi, mu0, mus, xs, Ps, out, &nobs};
    b.muf = muf;
    b.rows = rows.data();
    HostLanes<N, Steps> lanes;
    lanes.r = r;
    imm_smooth_walk<N, Steps>(b, 0, lanes);
    out[1] = (double)nobs;
}

// nx = 4 or 6; A [nx][nx], C [2][nx] row-major float64; one track of L nodes in arrays of L_max rows, as imm_host.cpp takes it
extern "C" void imm_smooth_lin_host(int32_t nx, const double* A, const double* C, int32_t L, int32_t L_max, const double* x_init,
                                    const double* P_init, const double* z, const uint8_t* has_z, int32_t r, const double* Q, const double* R,
                                    const double* Pi, const double* mu0, double* mus, double* xs, double* Ps, double* muf, double* out) {
    if (nx == 4) {
        LinearSteps<4> s;
        std::copy(A, A + 16, s.model.A);
        fill<4>(s.model, C);
        walk<4>(s, L, L_max, x_init, P_init, z, has_z, r, Q, R, Pi, mu0, mus, xs, Ps, muf, out);
    } else {
        LinearSteps<6> s;
        std::copy(A, A + 36, s.model.A);
        fill<6>(s.model, C);
        walk<6>(s, L, L_max, x_init, P_init, z, has_z, r, Q, R, Pi, mu0, mus, xs, Ps, muf, out);
    }
}

extern "C" void imm_smooth_ct_host(double T, const double* C, int32_t L, int32_t L_max, const double* x_init, const double* P_init,
                                   const double* z, const uint8_t* has_z, int32_t r, const double* Q, const double* R, const double* Pi,
                                   const double* mu0, double* mus, double* xs, double* Ps, double* muf, double* out) {
    ConstantTurnSteps s;
    fill<6>(s.model, C);
    s.model.T = T;
    walk<6>(s, L, L_max, x_init, P_init, z, has_z, r, Q, R, Pi, mu0, mus, xs, Ps, muf, out);
}
