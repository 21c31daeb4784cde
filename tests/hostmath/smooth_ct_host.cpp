// TEST-ONLY host build of csrc/mht_smooth_ct_math.h (and of the mht_smooth_math.h functions it shares with the linear smoother): one track
// walked forward and backward on the CPU with exactly the functions a lane of smooth_rts_ct_kernel calls, so that the structured
// transition, the update and the backward step are checked against tests/smooth_ct_ref.py without a GPU (tests/test_smooth_ct_cpu.py).
// The host's libm stands in for the device's sin / cos.
#include <cmath>
#include <cstdint>
#include <vector>
using std::fma;
using std::sqrt;
using std::fabs;
using std::sin;
using std::cos;
#include "../../pymht_amd/csrc/mht_smooth_ct_math.h"

using namespace mht;

// Q [36], C [12], R [4] row-major float64; z [L][2], has_z [L]; xs [L][6], Ps [L][21] packed.  cov = 0: means only.
extern "C" void smooth_ct_host(double T, const double* Q, const double* C, const double* R, int32_t L, const double* x_init, const double* P_init,
                               const double* z, const uint8_t* has_z, double* xs, double* Ps, int32_t cov) {
    SmoothCtModel m;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) m.Q[sym_idx(6, i, j)] = Q[i * 6 + j];
    for (int i = 0; i < 12; ++i) m.C[i] = C[i];
    m.R[0] = R[0]; m.R[1] = R[1]; m.R[2] = R[3];
    m.T = T;
    double x[6], P[21];
    for (int i = 0; i < 6; ++i) x[i] = x_init[i];
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) P[sym_idx(6, i, j)] = P_init[i * 6 + j];
    std::vector<double> xf((size_t)L * 6), Pf((size_t)L * 21);
    for (int k = 0; k < L; ++k) {
        if (k > 0) {
            double xp[6], AP[36], Pp[21];
            smooth_ct_predict(m, ct_transition(m.T, x[4]), x, P, xp, AP, Pp);
            for (int i = 0; i < 6; ++i) x[i] = xp[i];
            for (int e = 0; e < 21; ++e) P[e] = Pp[e];
            if (has_z[k]) smooth_update<6>(m, z[2 * k], z[2 * k + 1], x, P);
        }
        for (int i = 0; i < 6; ++i) xf[(size_t)k * 6 + i] = x[i];
        for (int e = 0; e < 21; ++e) Pf[(size_t)k * 21 + e] = P[e];
    }
    for (int k = L - 1; k >= 0; --k) {
        if (k < L - 1) {
            if (cov) smooth_ct_backward<true>(m, &xf[(size_t)k * 6], &Pf[(size_t)k * 21], x, P);
            else smooth_ct_backward<false>(m, &xf[(size_t)k * 6], &Pf[(size_t)k * 21], x, P);
        }
        for (int i = 0; i < 6; ++i) xs[(size_t)k * 6 + i] = x[i];
        if (cov)
            for (int e = 0; e < 21; ++e) Ps[(size_t)k * 21 + e] = P[e];
    }
}
