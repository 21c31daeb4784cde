// TEST-ONLY host build of csrc/mht_smooth_ais_math.h (and of the mht_smooth_math.h functions it shares with the linear smoother): one
// track walked forward and backward on the CPU with exactly the functions a lane of smooth_ais_kernel calls, in its order, so that the
// AIS update and the two-leg backward step are checked against tests/smooth_ais_ref.py without a GPU (tests/test_smooth_ais_cpu.py).
#include <cmath>
#include <cstdint>
#include <vector>
using std::fma;
using std::sqrt;
using std::fabs;
#include "../../pymht_amd/csrc/mht_smooth_ais_math.h"

using namespace mht;

// A [16], Q [16], C [8], R [4] row-major float64; z [L][2], has_z [L], kind [L], ais_z [L][4], ais_r [L], leg [L], legs [n_legs][52];
// xs [L][4], Ps [L][10] packed.  cov = 0: means only.
extern "C" void smooth_ais_host(const double* A, const double* Q, const double* C, const double* R, int32_t L, const double* x_init,
                                const double* P_init, const double* z, const uint8_t* has_z, const uint8_t* kind, const double* ais_z,
                                const double* ais_r, const int32_t* leg, const double* legs, double* xs, double* Ps, int32_t cov) {
    SmoothModel<4> m;
    for (int i = 0; i < 16; ++i) m.A[i] = A[i];
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j) m.Q[sym_idx(4, i, j)] = Q[i * 4 + j];
    for (int i = 0; i < 8; ++i) m.C[i] = C[i];
    m.R[0] = R[0]; m.R[1] = R[1]; m.R[2] = R[3];
    double x[4], P[10];
    for (int i = 0; i < 4; ++i) x[i] = x_init[i];
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j) P[sym_idx(4, i, j)] = P_init[i * 4 + j];
    std::vector<double> xf((size_t)L * 8), Pf((size_t)L * 20);      // two slots per node: at the scan's time, at the message's time
    for (int k = 0; k < L; ++k) {
        if (k > 0) {
            if (kind[k] >= 2) {
                smooth_ais_forward(legs + (size_t)leg[k] * SMOOTH_AIS_LEG_DOUBLES, ais_z + 4 * k, ais_r[k], x, P, &xf[(size_t)k * 8 + 4], &Pf[(size_t)k * 20 + 10]);
            } else {
                double xp[4], AP[16], Pp[10];
                smooth_predict<4>(m, x, P, xp, AP, Pp);
                for (int i = 0; i < 4; ++i) x[i] = xp[i];
                for (int e = 0; e < 10; ++e) P[e] = Pp[e];
            }
            if (has_z[k]) smooth_update<4>(m, z[2 * k], z[2 * k + 1], x, P);
        }
        for (int i = 0; i < 4; ++i) xf[(size_t)k * 8 + i] = x[i];
        for (int e = 0; e < 10; ++e) Pf[(size_t)k * 20 + e] = P[e];
    }
    for (int k = L - 1; k >= 0; --k) {
        if (k < L - 1) {
            const double* xfk = &xf[(size_t)k * 8];
            const double* Pfk = &Pf[(size_t)k * 20];
            if (kind[k + 1] >= 2) {
                const double* entry = legs + (size_t)leg[k + 1] * SMOOTH_AIS_LEG_DOUBLES;
                if (cov) smooth_ais_backward<true>(entry, &xf[(size_t)(k + 1) * 8 + 4], &Pf[(size_t)(k + 1) * 20 + 10], xfk, Pfk, x, P);
                else smooth_ais_backward<false>(entry, &xf[(size_t)(k + 1) * 8 + 4], &Pf[(size_t)(k + 1) * 20 + 10], xfk, Pfk, x, P);
            } else {
                if (cov) smooth_backward<4, true>(m, xfk, Pfk, x, P);
                else smooth_backward<4, false>(m, xfk, Pfk, x, P);
            }
        }
        for (int i = 0; i < 4; ++i) xs[(size_t)k * 4 + i] = x[i];
        if (cov)
            for (int e = 0; e < 10; ++e) Ps[(size_t)k * 10 + e] = P[e];
    }
}
