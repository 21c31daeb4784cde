// TEST-ONLY host build of csrc/mht_nees.h: nees_cell itself -- what a lane of the kernels of mht_nees.hip runs per cell, with
// smooth_cholesky under it -- compiled for the CPU and run over a batch in the seam's own track-minor layouts, so that the evaluation,
// its indexing and its NaN rules are checked against tests/nees_ref.py without a GPU (tests/test_nees_cpu.py).
#include <cmath>
#include <cstdint>
using std::fma;
using std::sqrt;
using std::fabs;
#include "../../pymht_amd/csrc/mht_nees.h"

using namespace mht;

// nx = 4 or 6, D = 2, 4 or nx: x [L_max][nx][n], P [L_max][nx (nx + 1) / 2][n], truth [L_max][nx][n], present [L_max][n],
// out [L_max][nx + 3][n].  Returns 0, or -1 for a bad nx or D (nothing written).
extern "C" int nees_nodes_host(int32_t nx, int32_t n, int32_t L_max, int32_t D, const double* x, const double* P, const double* truth,
                               const uint8_t* present, double* out) {
    if ((nx != 4 && nx != 6) || (D != 2 && D != 4 && D != nx)) return -1;
    const NeesArgs a = {n, L_max, D, x, P, truth, present, out};
    for (int k = 0; k < L_max; ++k)
        for (int t = 0; t < n; ++t) {
            if (nx == 4) nees_cell<4>(a, k, t);
            else nees_cell<6>(a, k, t);
        }
    return 0;
}
