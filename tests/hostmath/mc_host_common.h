// TEST-ONLY: what the host twins of the two Monte-Carlo engines (mc_host.cpp, mc_pair_host.cpp) share -- the names csrc/mht_mc.h wants
// from <cmath>, the set-up of a call (the model, the components' factors, the targets' statuses), the seam's checks of what both
// seams take, and csrc/mht_mc.h's own dispatcher from (nx, transition) to <N, CT>.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstddef>
#include <cstdio>
#include <vector>
using std::fma;
using std::sqrt;
using std::fabs;
using std::fmin;
using std::fmax;
using std::log;
using std::sin;
using std::cos;
#include "../../pymht_amd/csrc/mht_mc_pair.h"

using namespace mht;

namespace {

// The model of a call, every component's factor Lw (as a lane of mc_factor_kernel leaves it) and every target's status tst.  False: Q
// is not positive semidefinite.
template <int N, bool CT>
bool prepare(int32_t nComp, int32_t T, double dt, double R, const double* Phi, const double* Q, const double* x, const double* P, const int32_t* first,
             const double* cdf, McModel<N>& m, std::vector<double>& Lw, std::vector<int32_t>& tst) {
    if (!mc_model<N>(CT ? nullptr : Phi, Q, dt, R, m)) return false;
    Lw.assign((size_t)(N * (N + 1) / 2) * (size_t)nComp, 0.0);
    std::vector<int32_t> cst((size_t)nComp);
    for (int c = 0; c < nComp; ++c) mc_component<N>(x, P, cdf, nComp, c, Lw.data(), cst.data());      // a lane's component
    tst.assign((size_t)T, 0);
    for (int t = 0; t < T; ++t) tst[t] = mc_target_status(first, cst.data(), t);
    return true;
}

// What both seams check of the arguments both take (the particles apart: mc_pair_path_host walks one)
bool fits(int32_t nx, int32_t transition, int32_t nComp, int32_t T, int32_t K, double dt, double R, const double* Phi, const double* Q, const int32_t* first) {
    if ((nx != 4 && nx != 6) || (transition != 0 && transition != 1) || (transition == 1 && nx != 6)) return false;
    if (nComp < 1 || T < 1 || T > nComp || K < 1 || K > MC_MAX_STEPS) return false;
    if (!(R > 0.0) || !(dt > 0.0) || !mc_finite(R) || !mc_finite(dt)) return false;
    if (first[0] != 0 || first[T] != nComp) return false;
    for (int t = 0; t < T; ++t)
        if (first[t + 1] <= first[t]) return false;
    for (int c = 0; c < nx * nx; ++c)
        if (!mc_finite(Q[c]) || (transition == 0 && !mc_finite(Phi[c]))) return false;
    return true;
}

bool particles_fit(int32_t S) { return S >= MC_WARP && S <= MC_MAX_PARTICLES && S % MC_WARP == 0; }

}  // namespace
