// TEST-ONLY host build of csrc/mht_smooth_score_grid.h: smooth_score_grid_walk itself -- the code a lane of the kernels of
// mht_smooth_score_grid.hip runs -- compiled for the CPU and run one (track, candidate) at a time (n = 1, t = 0: the track-minor layout is
// then plain [node][element], and row g of the outputs is element g), next to the host build of the score walk it must agree with
// (smooth_score_host.cpp, included: smooth_score_lin_host / smooth_score_ct_host of the same library).  tests/test_smooth_score_grid_cpu.py.
#include "smooth_score_host.cpp"
#include "../../pymht_amd/csrc/mht_smooth_score_grid.h"

// The table the seams build: per candidate Q's upper triangle packed, then R00, R01, R11
template <int N>
static std::vector<double> table(int32_t G, const double* Q_cand, const double* R_cand) {
    constexpr int NS = N * (N + 1) / 2;
    std::vector<double> t((size_t)G * (NS + 3));
    for (int32_t g = 0; g < G; ++g) {
        for (int i = 0; i < N; ++i)
            for (int j = i; j < N; ++j) t[(size_t)g * (NS + 3) + sym_idx(N, i, j)] = Q_cand[((size_t)g * N + i) * N + j];
        t[(size_t)g * (NS + 3) + NS] = R_cand[g * 4]; t[(size_t)g * (NS + 3) + NS + 1] = R_cand[g * 4 + 1]; t[(size_t)g * (NS + 3) + NS + 2] = R_cand[g * 4 + 3];
    }
    return t;
}

// ll [G], nis [G], nobs [1]; the policy's own Q and R are poisoned: a walk that read them would show it
template <int N, typename Steps>
static void grid(Steps steps, int32_t L, const double* x_init, const double* P_init, const double* z, const uint8_t* has_z, int32_t G,
                 const double* Q_cand, const double* R_cand, double* ll, double* nis, int32_t* nobs) {
    for (double& q : steps.model.Q) q = __builtin_nan("");
    for (double& r : steps.model.R) r = __builtin_nan("");
    const std::vector<double> t = table<N>(G, Q_cand, R_cand);
    ScoreGridArgs<N, Steps> a = {};
    a.s = {steps, 1, L, &L, x_init, P_init, z, has_z, nullptr, ll, nis, nobs, nullptr, nullptr};
    a.cand = t.data();
    a.n_cand = G;
    for (int32_t g = G - 1; g >= 0; --g) smooth_score_grid_walk<N>(a, 0, g);
}

// As smooth_score_lin_host, with Q_cand [G][nx][nx] and R_cand [G][4] in place of Q and R
extern "C" void smooth_score_grid_lin_host(int32_t nx, const double* A, const double* C, int32_t L, const double* x_init, const double* P_init,
                                           const double* z, const uint8_t* has_z, int32_t G, const double* Q_cand, const double* R_cand, double* ll,
                                           double* nis, int32_t* nobs) {
    if (nx == 4) {
        LinearSteps<4> s = {};
        std::copy(A, A + 16, s.model.A);
        std::copy(C, C + 8, s.model.C);
        grid<4>(s, L, x_init, P_init, z, has_z, G, Q_cand, R_cand, ll, nis, nobs);
    } else {
        LinearSteps<6> s = {};
        std::copy(A, A + 36, s.model.A);
        std::copy(C, C + 12, s.model.C);
        grid<6>(s, L, x_init, P_init, z, has_z, G, Q_cand, R_cand, ll, nis, nobs);
    }
}

extern "C" void smooth_score_grid_ct_host(double T, const double* C, int32_t L, const double* x_init, const double* P_init, const double* z,
                                          const uint8_t* has_z, int32_t G, const double* Q_cand, const double* R_cand, double* ll, double* nis,
                                          int32_t* nobs) {
    ConstantTurnSteps s = {};
    std::copy(C, C + 12, s.model.C);
    s.model.T = T;
    grid<6>(s, L, x_init, P_init, z, has_z, G, Q_cand, R_cand, ll, nis, nobs);
}
