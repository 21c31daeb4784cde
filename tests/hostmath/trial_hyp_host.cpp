// TEST-ONLY host build of csrc/mht_trial_hyp.h: hyp_weights, hyp_cell, hyp_piece and hyp_target themselves -- what a lane of the
// kernels of mht_trial_hyp.hip runs per target, per cell, per piece and per (candidate, target) -- compiled for the CPU and run over a
// batch in the seam's own layouts, with the lanes of a tile, the tiles of a row and the pieces of a tile as loops, so that the weights,
// the segmented fold, its slots and the NaN rules are checked against tests/trial_hyp_ref.py without a GPU (tests/test_trial_hyp_cpu.py).
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
#include "../../pymht_amd/csrc/mht_trial_hyp.h"

using namespace mht;

static bool finite_or_nan(double v) { return v != v || v - v == 0.0; }

template <int N>
static void leaves(int32_t L, int32_t G, int32_t K, const double* Phi, const double* Q, const double* x, const double* P, double* xs, double* Ps,
                   double* pos, double* S) {
    EncounterModel<N> m;
    for (int c = 0; c < N * N; ++c) {
        m.Phi[c] = Phi[c];
        m.Q[c] = Q[c];
    }
    for (int l = 0; l < L; ++l) trial_track<N>(m, x, P, L, L + G, K, l, xs, Ps, pos, S);
}

// The doubles of the twin's work buffer: pos [K + 1][2][L + G], S [K + 1][3][L + G], partials [6][G][tiles + T], the staging xs [6][L + G]
// and Ps [21][L + G], wl [L], and the leaves' targets [L] as int32 in the space of L doubles
extern "C" int64_t trial_hyp_host_work_doubles(int32_t L, int32_t T, int32_t G, int32_t K) {
    const int64_t nt = (int64_t)L + G, chunks = ((int64_t)L + TRIAL_TILE - 1) / TRIAL_TILE;
    return 5 * (int64_t)(K + 1) * nt + HYP_PARTIAL * (int64_t)G * (chunks + T) + 27 * nt + 2 * (int64_t)L;
}

// The seam's arguments on host arrays; table may be null.  The partials are preset to `hole`, so that a slot read without having been
// written shows.  Returns 0, or -1 where the seam refuses (nothing written).
extern "C" int trial_hypotheses_host(int32_t nx, int32_t L, int32_t T, int32_t G, int32_t K, double dt, double R, const double* Phi, const double* Q,
                                     const double* x, const double* P, const double* cnllr, const int32_t* seg, const int32_t* sel, const double* own,
                                     const double* Sown, double w, const double* cand, double* table, double* fig, double* weight, double* work,
                                     double hole) {
    if ((nx != 4 && nx != 6) || K < 1 || K > ENCOUNTER_MAX_STEPS || G < 1 || G > TRIAL_MAX_CANDIDATES || L < 0) return -1;
    if (!(R > 0.0) || !(dt > 0.0) || !(w > 0.0) || R - R != 0.0 || dt - dt != 0.0 || w - w != 0.0) return -1;
    if (L == 0) return 0;
    if (T < 1 || T > L || seg[0] != 0 || seg[T] != L) return -1;
    for (int t = 0; t < T; ++t)
        if (seg[t + 1] < seg[t] || !(sel[t] == -1 || (sel[t] >= seg[t] && sel[t] < seg[t + 1]))) return -1;
    for (int c = 0; c < 4; ++c)
        if (!finite_or_nan(own[c])) return -1;
    for (int c = 0; c < 3; ++c)
        if (!finite_or_nan(Sown[c])) return -1;
    for (int c = 0; c < 3 * G; ++c)
        if (!finite_or_nan(cand[c])) return -1;
    for (int g = 0; g < G; ++g)
        if (fabs(cand[3 * g]) > 3.14159265358979323846 || cand[3 * g + 1] < 0.0 || cand[3 * g + 2] < 0.0) return -1;
    const size_t nt = (size_t)L + (size_t)G, steps = (size_t)(K + 1), chunks = ((size_t)L + TRIAL_TILE - 1) / TRIAL_TILE, slots = chunks + (size_t)T;
    double* pos = work;
    double* S = pos + 2 * steps * nt;
    double* partials = S + 3 * steps * nt;
    double* xs = partials + (size_t)HYP_PARTIAL * (size_t)G * slots;
    double* Ps = xs + 6 * nt;
    double* wl = Ps + 21 * nt;
    int32_t* target_of = (int32_t*)(wl + L);
    for (size_t i = 0; i < (size_t)HYP_PARTIAL * (size_t)G * slots; ++i) partials[i] = hole;
    for (int t = 0; t < T; ++t) hyp_weights(cnllr, seg, t, wl, weight, target_of);      // a lane's target
    if (nx == 4) leaves<4>(L, G, K, Phi, Q, x, P, xs, Ps, pos, S);
    else leaves<6>(L, G, K, Phi, Q, x, P, xs, Ps, pos, S);
    const TrialOwn o = {{own[0], own[1]}, {own[2], own[3]}, {Sown[0], Sown[1], Sown[2]}, w};
    for (int g = 0; g < G; ++g) trial_candidate(o, cand[3 * g], cand[3 * g + 1], cand[3 * g + 2], L + G, K, dt, L + g, pos, S);
    for (size_t tile = 0; tile < (size_t)G * chunks; ++tile) {      // a workgroup's tile
        double pc[TRIAL_TILE], dcpa[TRIAL_TILE], wt[TRIAL_TILE];
        const int g = (int)(tile / chunks);
        const size_t chunk = tile % chunks;
        const int base = (int)(chunk * TRIAL_TILE);
        for (int lane = 0; lane < TRIAL_TILE && base + lane < L; ++lane) {      // the lanes in turn: their cells
            const int l = base + lane, t = target_of[l];
            double o5[ENCOUNTER_FIGURES];
            hyp_cell(pos, S, L, G, K, dt, R, g, l, table, o5);
            if (sel[t] == l) hyp_store_selected(o5, G, T, g, t, fig);
            pc[lane] = o5[3];
            dcpa[lane] = o5[1];
            wt[lane] = wl[l];
        }
        for (int lane = 0; lane < TRIAL_TILE && base + lane < L; ++lane) {      // behind the barrier: the heads of the pieces
            const int l = base + lane, t = target_of[l];
            if (lane == 0 || target_of[l - 1] != t)
                hyp_store(hyp_piece(pc, dcpa, wt, base, lane, seg[t + 1]), partials + (size_t)g * slots + chunk + (size_t)t, (size_t)G * slots);
        }
    }
    for (int g = 0; g < G; ++g)      // a lane's (candidate, target)
        for (int t = 0; t < T; ++t) hyp_target(partials, seg, sel, G, T, slots, g, t, fig);
    return 0;
}
