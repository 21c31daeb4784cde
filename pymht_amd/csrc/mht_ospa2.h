// OSPA(2) of one window (mht_ospa2_windows, include/mht_amd.h; Beard, Vo, Vo 2020): OSPA between the set of tracks and the set of truth
// trajectories, whose base distance between one track and one trajectory is their time-averaged cut-off distance over the window's
// steps.  This header holds what the device kernels (mht_ospa2.hip) and the host twin (tests/hostmath/ospa2_host.cpp) share: the base
// distance (ospa2_add per step, ospa2_close at the end) and the window's search and closing formula (ospa2_window), which is the search
// of mht_gospa.h (gospa_search) with its cost read from the window's matrix of base distances.
//
//   members       a track / truth present at one or more of the window's steps; n_w, m_w of them, N = max(n_w, m_w)
//   D_ij          over the U >= 1 steps of the window at which at least one of i, j is present: a step is NEAR if both are present and
//                 d = sqrt(dx dx + dy dy) < c, else FAR.  No near step: D = c exactly, no edge.  Else D = (c nFar + sum of the near d) / U,
//                 an edge iff D < c as computed.  (Order 1 in time: no pow.)
//   total         min over one-to-one assignments on edges of  sum D_ij^p + c^p (N - nAssigned)
// The smaller side are the rows, an edge weighs D^p - c^p, every row has a zero exit: gospa_search's problem.  Positions at cells whose
// presence flag is 0 never reach a result: they enter a comparison and a select only.
#pragma once
#include "mht_gospa.h"

namespace mht {

struct Ospa2Acc {      // one (row, column) pair over the steps of a window
    double sum;        // of d over the near steps, in step order
    int32_t n_near, n_any;
};

GOSPA_FN void ospa2_add(Ospa2Acc& a, bool on_r, double rx, double ry, bool on_c, double cx, double cy, double c) {
    const double dx = cx - rx, dy = cy - ry;
    const double d = sqrt(dx * dx + dy * dy);
    const bool near = on_r && on_c && d < c;
    a.n_any += (on_r || on_c) ? 1 : 0;
    a.n_near += near ? 1 : 0;
    a.sum += near ? d : 0.0;
}

// D of the pair.  (Called for members only, so n_any >= 1 wherever n_near >= 1.)
GOSPA_FN double ospa2_close(const Ospa2Acc& a, double c) {
    if (a.n_near == 0) return c;
    return (c * (double)(a.n_any - a.n_near) + a.sum) / (double)a.n_any;
}

// Present at one or more of the steps lo .. hi?  on [n_steps][n_obj]
GOSPA_FN bool ospa2_member(const uint8_t* on, int32_t n_obj, int32_t i, int32_t lo, int32_t hi) {
    bool mem = false;
    for (int32_t t = lo; t <= hi; ++t) mem = mem || on[(size_t)t * n_obj + i] != 0;
    return mem;
}

struct Ospa2Window {
    const double* D;             // [n_rows][n_cols] base distances of the members, the smaller side the rows
    const int32_t* row_idx;      // [n_rows] member -> track / truth index
    const int32_t* col_idx;      // [n_cols]
    int32_t n_rows, n_cols;
    bool rows_are_trk;
    int32_t p;                   // 1 or 2
    double c, cp;                // the cut-off and c^p
};

// The search's cost from the window's matrix: a sweep reads a contiguous row
struct Ospa2Cost {
    const Ospa2Window& w;
    const double* cur;
    GOSPA_FN explicit Ospa2Cost(const Ospa2Window& win) : w(win), cur(win.D) {}
    GOSPA_FN void row(int i) { cur = w.D + (size_t)i * w.n_cols; }
    GOSPA_FN bool edge(int j, double& wt) const {
        const double d = cur[j];
        wt = (w.p == 2 ? d * d : d) - w.cp;
        return d < w.c;
    }
};

// One window from its matrix to its outputs: win_out [2] = total, localisation; count_out [3] = nAssigned, n_w, m_w; match_out
// [n_trk], which the caller has filled with -1 at the members and -2 elsewhere: the assigned tracks get their truth's index.  A failed
// search: NaN, NaN, 0 assigned and match_out as it came.
GOSPA_FN void ospa2_window(const Ospa2Window& w, const GospaTables& t, double* win_out, int32_t* count_out, int32_t* match_out, int32_t* sweeps) {
    const int nr = w.n_rows, nc = w.n_cols;
    Ospa2Cost cost(w);
    const bool ok = gospa_search(cost, nr, nc, t, sweeps);
    GOSPA_PER_LANE(double, part);
    GOSPA_PER_LANE(int, cnt);
    GOSPA_EACH_LANE(lane) {
        double sum = 0.0;
        int k = 0;
        for (int j = lane; j < nc; j += GOSPA_LANES) {
            const int o = t.owner[j];
            if (ok && o != GOSPA_NONE) {
                const double d = w.D[(size_t)o * nc + j];
                sum += w.p == 2 ? d * d : d;
                ++k;
                if (w.rows_are_trk) match_out[w.row_idx[o]] = w.col_idx[j];
                else match_out[w.col_idx[j]] = w.row_idx[o];
            }
        }
        GOSPA_AT(part, lane) = sum;
        GOSPA_AT(cnt, lane) = k;
    }
    double loc;
    int n_assigned;
    gospa_sum(part, cnt, loc, n_assigned);
    GOSPA_ONE_LANE {
        const double nan = NAN;
        win_out[0] = ok ? loc + w.cp * (double)(nc - n_assigned) : nan;      // (N = max(n_w, m_w) are the columns)
        win_out[1] = ok ? loc : nan;
        count_out[0] = n_assigned;
        count_out[1] = w.rows_are_trk ? nr : nc;
        count_out[2] = w.rows_are_trk ? nc : nr;
    }
}

}  // namespace mht
