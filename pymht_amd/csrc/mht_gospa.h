// GOSPA of one step (mht_gospa_steps, include/mht_amd.h): the optimal partial assignment between a set of estimates and a set of true
// positions under a cut-off c, and its split into localisation error, missed targets and false tracks.  The code ONE WAVEFRONT of
// gospa_kernel (mht_gospa.hip) runs for its step, and tests/hostmath/gospa_host.cpp on the CPU with the 64 lanes as a loop.
//
//   total = min over partial one-to-one assignments of  sum d_ij^p + c^p / 2 (n + m - 2 |assigned|),   only pairs with d_ij < c
//
// Solved in its unbalanced form, not as a square problem padded with cut-off costs (there every object without a partner ties with
// every other and a shortest-path search walks long chains through the ties): the smaller side are the ROWS, an edge (i, j) exists
// where d_ij < c and weighs d_ij^p - c^p, every row has a private exit of weight 0 ("stays unassigned"), a column may stay free at no
// cost; minimise the weight of the rows' choices.  Rows are inserted one at a time by a Dijkstra over the columns under dual prices
// (u per row, v per column; the Hungarian / Jonker-Volgenant row insertion): a SWEEP relaxes the slack of every unvisited column from
// the row just reached and takes the nearest; the exits of the visited rows are one more, virtual, column (an exit is private, so
// its price is 0 and its slack from row i is -u_i).  The search ends at a free column, or at an exit: then the row whose exit it is
// leaves its column and the path shifts back to the new row.  u_i <= 0 and v_j <= 0 throughout, v_j = 0 on a free column.
//
// Every loop is counted: a row insertion makes at most n_cols + 1 sweeps (every sweep but the last visits a new column), a path has
// at most n_cols columns.  A step that runs into a bound is reported as failed (NaN), it never spins.
//
// Lanes: lane l owns columns l, l + 64, ..: their slack, predecessor and price are read and written by that lane alone, its visited
// columns are one 32-bit word in a register (GOSPA_MAX_SET / 64 = 32).  The row prices, the owners and the predecessors on the path
// cross lanes; GOSPA_SYNC orders those accesses (one wavefront: a fence, no hardware barrier to wait at).  What is uniform over the
// wavefront by construction is made uniform for the compiler too (gospa_uniform), so the loops branch on scalars.
#pragma once
#include <math.h>
#include <stdint.h>
#include <cmath>

// (hipcc parses a kernel's callees in its host pass as well: under it the functions are host and device, and the lane macros below
// follow the pass)
#if defined(__HIPCC__)
#define GOSPA_HD __host__ __device__ inline
#define GOSPA_FN __host__ __device__ __forceinline__
#else
#define GOSPA_HD inline
#define GOSPA_FN inline
#endif

namespace mht {

constexpr int GOSPA_MAX_SET = 2048;      // objects of one step on either side
constexpr int GOSPA_LANES = 64;
constexpr int GOSPA_NONE = 0xFFFF;       // no owner / no predecessor (indices are 16-bit: GOSPA_MAX_SET <= 0xFFFF)
static_assert(GOSPA_MAX_SET / GOSPA_LANES <= 32, "a lane's visited columns are one 32-bit word");

struct GospaStep {
    const double* row_xy;      // [n_rows][2], the smaller side
    const double* col_xy;      // [n_cols][2]
    int32_t n_rows, n_cols;
    int32_t p;                 // 1 or 2
    double cp;                 // c^p
    double lim;                // an edge has d^p < lim: exactly the pairs with sqrt(dx dx + dy dy) < c (gospa_cutoff)
};

struct GospaTables {           // LDS on the device
    double* u;                 // [n_rows] row prices
    double* v;                 // [n_cols] column prices
    double* minv;              // [n_cols] slack of the column in the current search
    uint16_t* way;             // [n_cols] the column in front of it on its shortest path (GOSPA_NONE: the new row);
                               //          after the search: row -> its column (n_rows <= n_cols)
    uint16_t* owner;           // [n_cols] the row assigned to it
};

// Bytes of the tables for the largest step of a launch; every carve is a multiple of 16
inline constexpr size_t gospa_round8(int n) { return (size_t)((n + 7) / 8) * 8; }
inline constexpr size_t gospa_table_bytes(int max_rows, int max_cols) { return gospa_round8(max_rows) * 8 + gospa_round8(max_cols) * (8 + 8 + 2 + 2); }

GOSPA_HD GospaTables gospa_carve(char* base, int max_rows, int max_cols) {
    const size_t r = gospa_round8(max_rows), c = gospa_round8(max_cols);
    GospaTables t;
    t.u = reinterpret_cast<double*>(base);
    t.v = t.u + r;
    t.minv = t.v + c;
    t.way = reinterpret_cast<uint16_t*>(t.minv + c);
    t.owner = t.way + c;
    return t;
}

// c^p and the edge limit (host).  p == 1: d < c.  p == 2: d^2 is compared and no root is taken, so lim is the smallest float64 whose
// correctly rounded root is >= c: d2 < lim iff sqrt(d2) < c, bit for bit what a caller computing distances sees.  false: c^p is not a
// positive finite number.
inline bool gospa_cutoff(double c, int32_t p, double* cp, double* lim) {
    if (!(c > 0.0) || !std::isfinite(c)) return false;
    if (p == 1) {
        *cp = c;
        *lim = c;
        return true;
    }
    const double c2 = c * c;
    if (!(c2 > 0.0) || !std::isfinite(c2)) return false;
    double t = c2;      // the largest float64 whose root is below c lies within a few ulp of c * c
    for (int k = 0; k < 8 && sqrt(t) >= c; ++k) t = nextafter(t, 0.0);
    for (int k = 0; k < 8 && sqrt(nextafter(t, HUGE_VAL)) < c; ++k) t = nextafter(t, HUGE_VAL);
    *cp = c2;
    *lim = nextafter(t, HUGE_VAL);
    return std::isfinite(*lim) && sqrt(t) < c && !(sqrt(*lim) < c);
}

#if defined(__HIP_DEVICE_COMPILE__)
#define GOSPA_EACH_LANE(lane) for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define GOSPA_PER_LANE(T, name) T name
#define GOSPA_AT(name, lane) name
#define GOSPA_ONE_LANE if (threadIdx.x == 0)
#define GOSPA_SYNC()                                              \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");    \
    } while (0)

GOSPA_FN int gospa_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
GOSPA_FN double gospa_uniform(double x) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
// the smallest value of the wavefront, the smallest index among equals
GOSPA_FN void gospa_argmin(double val, int idx, double& out_val, int& out_idx) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(val, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (ov < val || (ov == val && oi < idx)) {
            val = ov;
            idx = oi;
        }
    }
    out_val = gospa_uniform(val);
    out_idx = gospa_uniform(idx);
}
GOSPA_FN void gospa_sum(double part, int cnt, double& out_sum, int& out_cnt) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        part += __shfl_xor(part, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
    }
    out_sum = gospa_uniform(part);
    out_cnt = gospa_uniform(cnt);
}
#else
#define GOSPA_EACH_LANE(lane) for (int lane = 0; lane < GOSPA_LANES; ++lane)
#define GOSPA_PER_LANE(T, name) T name[GOSPA_LANES]
#define GOSPA_AT(name, lane) name[lane]
#define GOSPA_ONE_LANE
#define GOSPA_SYNC() ((void)0)

GOSPA_FN int gospa_uniform(int x) { return x; }
GOSPA_FN double gospa_uniform(double x) { return x; }
GOSPA_FN void gospa_argmin(const double* val, const int* idx, double& out_val, int& out_idx) {
    out_val = val[0];
    out_idx = idx[0];
    for (int l = 1; l < GOSPA_LANES; ++l)
        if (val[l] < out_val || (val[l] == out_val && idx[l] < out_idx)) {
            out_val = val[l];
            out_idx = idx[l];
        }
}
GOSPA_FN void gospa_sum(const double* part, const int* cnt, double& out_sum, int& out_cnt) {
    out_sum = 0.0;
    out_cnt = 0;
    for (int l = 0; l < GOSPA_LANES; ++l) {
        out_sum += part[l];
        out_cnt += cnt[l];
    }
}
#endif

// d^p between a row and a column: p == 2 without a root.  Not finite where a coordinate is not.
GOSPA_FN double gospa_dp(const GospaStep& s, double rx, double ry, int j) {
    const double dx = s.col_xy[2 * j] - rx, dy = s.col_xy[2 * j + 1] - ry;
    const double d2 = dx * dx + dy * dy;
    return s.p == 2 ? d2 : sqrt(d2);
}

// Where the search takes an edge's weight from (its COST): row(i) makes row i the one the next sweep relaxes from (wavefront-uniform),
// edge(j, w) says whether (that row, column j) is an edge and gives its weight w = d^p - c^p.  GospaXYCost is GOSPA's own, distances
// between positions; mht_ospa2.h reads a matrix of base distances instead.
struct GospaXYCost {
    const GospaStep& s;
    double rx, ry;
    GOSPA_FN explicit GospaXYCost(const GospaStep& step) : s(step), rx(0.0), ry(0.0) {}
    GOSPA_FN void row(int i) {
        rx = gospa_uniform(s.row_xy[2 * i]);
        ry = gospa_uniform(s.row_xy[2 * i + 1]);
    }
    GOSPA_FN bool edge(int j, double& w) const {
        const double dp = gospa_dp(s, rx, ry, j);
        w = dp - s.cp;
        return dp < s.lim;
    }
};

// The assignment of nr rows to nc >= nr columns under a cost: owner[j] of every column on return.  false: a loop ran into its bound.
// *sweeps counts the sweeps.
template <class Cost>
GOSPA_FN bool gospa_search(Cost& cost, int nr, int nc, const GospaTables& t, int32_t* sweeps) {
    const double inf = HUGE_VAL;
    GOSPA_EACH_LANE(lane) {
        for (int j = lane; j < nc; j += GOSPA_LANES) {
            t.v[j] = 0.0;
            t.owner[j] = (uint16_t)GOSPA_NONE;
        }
        for (int i = lane; i < nr; i += GOSPA_LANES) t.u[i] = 0.0;
    }
    GOSPA_SYNC();
    int32_t n_sweeps = 0;
    bool ok = true;
    for (int r = 0; r < nr; ++r) {      // insert row r
        GOSPA_PER_LANE(uint32_t, used);      // bit k: column lane + 64 k is on the search tree
        GOSPA_EACH_LANE(lane) {
            GOSPA_AT(used, lane) = 0u;
            for (int j = lane; j < nc; j += GOSPA_LANES) t.minv[j] = inf;
        }
        int i0 = r, j0 = GOSPA_NONE;         // the row the sweep relaxes from, and the column it was reached through
        double min_exit = inf;               // slack of the nearest exit among the visited rows, and the column of that row
        int way_exit = GOSPA_NONE, end_col = GOSPA_NONE;
        bool found = false;
        for (int sweep = 0; sweep < nc + 2; ++sweep) {
            ++n_sweeps;
            cost.row(i0);
            const double ui = gospa_uniform(t.u[i0]);
            if (-ui < min_exit) {
                min_exit = -ui;
                way_exit = j0;
            }
            GOSPA_PER_LANE(double, best);
            GOSPA_PER_LANE(int, best_j);
            GOSPA_EACH_LANE(lane) {
                const uint32_t um = GOSPA_AT(used, lane);
                double b = inf;
                int bj = 0x7fffffff;
                for (int k = 0, j = lane; j < nc; ++k, j += GOSPA_LANES) {
                    if ((um >> k) & 1u) continue;
                    double w;
                    const bool is_edge = cost.edge(j, w);
                    double m = t.minv[j];
                    if (is_edge) {
                        const double cur = w - ui - t.v[j];
                        if (cur < m) {
                            m = cur;
                            t.minv[j] = cur;
                            t.way[j] = (uint16_t)j0;
                        }
                    }
                    if (m < b) {
                        b = m;
                        bj = j;
                    }
                }
                GOSPA_AT(best, lane) = b;
                GOSPA_AT(best_j, lane) = bj;
            }
            double delta;
            int j1;
            gospa_argmin(best, best_j, delta, j1);
            const bool take_exit = min_exit <= delta;      // (also: no column can be reached at all)
            if (take_exit) delta = min_exit;
            // move the prices by delta: the tree's rows up, its columns down, every slack outside it down
            GOSPA_ONE_LANE { t.u[r] += delta; }
            GOSPA_EACH_LANE(lane) {
                const uint32_t um = GOSPA_AT(used, lane);
                for (int k = 0, j = lane; j < nc; ++k, j += GOSPA_LANES) {
                    if ((um >> k) & 1u) {
                        t.u[t.owner[j]] += delta;
                        t.v[j] -= delta;
                    } else {
                        t.minv[j] -= delta;
                    }
                }
            }
            min_exit -= delta;
            GOSPA_SYNC();
            if (take_exit) {
                end_col = way_exit;
                found = true;
                break;
            }
            const int o1 = gospa_uniform((int)t.owner[j1]);
            if (o1 == GOSPA_NONE) {
                end_col = j1;
                found = true;
                break;
            }
            GOSPA_EACH_LANE(lane) {
                if ((j1 & (GOSPA_LANES - 1)) == lane) GOSPA_AT(used, lane) |= 1u << (j1 / GOSPA_LANES);
            }
            j0 = j1;
            i0 = o1;
        }
        if (!found) {
            ok = false;
            break;
        }
        // shift the path: every column on it takes the row of the column in front of it, the first one takes row r.  (Ended at an
        // exit: end_col is the column of the row that leaves, which is thereby unassigned; GOSPA_NONE if row r itself stays out.)
        int j = end_col;
        for (int hop = 0; hop < nc + 1 && j != GOSPA_NONE; ++hop) {
            const int jp = gospa_uniform((int)t.way[j]);
            const int o = jp == GOSPA_NONE ? r : gospa_uniform((int)t.owner[jp]);
            GOSPA_ONE_LANE { t.owner[j] = (uint16_t)o; }
            j = jp;
        }
        GOSPA_SYNC();
        if (j != GOSPA_NONE) {
            ok = false;
            break;
        }
    }
    if (sweeps) *sweeps = n_sweeps;
    return ok;
}

// GOSPA's own instance: the cost from the step's positions
GOSPA_FN bool gospa_solve(const GospaStep& s, const GospaTables& t, int32_t* sweeps) {
    GospaXYCost cost(s);
    return gospa_search(cost, s.n_rows, s.n_cols, t, sweeps);
}

// One step from its sets to its outputs: step_out [2] = total, loc; count_out [3] = nAssigned, nMissed, nFalse; match_out [n_est] =
// the truth of every estimate or -1.  rows_are_est: the estimates are the rows (the smaller side), else the truths are.  Every cell
// is written.  A failed search: NaN, NaN; 0, every truth missed, every estimate false; -1.
GOSPA_FN void gospa_step(const GospaStep& s, const GospaTables& t, bool rows_are_est, double* step_out, int32_t* count_out, int32_t* match_out,
                         int32_t* sweeps) {
    const int nr = s.n_rows, nc = s.n_cols;
    const int n_est = rows_are_est ? nr : nc, n_tru = rows_are_est ? nc : nr;
    const bool ok = gospa_solve(s, t, sweeps);
    GOSPA_PER_LANE(double, part);
    GOSPA_PER_LANE(int, cnt);
    GOSPA_EACH_LANE(lane) {
        double sum = 0.0;
        int k = 0;
        for (int j = lane; j < nc; j += GOSPA_LANES) {
            const int o = t.owner[j];
            if (ok && o != GOSPA_NONE) {
                sum += gospa_dp(s, s.row_xy[2 * o], s.row_xy[2 * o + 1], j);
                ++k;
            }
        }
        GOSPA_AT(part, lane) = sum;
        GOSPA_AT(cnt, lane) = k;
    }
    double loc;
    int n_assigned;
    gospa_sum(part, cnt, loc, n_assigned);
    if (rows_are_est) {      // row -> column, in the predecessors' place: the search is over
        uint16_t* col_of = t.way;
        GOSPA_EACH_LANE(lane) {
            for (int i = lane; i < nr; i += GOSPA_LANES) col_of[i] = (uint16_t)GOSPA_NONE;
        }
        GOSPA_SYNC();
        GOSPA_EACH_LANE(lane) {
            for (int j = lane; j < nc; j += GOSPA_LANES)
                if (ok && t.owner[j] != GOSPA_NONE) col_of[t.owner[j]] = (uint16_t)j;
        }
        GOSPA_SYNC();
        GOSPA_EACH_LANE(lane) {
            for (int i = lane; i < nr; i += GOSPA_LANES) match_out[i] = col_of[i] == GOSPA_NONE ? -1 : (int32_t)col_of[i];
        }
    } else {
        GOSPA_EACH_LANE(lane) {
            for (int j = lane; j < nc; j += GOSPA_LANES) match_out[j] = (ok && t.owner[j] != GOSPA_NONE) ? (int32_t)t.owner[j] : -1;
        }
    }
    GOSPA_ONE_LANE {
        const double nan = NAN;
        step_out[0] = ok ? loc + 0.5 * s.cp * (double)(n_est + n_tru - 2 * n_assigned) : nan;
        step_out[1] = ok ? loc : nan;
        count_out[0] = n_assigned;
        count_out[1] = n_tru - n_assigned;
        count_out[2] = n_est - n_assigned;
    }
}

}  // namespace mht
