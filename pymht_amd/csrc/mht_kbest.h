// The K best global hypotheses of one cluster (mht_kbest_hypotheses, include/mht_amd.h).  The cluster's targets each own a group of
// columns (a column is a leaf: a cost and up to `depth` row ids, the plots on its window path); a global hypothesis picks one column
// per target so that no two picked columns share a row id; its cost is the float64 sum of the picked costs, from 0.0, left to right
// in target order.  Listed are the K cheapest under the total order (cost, then the tuple of column indices in target order): the
// list is unique.  The code ONE WAVEFRONT of kbest_kernel (mht_kbest.hip) runs for its cluster, and tests/hostmath/kbest_host.cpp on
// the CPU with the 64 lanes as a loop.
//
// A plain depth-first branch and bound, the targets in order, each target's columns by ascending (cost, index) -- ranked in the
// prologue, columns with a non-finite cost last and never tested.  The wavefront walks ONE search and stays uniform: at the current
// target its 64 lanes test 64 sibling columns at once (a CHUNK), each lane its column's row ids against the used-row table in LDS, and
// a ballot yields the viable ones; the wavefront descends into the first and keeps the rest of the mask.  The current level's state
// (mask, chunk, partial sum) is scalar; the levels below it are a stack in LDS (runtime-indexed registers would be scratch).
//
// BOUND.  lb = (S + c) + tail[j + 1]: S the partial sum of the levels above, c the sibling's cost, tail the sum of the remaining
// targets' cheapest columns.  The siblings ascend in cost, so the bound fails for a suffix: the first chunk with a failing lane is
// the level's last.  A branch is cut only when lb > kth + allow, kth the cost of the last entry of a full list (+inf before):
//     allow = 2 (n + 1) eps A,      A = sum over the targets of max |cost| of the target's finite columns,  eps = 2^-52.
// Derivation: the cost of a completion and lb are float64 sums of at most n + 1 terms each over values whose magnitudes sum to at most
// A, associated differently; a recursive sum of m terms is within (m - 1) u sum |terms| (1 + O(m u)) of the exact one (u = eps / 2),
// so fl(cost) >= exact cost - n u A and fl(lb) <= exact bound + (n + 1) u A, exact bound <= exact cost: fl(lb) - fl(cost) <=
// (2 n + 1) u A < (n + 1) eps A.  The factor 2 covers the rounding of kth + allow itself and the second-order terms (n <= 32).  A
// hypothesis that ties with the K-th cost is therefore never cut, and the tuple decides at the insertion.  An allowance that is
// not finite cuts nothing.  (Departure from "1e-9 (1 + sum |cost|)": this one is derived and scales with the costs.)
//
// LIST.  One entry per lane: lane r holds the cost of rank r and the slot of its tuple; an insertion is a ballot (how many entries
// come before the new one) and a lane shift.  The tuples are 16-bit column offsets inside their targets; they live in the seam's
// workspace in global memory (K * n per cluster), not in LDS: they are written at an insertion and read back only where costs tie
// and in the epilogue.  (Departure from the issue's sketch, which had them in LDS: this keeps the launch under the 48 KB a kernel has
// without raising its limit.)
//
// Every loop is counted.  `nodes` counts sibling tests (the lanes of every chunk that hold a column); a chunk that would pass
// node_limit is not tested, the search stops and says so (MHT_KBEST_NODE_LIMIT; the list holds the best found, nodes <= node_limit).
// The walk makes at most one pop per test and one ascent per descent, and has a step bound on top.
//
// Nothing here trusts the index arrays: a cluster whose target range, target indices or column ranges fall outside the arrays, or
// that exceeds a limit, is not searched (MHT_KBEST_TOO_LARGE); a row id other than -1 outside [0, MHT_KBEST_MAX_ROWS) is never used as
// an index (MHT_KBEST_BAD_ROWS).
#pragma once
#include <math.h>
#include <stdint.h>
#include <cmath>
#include "../../include/mht_amd.h"

#if defined(__HIPCC__)
#define KB_FN __host__ __device__ __forceinline__
#else
#define KB_FN inline
#endif

namespace mht {

constexpr int KB_LANES = 64;
constexpr int KB_EMPTY = 0xFFFF;      // no row (row ids are 16-bit in LDS: MHT_KBEST_MAX_ROWS <= 0xFFFF)
static_assert(MHT_KBEST_MAX_K <= KB_LANES, "the list is one entry per lane");
static_assert(MHT_KBEST_MAX_ROWS < KB_EMPTY && MHT_KBEST_MAX_COLUMNS < 0xFFFF, "16-bit indices");

struct KbestArgs {
    int32_t nHyp, nT, nC, depth, K, node_limit;
    int32_t max_t, max_col;      // what the LDS tables are carved for: min(nT, MAX_TARGETS), min(nHyp, MAX_COLUMNS)
    const int32_t* group_ptr;
    const int32_t* rows;
    const double* cost;
    const int32_t* cluster_ptr;
    const int32_t* cluster_targets;
    int32_t* count;
    int32_t* status;
    int32_t* nodes;
    double* hyp_cost;
    double* hyp_prob;
    int32_t* hyp_sel;
    double* marginal;
    uint16_t* tuples;            // the workspace: [K * nT], cluster c owns K * n_c entries from K * cluster_ptr[c]
};

struct KbestLevel {              // the stack: a level's state while the search is below it
    double S;                    // partial sum above the level
    uint64_t mask;               // viable siblings of the level's chunk not yet descended into
    int32_t pos;                 // ranked siblings tested so far (nfin: the level is over)
    int32_t cstart;              // rank of the chunk's first sibling
    int32_t path;                // local column picked at the level
    int32_t pad;
};
struct KbestTarget {
    double tail;                 // sum of the cheapest columns of this target and those behind it
    int32_t tg;                  // the target
    int32_t g0;                  // its first global column
    int32_t base;                // its first local column
    int32_t nfin;                // its columns with a finite cost
};
struct KbestTables {             // LDS on the device (few pointers: they live in scalar registers through the search)
    double* cost;                // [max_col] the cluster's columns, targets concatenated; non-finite: +inf
    KbestLevel* lv;              // [max_t]
    KbestTarget* tt;             // [max_t + 1] (base and tail have an entry behind the last target)
    uint16_t* order;             // [max_col] rank -> local column, per target
    uint16_t* rows;              // [max_col][depth]
    uint8_t* used;               // [MHT_KBEST_MAX_ROWS] 1: a picked column holds the row
};

inline constexpr size_t kbest_round8(size_t n) { return (n + 7) / 8 * 8; }
// Bytes of the tables; every carve is a multiple of 8
inline constexpr size_t kbest_table_bytes(int max_t, int max_col, int depth) {
    return (size_t)max_col * 8 + (size_t)max_t * sizeof(KbestLevel) + ((size_t)max_t + 1) * sizeof(KbestTarget) + kbest_round8((size_t)max_col * 2) +
           kbest_round8((size_t)max_col * depth * 2) + MHT_KBEST_MAX_ROWS;
}
// Bytes of the seam's workspace: the tuples
inline constexpr size_t kbest_work_bytes(int32_t nT, int32_t K) { return ((size_t)nT * K * 2 + 255) / 256 * 256; }

KB_FN KbestTables kbest_carve(char* p, int max_t, int max_col, int depth) {
    KbestTables t;
    t.cost = reinterpret_cast<double*>(p); p += (size_t)max_col * 8;
    t.lv = reinterpret_cast<KbestLevel*>(p); p += (size_t)max_t * sizeof(KbestLevel);
    t.tt = reinterpret_cast<KbestTarget*>(p); p += ((size_t)max_t + 1) * sizeof(KbestTarget);
    t.order = reinterpret_cast<uint16_t*>(p); p += kbest_round8((size_t)max_col * 2);
    t.rows = reinterpret_cast<uint16_t*>(p); p += kbest_round8((size_t)max_col * depth * 2);
    t.used = reinterpret_cast<uint8_t*>(p);
    return t;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define KB_EACH_LANE(lane) for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define KB_PER_LANE(T, name) T name
#define KB_AT(name, lane) name
#define KB_ONE_LANE if (threadIdx.x == 0)
#define KB_SYNC()                                                 \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");    \
    } while (0)
KB_FN int kb_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
KB_FN double kb_uniform(double x) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
KB_FN uint64_t kb_ballot(bool p) { return __ballot(p); }
KB_FN int kb_any_sum(int v) {      // the sum over the wavefront
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return kb_uniform(v);
}
KB_FN double kb_lane_value(double v, int lane) { return kb_uniform(__shfl(v, lane, 64)); }
// the list's lane shift: entries p .. move one rank down, rank p takes the new one
KB_FN void kb_shift_in(double& lcost, int& lslot, int p, double c, int slot) {
    const int me = (int)threadIdx.x;
    const double pc = __shfl_up(lcost, 1, 64);
    const int ps = __shfl_up(lslot, 1, 64);
    if (me > p) {
        lcost = pc;
        lslot = ps;
    } else if (me == p) {
        lcost = c;
        lslot = slot;
    }
}
#else
#define KB_EACH_LANE(lane) for (int lane = 0; lane < KB_LANES; ++lane)
#define KB_PER_LANE(T, name) T name[KB_LANES]
#define KB_AT(name, lane) name[lane]
#define KB_ONE_LANE
#define KB_SYNC() ((void)0)
KB_FN int kb_uniform(int x) { return x; }
KB_FN double kb_uniform(double x) { return x; }
KB_FN uint64_t kb_ballot(const bool* p) {
    uint64_t m = 0;
    for (int l = 0; l < KB_LANES; ++l)
        if (p[l]) m |= 1ull << l;
    return m;
}
KB_FN int kb_any_sum(const int* v) {
    int s = 0;
    for (int l = 0; l < KB_LANES; ++l) s += v[l];
    return s;
}
KB_FN double kb_lane_value(const double* v, int lane) { return v[lane]; }
KB_FN void kb_shift_in(double* lcost, int* lslot, int p, double c, int slot) {
    for (int l = KB_LANES - 1; l > p; --l) {
        lcost[l] = lcost[l - 1];
        lslot[l] = lslot[l - 1];
    }
    lcost[p] = c;
    lslot[p] = slot;
}
#endif

KB_FN int kb_ctz(uint64_t m) { return __builtin_ctzll(m); }
KB_FN int kb_popc(uint64_t m) { return __builtin_popcountll(m); }

// Status of a cluster before any table is filled: MHT_KBEST_OK and its n targets from c0, or MHT_KBEST_TOO_LARGE.  range_ok:
// [c0, c1) lies inside cluster_targets.  n_col: its columns.  Uniform; reads cluster_ptr, cluster_targets and group_ptr only inside their bounds.
KB_FN int kbest_shape(const KbestArgs& a, int c, int& c0, int& c1, bool& range_ok, int& n, int& n_col) {
    c0 = kb_uniform(a.cluster_ptr[c]);
    c1 = kb_uniform(a.cluster_ptr[c + 1]);
    n = 0;
    n_col = 0;
    range_ok = c0 >= 0 && c1 >= c0 && c1 <= a.nT;
    if (!range_ok) return MHT_KBEST_TOO_LARGE;
    if (c1 - c0 > MHT_KBEST_MAX_TARGETS || a.depth > MHT_KBEST_MAX_DEPTH) return MHT_KBEST_TOO_LARGE;
    n = c1 - c0;
    for (int j = 0; j < n; ++j) {
        const int t = kb_uniform(a.cluster_targets[c0 + j]);
        if (t < 0 || t >= a.nT) return MHT_KBEST_TOO_LARGE;
        const int g0 = kb_uniform(a.group_ptr[t]), g1 = kb_uniform(a.group_ptr[t + 1]);
        if (g0 < 0 || g1 < g0 || g1 > a.nHyp) return MHT_KBEST_TOO_LARGE;
        n_col += g1 - g0;
        if (n_col > a.max_col) return MHT_KBEST_TOO_LARGE;      // (max_col <= MHT_KBEST_MAX_COLUMNS: what the tables are carved for)
    }
    return MHT_KBEST_OK;
}

// One cluster from the seam's arrays to its outputs.  hyp_sel and marginal are preset by the seam (-1 and 0): written here are the
// cells of the listed hypotheses, and NaN marginals for a cluster that is not searched.
KB_FN void kbest_cluster(const KbestArgs& a, const KbestTables& t, int c) {
    const int K = a.K, depth = a.depth;
    const double inf = HUGE_VAL, nan = NAN;
    int c0, c1, n, n_col;
    bool range_ok;
    int status = kbest_shape(a, c, c0, c1, range_ok, n, n_col);
    int count = 0, nodes = 0;
    KB_PER_LANE(double, lcost);      // the list: lane r holds rank r
    KB_PER_LANE(int, lslot);
    KB_EACH_LANE(lane) {
        KB_AT(lcost, lane) = nan;
        KB_AT(lslot, lane) = lane;
    }
    uint16_t* tuples = a.tuples + (size_t)K * (status == MHT_KBEST_OK ? c0 : 0);      // [K][n]
    bool feasible = status == MHT_KBEST_OK && n > 0;

    if (status == MHT_KBEST_OK && n > 0) {
        // ---- prologue: the targets, the columns' costs and rows, the ranking, the tails
        KB_ONE_LANE {
            int b = 0;
            for (int j = 0; j < n; ++j) {
                const int tj = a.cluster_targets[c0 + j];
                t.tt[j].tg = tj;
                t.tt[j].g0 = a.group_ptr[tj];
                t.tt[j].base = b;
                b += a.group_ptr[tj + 1] - a.group_ptr[tj];
            }
            t.tt[n].base = b;
        }
        KB_SYNC();
        KB_PER_LANE(bool, bad);
        KB_EACH_LANE(lane) {
            bool bd = false;
            for (int i = lane; i < MHT_KBEST_MAX_ROWS; i += KB_LANES) t.used[i] = 0;
            for (int j = 0; j < n; ++j) {
                const int b = t.tt[j].base, s = t.tt[j + 1].base - b, g = t.tt[j].g0;
                for (int i = lane; i < s; i += KB_LANES) {
                    const double v = a.cost[g + i];
                    t.cost[b + i] = fabs(v) < inf ? v : inf;      // (NaN and both infinities: never picked)
                    for (int d = 0; d < depth; ++d) {
                        const int r = a.rows[(size_t)d * a.nHyp + g + i];
                        const bool in_range = r >= 0 && r < MHT_KBEST_MAX_ROWS;
                        if (r != -1 && !in_range) bd = true;
                        t.rows[(size_t)(b + i) * depth + d] = (uint16_t)(in_range ? r : KB_EMPTY);
                    }
                }
            }
            KB_AT(bad, lane) = bd;
        }
        if (kb_ballot(bad) != 0) status = MHT_KBEST_BAD_ROWS;
        KB_SYNC();
        if (status == MHT_KBEST_OK) {
            for (int j = 0; j < n; ++j) {      // rank the target's columns by (cost, index); the finite costs come first
                const int b = kb_uniform(t.tt[j].base), s = kb_uniform(t.tt[j + 1].base) - b;
                KB_PER_LANE(int, fin);
                KB_EACH_LANE(lane) {
                    int f = 0;
                    for (int i = lane; i < s; i += KB_LANES) {
                        const double v = t.cost[b + i];
                        int rank = 0;
                        for (int k = 0; k < s; ++k) {
                            const double w = t.cost[b + k];
                            rank += (w < v || (w == v && k < i)) ? 1 : 0;
                        }
                        t.order[b + rank] = (uint16_t)(b + i);
                        f += v < inf ? 1 : 0;
                    }
                    KB_AT(fin, lane) = f;
                }
                const int nf = kb_any_sum(fin);
                KB_ONE_LANE { t.tt[j].nfin = nf; }
            }
            KB_SYNC();
        }
        feasible = status == MHT_KBEST_OK;
        double A = 0.0;
        if (feasible) {
            for (int j = 0; j < n; ++j)
                if (kb_uniform(t.tt[j].nfin) == 0) feasible = false;
        }
        if (feasible) {
            KB_ONE_LANE {
                double tl = 0.0;
                t.tt[n].tail = 0.0;
                for (int j = n - 1; j >= 0; --j) {
                    tl += t.cost[t.order[t.tt[j].base]];
                    t.tt[j].tail = tl;
                }
            }
            for (int j = 0; j < n; ++j) {
                const int b = kb_uniform(t.tt[j].base);
                const double lo = kb_uniform(t.cost[t.order[b]]), hi = kb_uniform(t.cost[t.order[b + kb_uniform(t.tt[j].nfin) - 1]]);
                A += fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi);
            }
            KB_SYNC();
        }
        const double allow = 2.0 * (double)(n + 1) * 2.220446049250313e-16 * A;

        // ---- the search
        if (feasible) {
            int j = 0, pos = 0, cstart = 0;
            uint64_t mask = 0;
            double S = 0.0, thr = inf;      // thr = kth + allow
            // (a search of more than 2^32 steps ends as one that met its node limit)
            const uint64_t want_steps = 4 * (uint64_t)a.node_limit + 4 * (uint64_t)n + 64;
            const uint32_t max_steps = want_steps < 0xFFFFFFFFull ? (uint32_t)want_steps : 0xFFFFFFFFu;
            bool done = false;
            for (uint32_t step = 0; step < max_steps; ++step) {
                const int b = kb_uniform(t.tt[j].base), nf = kb_uniform(t.tt[j].nfin);
                const double tl = kb_uniform(t.tt[j + 1].tail);
                if (mask == 0) {
                    if (pos >= nf) {      // the level is over: back to the level above, its column gives its rows back
                        if (j == 0) {
                            done = true;
                            break;
                        }
                        --j;
                        const int col = kb_uniform(t.lv[j].path);
                        KB_EACH_LANE(lane) {
                            if (lane < depth) {
                                const int r = t.rows[(size_t)col * depth + lane];
                                if (r != KB_EMPTY) t.used[r] = 0;
                            }
                        }
                        pos = kb_uniform(t.lv[j].pos);
                        cstart = kb_uniform(t.lv[j].cstart);
                        mask = t.lv[j].mask;
#if defined(__HIP_DEVICE_COMPILE__)
                        mask = ((uint64_t)(uint32_t)kb_uniform((int)(mask >> 32)) << 32) | (uint32_t)kb_uniform((int)(mask & 0xffffffffu));
#endif
                        S = kb_uniform(t.lv[j].S);
                        KB_SYNC();
                        continue;
                    }
                    const int cnt = nf - pos < KB_LANES ? nf - pos : KB_LANES;      // a chunk of siblings
                    if (a.node_limit - nodes < cnt) break;      // (not done: the node limit)
                    nodes += cnt;
                    KB_PER_LANE(bool, viable);
                    KB_PER_LANE(bool, cut);
                    KB_EACH_LANE(lane) {
                        bool v = false, ct = false;
                        if (lane < cnt) {
                            const int col = t.order[b + pos + lane];
                            const double lb = (S + t.cost[col]) + tl;
                            ct = lb > thr;
                            bool clash = false;
                            for (int d = 0; d < depth; ++d) {
                                const int r = t.rows[(size_t)col * depth + d];
                                if (r != KB_EMPTY && t.used[r]) clash = true;
                            }
                            v = !ct && !clash;
                        }
                        KB_AT(viable, lane) = v;
                        KB_AT(cut, lane) = ct;
                    }
                    mask = kb_ballot(viable);
                    cstart = pos;
                    pos = kb_ballot(cut) != 0 ? nf : pos + cnt;      // (the bound fails for a suffix of the siblings)
                    continue;
                }
                const int l = kb_ctz(mask);
                mask &= mask - 1;
                const int col = kb_uniform((int)t.order[b + cstart + l]);
                const double cc = kb_uniform(t.cost[col]);
                if ((S + cc) + tl > thr) {      // the list has moved since the chunk was tested: this sibling and all behind it are cut
                    mask = 0;
                    pos = nf;
                    continue;
                }
                if (j == n - 1) {      // a hypothesis: where does it rank?
                    const double total = S + cc;
                    KB_PER_LANE(bool, before);
                    KB_PER_LANE(bool, tie);
                    KB_EACH_LANE(lane) {
                        KB_AT(before, lane) = lane < count && KB_AT(lcost, lane) < total;
                        KB_AT(tie, lane) = lane < count && KB_AT(lcost, lane) == total;
                    }
                    if (kb_ballot(tie) != 0) {      // equal costs: the tuple decides
                        KB_SYNC();      // (the tuples written by earlier insertions)
                        KB_EACH_LANE(lane) {
                            (void)lane;
                            if (KB_AT(tie, lane)) {
                                const uint16_t* mine = tuples + (size_t)KB_AT(lslot, lane) * n;
                                bool less = false;
                                for (int k = 0; k < n; ++k) {
                                    const int theirs = (k == n - 1 ? col : t.lv[k].path) - t.tt[k].base;
                                    if ((int)mine[k] != theirs) {
                                        less = (int)mine[k] < theirs;
                                        break;
                                    }
                                }
                                KB_AT(before, lane) = less;
                            }
                        }
                    }
                    const int p = kb_popc(kb_ballot(before));
                    if (p < K) {
                        int slot = count;
                        if (count == K) {
                            KB_PER_LANE(int, last);
                            KB_EACH_LANE(lane) { KB_AT(last, lane) = lane == K - 1 ? KB_AT(lslot, lane) : 0; }
                            slot = kb_any_sum(last);      // the evicted entry's
                        } else {
                            ++count;
                        }
                        kb_shift_in(lcost, lslot, p, total, slot);
                        KB_EACH_LANE(lane) {
                            if (lane < n) tuples[(size_t)slot * n + lane] = (uint16_t)((lane == n - 1 ? col : t.lv[lane].path) - t.tt[lane].base);
                        }
                        if (count == K) thr = kb_lane_value(lcost, K - 1) + allow;
                    }
                    continue;
                }
                // descend: the column takes its rows, the level's state goes to the stack
                KB_ONE_LANE {
                    t.lv[j].path = col;
                    t.lv[j].pos = pos;
                    t.lv[j].cstart = cstart;
                    t.lv[j].mask = mask;
                    t.lv[j].S = S;
                }
                KB_EACH_LANE(lane) {
                    if (lane < depth) {
                        const int r = t.rows[(size_t)col * depth + lane];
                        if (r != KB_EMPTY) t.used[r] = 1;
                    }
                }
                KB_SYNC();
                S = S + cc;
                ++j;
                pos = 0;
                cstart = 0;
                mask = 0;
            }
            if (!done) status = MHT_KBEST_NODE_LIMIT;
        }
    }
    if (status != MHT_KBEST_OK && status != MHT_KBEST_NODE_LIMIT) {
        count = 0;
        nodes = 0;
    }

    // ---- epilogue: the weights in ascending rank, the listed cells, the marginals
    KB_SYNC();
    KB_PER_LANE(double, w);
    const double best = count > 0 ? kb_lane_value(lcost, 0) : 0.0;
    KB_EACH_LANE(lane) { KB_AT(w, lane) = lane < count ? exp(-(KB_AT(lcost, lane) - best)) : 0.0; }
    double Z = 0.0;
    for (int r = 0; r < count; ++r) Z += kb_lane_value(w, r);
    KB_EACH_LANE(lane) {
        if (lane < K) {
            a.hyp_cost[(size_t)lane * a.nC + c] = lane < count ? KB_AT(lcost, lane) : nan;
            a.hyp_prob[(size_t)lane * a.nC + c] = lane < count ? KB_AT(w, lane) / Z : nan;
        }
        KB_AT(w, lane) = lane < count ? KB_AT(w, lane) / Z : 0.0;
    }
    if (status == MHT_KBEST_OK || status == MHT_KBEST_NODE_LIMIT) {
        for (int r = 0; r < count; ++r) {      // (ascending rank: every marginal is one sum in a fixed order)
            const double pr = kb_lane_value(w, r);
            KB_PER_LANE(int, rs);
            KB_EACH_LANE(lane) { KB_AT(rs, lane) = lane == r ? KB_AT(lslot, lane) : 0; }
            const int slot = kb_any_sum(rs);
            KB_EACH_LANE(lane) {
                if (lane < n) {
                    const int g = t.tt[lane].g0 + (int)tuples[(size_t)slot * n + lane];
                    a.hyp_sel[(size_t)r * a.nT + t.tt[lane].tg] = g;
                    a.marginal[g] += pr;
                }
            }
        }
    } else if (range_ok) {      // not searched: the marginals of its columns are unknown (every index is checked again: nothing was)
        for (int j = c0; j < c1; ++j) {
            const int tj = kb_uniform(a.cluster_targets[j]);
            if (tj < 0 || tj >= a.nT) continue;
            const int g0 = kb_uniform(a.group_ptr[tj]), g1 = kb_uniform(a.group_ptr[tj + 1]);
            if (g0 < 0 || g1 < g0 || g1 > a.nHyp) continue;
            KB_EACH_LANE(lane) {
                for (int i = g0 + lane; i < g1; i += KB_LANES) a.marginal[i] = nan;
            }
        }
    }
    KB_ONE_LANE {
        a.count[c] = count;
        a.status[c] = status;
        a.nodes[c] = nodes;
    }
}

}  // namespace mht
