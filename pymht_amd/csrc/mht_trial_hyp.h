// Trial manoeuvres against every live hypothesis of every target (mht_trial_hypotheses, include/mht_amd.h).  The entries are the L
// leaves of the forest in target order; the leaves of target t are seg[t] .. seg[t + 1] - 1 (an empty target is allowed).  A cell
// (g, l) is encounter_pair of candidate g against leaf l: the leaf propagated by encounter_propagate<N> (through trial_track<N>), the
// candidate's path from trial_candidate, all three as they stand in mht_encounter.h and mht_trial.h -- so the table [5][G][L] is bit
// for bit what mht_trial_manoeuvres gives for n = L.  What this header adds is the SEGMENTED fold of a candidate's row, per target;
// the code a lane of the kernels of mht_trial_hyp.hip runs, and tests/hostmath/trial_hyp_host.cpp on the CPU.
//
// THE WEIGHTS, per target t, independent of the candidate (hyp_weights).  cnllr_l is the cumulative NLLR of leaf l; a LOWER one is the
// better hypothesis.  cmin_t is the smallest cnllr of the segment that is not NaN, and
//   w_l = exp(-(cnllr_l - cmin_t)),   weight_l = w_l / sum(w)       the sum over the leaves with a cnllr, serially in leaf order.
// A leaf whose cnllr is NaN has w_l = NaN and weight_l = NaN; a +inf cnllr gives w_l = 0 exactly (and a segment whose every cnllr is
// +inf gives inf - inf, NaN throughout).  A target of one leaf has w = exp(-0.0) = 1 exactly.
//
// THE FIGURES, per (g, t), over the leaves of the segment -- fig [8][G][T] in this order:
//   0 pcWorst, 1 pcWorstLeaf   the largest pc and its leaf, as a GLOBAL leaf index
//   2 dcpaMin, 3 dcpaMinLeaf   the smallest dcpa and its leaf
//                              both by trial_fold: a NaN figure takes no part, equal figures go to the lowest leaf, no figure gives NaN
//                              and -1.  That order is total: these four are the same bits in any grouping
//   4 pcMean                   sum(w_l pc_l) / sum(w_l) over the leaves whose pc_l and w_l are both not NaN; NaN where the second sum is
//                              not positive (no such leaf, or every such leaf's weight underflowed).  With one leaf: 1 * pc / 1 = pc,
//                              bit for bit
//   5 pcSel, 6 dcpaSel, 7 tcpaSel   the cell of leaf sel[t], a global index inside the segment: what the best-hypothesis view reports.
//                              NaN where sel[t] = -1
//
// THE APPROXIMATION.  The weights normalise INSIDE ONE TARGET.  The exclusion constraints between targets, which the ILP enforces (two
// targets cannot both take one plot), are ignored: w_l / sum(w) is the usual track-oriented approximation of a hypothesis' probability,
// not the probability of a global hypothesis.  pcMean is the mean of pc under those weights and nothing else.
//
// THE ORDER OF THE SUMS (the library is compiled with -ffp-contract=off; tests/trial_hyp_ref.py restates it).  A tile is 256
// consecutive leaves (TRIAL_TILE); a PIECE is the part of a segment inside one tile.  Both sums start at 0.0; a piece adds its leaves
// serially in leaf order (w_l * pc_l, and w_l); a target adds its pieces in tile order.  Every term is >= 0.  A piece of target t in
// tile c has slot c + t of a row of tiles + T slots: along the pieces of a row c or t or both grow at every step, so no two pieces share
// a slot, and a slot without a piece is never read.
#pragma once
#include "mht_trial.h"

namespace mht {

constexpr int HYP_FIGURES = 8;      // fig [8][G][T]
constexpr int HYP_PARTIAL = 6;      // partials [6][G][tiles + T]: pc, its leaf, dcpa, its leaf, sum w pc, sum w

// What the fold of a piece or of a target keeps
struct HypPart {
    TrialBest b;
    double spw, sw;
};

MHT_HD HypPart hyp_none() { return HypPart{trial_none(), 0.0, 0.0}; }

// a <- a with leaf j folded in: its pc and dcpa, and its weight w (NaN: the leaf has none)
MHT_HD void hyp_fold_leaf(HypPart& a, double pc, double dcpa, double w, int j) {
    trial_fold(a.b, trial_cell_best(pc, dcpa, j));
    const bool in = pc == pc && w == w;
    a.spw = in ? a.spw + w * pc : a.spw;
    a.sw = in ? a.sw + w : a.sw;
}

// a <- a with the later piece b folded in
MHT_HD void hyp_fold_part(HypPart& a, const HypPart& b) {
    trial_fold(a.b, b.b);
    a.spw = a.spw + b.spw;
    a.sw = a.sw + b.sw;
}

MHT_HD void hyp_store(const HypPart& a, double* q, size_t stride) {
    trial_store(a.b, q, stride);
    q[4 * stride] = a.spw;
    q[5 * stride] = a.sw;
}

MHT_HD HypPart hyp_load(const double* q, size_t stride) { return HypPart{trial_load(q, stride), q[4 * stride], q[5 * stride]}; }

// Target t: wl [L] and weight [L] of its leaves, and target_of [L] = t
MHT_HD void hyp_weights(const double* cnllr, const int32_t* seg, int t, double* wl, double* weight, int32_t* target_of) {
    const double nan = __builtin_nan("");
    const int a = seg[t], e = seg[t + 1];
    double cmin = nan;
    for (int l = a; l < e; ++l) {
        const double c = cnllr[l];
        cmin = c == c && !(cmin <= c) ? c : cmin;
    }
    double sum = 0.0;
    for (int l = a; l < e; ++l) {
        const double c = cnllr[l];
        const double w = c == c ? exp(-(c - cmin)) : nan;
        wl[l] = w;
        sum = c == c ? sum + w : sum;
        target_of[l] = t;
    }
    for (int l = a; l < e; ++l) weight[l] = wl[l] / sum;
}

// Cell (g, l): candidate g is entry L + g of L + G.  o5 = tcpa, dcpa, md2, pc, tpc; stored to table [5][G][L] where there is one.
MHT_HD void hyp_cell(const double* pos, const double* S, int L, int G, int K, double dt, double R, int g, int l, double* table, double* o5) {
    encounter_pair(pos, S, L + G, K, dt, R, L + g, l, o5);
    if (table) {
        double* cell = table + (size_t)g * (size_t)L + l;
#pragma unroll
        for (int f = 0; f < ENCOUNTER_FIGURES; ++f) cell[(size_t)f * (size_t)G * (size_t)L] = o5[f];
    }
}

// The cell of the selected leaf of target t into rows 5 .. 7 of fig [8][G][T]
MHT_HD void hyp_store_selected(const double* o5, int G, int T, int g, int t, double* fig) {
    double* q = fig + (size_t)g * (size_t)T + t;
    const size_t row = (size_t)G * (size_t)T;
    q[5 * row] = o5[3];
    q[6 * row] = o5[1];
    q[7 * row] = o5[0];
}

// The piece that begins at lane `lane` of a tile whose first leaf is `base`: pc, dcpa and w are the tile's [TRIAL_TILE] arrays, `end` is
// the end of the leaf's segment.  Serially, in leaf order.
MHT_HD HypPart hyp_piece(const double* pc, const double* dcpa, const double* w, int base, int lane, int end) {
    HypPart a = hyp_none();
    for (int i = lane; i < TRIAL_TILE && base + i < end; ++i) hyp_fold_leaf(a, pc[i], dcpa[i], w[i], base + i);
    return a;
}

// Target t of candidate g: its pieces in tile order out of partials [6][G][slots], slots = tiles + T, into rows 0 .. 4 of fig; and NaN
// into rows 5 .. 7 where the target has no selected leaf (where it has one, the cell's own lane has written them)
MHT_HD void hyp_target(const double* partials, const int32_t* seg, const int32_t* sel, int G, int T, size_t slots, int g, int t, double* fig) {
    const double nan = __builtin_nan("");
    const int a = seg[t], e = seg[t + 1];
    const size_t stride = (size_t)G * slots;
    HypPart p = hyp_none();
    if (e > a)
        for (int c = a / TRIAL_TILE; c <= (e - 1) / TRIAL_TILE; ++c) hyp_fold_part(p, hyp_load(partials + (size_t)g * slots + c + t, stride));
    double* q = fig + (size_t)g * (size_t)T + t;
    const size_t row = (size_t)G * (size_t)T;
    trial_store(p.b, q, row);
    q[4 * row] = p.sw > 0.0 ? p.spw / p.sw : nan;
    if (sel[t] < 0) {
        q[5 * row] = nan;
        q[6 * row] = nan;
        q[7 * row] = nan;
    }
}

}  // namespace mht
