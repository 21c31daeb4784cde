"""GPU: `mht_encounters`, `mht_trial_manoeuvres` and `mht_trial_hypotheses` where their grids stride.  Every launch of the three seams is
capped at 2048 workgroups of 256 lanes with a grid-stride loop for the rest, and the other GPU tests of these seams (at most 600 entries,
5 candidates) end inside the first trip of every loop.  The code round the per-lane arithmetic -- the tile indexing, the strided loops,
the LDS fold reused from trip to trip, the layout of the partials, the summary kernel's lane stride -- exists on the device only; the
cases here (tests/encounter_stride_util.py) are the smallest that reach each of those paths:

    E1  n = first = 683            3 chunks, 2049 tiles: encounter_pair_kernel makes a second trip
    E2  n = 524 588, first = 1     encounter_propagate_kernel's second trip covers two workgroups; row 0 spans 2050 tiles
    T1  n = 524 588, G = 1         trial_propagate_kernel and trial_cell_kernel stride; 2050 chunks, so a lane of trial_summary_kernel
                                   takes 33 of them; the row's extremes tied between chunks c and c + 64 (one lane) and 63 and 64 (two)
    T2  n = 257, G = 1025          2050 tiles, g changes from trip to trip, chunk 1 has one live lane; five workgroups of candidates
    T3  n = 1, G = 4096            every tile has one live lane, a cell workgroup makes two trips, trial_summary_kernel's grid strides
    H1  L = 513, T = 4, G = 683    segments of 250, 12, 250 and 1 leaves: 3 chunks, 2049 tiles of hyp_cell_kernel
    H2  L = T = 129, G = 4096      528 384 (candidate, target): hyp_target_kernel strides
    H3  L = 524 588, T = 524 573, G = 1   hyp_weight_kernel (a target a lane) and hyp_propagate_kernel (a leaf a lane) stride

The criterion is the project's, test_encounter_cpu.hold as the 70-entry cell cases use it: per figure e = max |got - truth| / (1 + |truth|)
<= 8 max(e_np, eps64) against the np.longdouble truth (pc: the float64 rule on the longdouble d_k and Sigma_k, with e_np from the mpmath
case), the NaN cells and the exact zeros of pc the truth's exactly, tpc by encounter_ref.hold_tpc; no cell is left out.  With G in the
thousands the candidates are trial_ref.CANDIDATES repeated cyclically: the rows of equal candidates must be bit-identical, one row of
each is held to the reference, and the summary is trial_ref.fold of the device's whole table bit for bit.  Every raw call presets its
outputs to a sentinel, none of which may be left, and has 4 KB of a pattern behind the work buffer the sizer asks for, which must be
untouched: an overrun from a wrong stride lands there.

The Monte-Carlo and the NEES launches, which have the same cap, are held in tests/test_mc_strides_gpu.py and test_nees_strides_gpu.py.

Every test prints the device's ratios, the time of the seam's call and the time of its reference; profiles/encounter_stride_shapes.txt
records them -- measured on an MI355X, tcpa / dcpa / md2 / pc:
    E1 1 / 1 / 1 / 2.05    E2 1 / 1 / 1 / 0.22    T1 1 / 1 / 1 / 0.72    T2 1 / 1 / 1 / 0.59    T3 0 / 1 / 1 / 0.48
    H1 1 / 1 / 1 / 0.31 (pcMean 5.2e-5 and weight 0.012 of property 8's bound)    H2 1 / 1 / 1 / 1.01
each call 1 .. 2 ms on the device; the references of the whole file 13 s, and 29 s more for the mpmath cases where the process has not
computed them already."""
import contextlib
import time

import numpy as np
import pytest

import encounter_ref as eref
import encounter_stride_util as u
import trial_ref as tref
from test_encounter_cpu import RADIUS, hold, pc_case
from test_encounter_gpu import SENTINEL
from test_encounter_gpu import _raw as raw_encounters
from test_trial_cpu import check_summary, mp_case
from test_trial_gpu import _raw as raw_trial
from test_encounter_strides_cpu import live_in_every_place
from test_trial_hyp_cpu import check_figures
from test_trial_hyp_gpu import _raw as raw_hyp

pytestmark = pytest.mark.gpu

GUARD = 4096
DT, K = u.DT, u.K


@pytest.fixture(scope="module")
def ctxs():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (pymht_amd has no CPU fallback)")
    from pymht_amd.device import Context
    c = {4: Context(0, nx=4), 6: Context(0, nx=6)}
    yield c
    for v in c.values():
        v.close()


@contextlib.contextmanager
def seam_time(label, ctx, name):
    """Prints the wall time spent inside the library's `name` (the seam returns after its stream has drained)"""
    inner, spent = getattr(ctx.lib, name), []

    def timed(*args):
        t = time.perf_counter()
        rc = inner(*args)
        spent.append(time.perf_counter() - t)
        return rc
    setattr(ctx.lib, name, timed)
    try:
        yield
    finally:
        setattr(ctx.lib, name, inner)
        print("%s: %s took %s ms" % (label, name, ", ".join("%.2f" % (1e3 * s) for s in spent)))


def reference(label, make):
    """make() and the seconds it took, printed (0 when another test of the process has computed it already)"""
    t = time.perf_counter()
    res = make()
    print("%s: reference %.1f s" % (label, time.perf_counter() - t))
    return res


def trial_scale(N):
    """e_np of pc for the trial seams: the smaller of the two mpmath cases' (the encounters' and the trial manoeuvres')"""
    return min(pc_case(N)[8], mp_case(N)[9])


def first_of_each(kind):
    return np.array([int(np.flatnonzero(kind == k)[0]) for k in range(len(tref.CANDIDATES))])


def equal_rows_are_identical(arr, kind):
    """arr [F, G, ...]: the rows of one candidate are the bits of its first"""
    for k in np.unique(kind):
        rows = arr[:, kind == k]
        assert np.array_equal(rows, np.broadcast_to(rows[:, :1], rows.shape), equal_nan=True), "rows of candidate %d differ" % k


# ---- encounters ----------------------------------------------------------------------------------------------------------------------
def test_e1_all_pairs_of_683_entries_the_pair_kernel_strides(ctxs):
    """E1, models/pv on the four-state build: 3 chunks and 2049 tiles.  Every cell to the truth, the special pairs, and the rows of a
    first = 3 call (9 tiles, one trip) are the first three rows of the full call bit for bit."""
    assert np.finfo(np.longdouble).eps < 1e-18
    label = "E1 n 683 first 683, pv, 4-state build"
    x, P, Phi, Q, f64, truth = reference(label, lambda: u.e1(4))
    with seam_time(label, ctxs[4], "mht_encounters"):
        rc, out = raw_encounters(ctxs[4], x, P, Phi, Q, K, DT, RADIUS, guard=GUARD)
    assert rc == 0 and not (out == SENTINEL).any()
    got = eref.seam_dict(out)
    hold(label, got, truth, f64, DT, pc_scale=pc_case(4)[8])
    eref.check_special_cells(got, K, DT)
    rc, part = raw_encounters(ctxs[4], x, P, Phi, Q, K, DT, RADIUS, first=3, guard=GUARD)
    assert rc == 0 and part.shape == (5, 3, u.E1_N) and np.array_equal(part, out[:, :3], equal_nan=True)


def test_e2_one_row_of_524588_entries_the_propagate_kernel_strides(ctxs):
    """E2, models/ca on the six-state build: the propagate kernel's second trip covers entries 524 288 .. 524 587 (two workgroups), row 0
    spans 2050 tiles, the last of them with 44 live lanes.  Every cell of the row to the truth; the planted entries -- tile 0, round
    256, round 524 288, the last tile -- are the cells with a pc."""
    label = "E2 n 524588 first 1, ca, 6-state build"
    x, P, Phi, Q, f64, truth = reference(label, lambda: u.e2(6))
    with seam_time(label, ctxs[6], "mht_encounters"):
        rc, out = raw_encounters(ctxs[6], x, P, Phi, Q, K, DT, RADIUS, first=1, guard=GUARD)
    assert rc == 0 and out.shape == (5, 1, u.BIG) and not (out == SENTINEL).any()
    got = eref.seam_dict(out)
    hold(label, got, truth, f64, DT, pc_scale=pc_case(6)[8])
    assert np.isnan(out[:, 0, 0]).all() and np.isnan(out[:, 0, u.NAN_ENTRY]).all()
    assert all(int(np.sum(got["pc"][0, m] > 0)) >= min(64, int(m.sum())) for m in u.places().values())


# ---- trial manoeuvres ----------------------------------------------------------------------------------------------------------------
def test_t1_one_candidate_against_524588_tracks_and_ties_across_the_summarys_lanes(ctxs):
    """T1, models/pv on the six-state build: propagate, cell and summary all stride (2050 chunks: 33 trips a lane of the summary).  The
    row to the truth; the summary is the fold of the device's own row bit for bit; the largest pc and the smallest dcpa are each held by
    two identical tracks in chunks c and c + 64 -- the same lane of the summary -- and the summary names the lower; then the same
    tracks in chunks 63 and 64, two lanes."""
    label = "T1 n 524588 G 1, pv, 6-state build"
    x, P, Phi, Q, own, Sown, f64, truth = reference(label, lambda: u.t1(4))
    scale = trial_scale(4)
    for ties, perm in ((u.TIES_SAME_LANE, None), (u.TIES_TWO_LANES, u.t1_swap())):
        xs, Ps, fs, ts = (x, P, f64, truth) if perm is None else (x[perm], P[perm], u.permuted(f64, perm), u.permuted(truth, perm))
        with seam_time(label, ctxs[6], "mht_trial_manoeuvres"):
            rc, out, summary = raw_trial(ctxs[6], xs, Ps, Phi, Q, K, DT, RADIUS, own, Sown, tref.TURN_RATE, u.T1_CANDIDATE, guard=GUARD)
        assert rc == 0 and not (out == SENTINEL).any() and not (summary == SENTINEL).any()
        got = eref.seam_dict(out)
        hold(label + (", ties in chunks %d and %d" % (ties[0][0] // u.TILE, ties[0][1] // u.TILE)), got, ts, fs, DT, pc_scale=scale)
        check_summary(summary, got)
        (p1, p2), (d1, d2) = ties
        assert got["pc"][0, p1] == got["pc"][0, p2] == np.nanmax(got["pc"]) and got["dcpa"][0, d1] == got["dcpa"][0, d2] == np.nanmin(got["dcpa"])
        assert summary[:, 0].tolist() == [got["pc"][0, p1], p1, got["dcpa"][0, d1], d1], summary[:, 0]
        assert all(int(np.sum(got["pc"][0, m] > 0)) >= min(64, int(m.sum())) for m in u.places().values())


def held_rows(label, ctx, N, scene, key):
    """One call on a scene of cyclic candidates: no sentinel left, equal candidates give identical rows, one row of each candidate under
    the criterion, the summary the fold of the whole table; returns (out, summary, kind)"""
    x, P, Phi, Q, own, Sown, cand, kind = scene
    f64, truth = reference(label, lambda: u.distinct_rows(x, P, Phi, Q, own, Sown, key))
    with seam_time(label, ctx, "mht_trial_manoeuvres"):
        rc, out, summary = raw_trial(ctx, x, P, Phi, Q, K, DT, RADIUS, own, Sown, tref.TURN_RATE, cand, guard=GUARD)
    assert rc == 0 and out.shape == (5, len(cand), len(x)) and not (out == SENTINEL).any() and not (summary == SENTINEL).any()
    equal_rows_are_identical(out, kind)
    equal_rows_are_identical(summary, kind)
    hold(label, eref.seam_dict(out[:, first_of_each(kind)]), truth, f64, DT, pc_scale=trial_scale(N))
    check_summary(summary, eref.seam_dict(out))
    return out, summary, kind


def test_t2_1025_candidates_against_257_tracks_the_cell_kernel_strides_over_g(ctxs):
    """T2, models/ca on the four-state build: 2 chunks and 2050 tiles, so that g changes from trip to trip and the partials of 1025 rows
    lie side by side; chunk 1 has one live lane; the candidates take five workgroups; a NaN candidate's row is NaN, its summary NaN
    and -1."""
    out, summary, kind = held_rows("T2 n 257 G 1025, ca, 4-state build", ctxs[4], 6, u.t2_scene(6), ("t2", 6))
    assert kind[u.T2_NAN] == -1 and np.isnan(out[:, u.T2_NAN]).all() and np.isnan(summary[[0, 2], u.T2_NAN]).all() and (summary[[1, 3], u.T2_NAN] == -1).all()
    assert not np.isnan(summary[:, kind >= 0]).any() and int(np.sum(out[3, -1] > 0)) >= 20 and not np.isnan(out[1, kind >= 0, 256]).any()


def test_t3_4096_candidates_against_one_track_the_summary_grid_strides(ctxs):
    """T3, models/pv on the four-state build: 4096 tiles of one live lane, two trips a cell workgroup, two a summary workgroup"""
    out, summary, kind = held_rows("T3 n 1 G 4096, pv, 4-state build", ctxs[4], 4, u.t3_scene(4), ("t3", 4))
    assert (out[3] > 0).all() and (summary[1] == 0).all() and (summary[3] == 0).all() and len(np.unique(out[1])) >= 3 and len(np.unique(out[3])) >= 3 and (out[3] < 0.99).all()


# ---- trial hypotheses ----------------------------------------------------------------------------------------------------------------
def held_hypotheses(label, ctx, N, scene, key):
    """One call on a scene of cyclic candidates: the table is mht_trial_manoeuvres' bit for bit and one row of each candidate meets the
    criterion; equal candidates give identical rows of table and fig, and check_figures holds on one row of each (hence on all); a
    table = NULL call gives the same fig and weight bits.  Returns (table, fig, weight)."""
    x, P, cnllr, seg, sel, own, Sown, Phi, Q, cand, kind = scene
    args = (Phi, Q, K, DT, RADIUS, own, Sown, tref.TURN_RATE)
    f64, truth = reference(label, lambda: u.distinct_rows(x, P, Phi, Q, own, Sown, key))
    with seam_time(label, ctx, "mht_trial_hypotheses"):
        rc, table, fig, weight, _ = raw_hyp(ctx, x, P, cnllr, seg, sel, *args, cand, guard=GUARD)
    assert rc == 0 and not (table == SENTINEL).any() and not (fig == SENTINEL).any() and not (weight == SENTINEL).any()
    rc, out, _ = raw_trial(ctx, x, P, *args, cand, guard=GUARD)
    assert rc == 0 and np.array_equal(table, out, equal_nan=True)
    equal_rows_are_identical(table, kind)
    equal_rows_are_identical(fig, kind)
    rows = first_of_each(kind)
    hold(label, eref.seam_dict(table[:, rows]), truth, f64, DT, pc_scale=trial_scale(N))
    t = time.perf_counter()
    check_figures(label, fig[:, rows], weight, table[:, rows], cnllr, seg, sel)
    print("%s: check_figures %.1f s" % (label, time.perf_counter() - t))
    rc, _, bare, bw, untouched = raw_hyp(ctx, x, P, cnllr, seg, sel, *args, cand, table=False, guard=GUARD)
    assert rc == 0 and np.array_equal(bare, fig, equal_nan=True) and np.array_equal(bw, weight, equal_nan=True) and (untouched == SENTINEL).all()
    return table, fig, weight


def test_h1_683_candidates_against_513_leaves_in_four_targets(ctxs):
    """H1, models/ca on the six-state build: 3 chunks and 2049 tiles; a target of 12 leaves straddles leaf 256, one of 250 ends exactly at
    512, one of a single leaf begins the third tile alone; cnllr as make_leaves draws it with its special leaves; a target without a
    selected leaf."""
    scene = u.h1_scene(6)
    seg, sel = scene[3], scene[4]
    assert seg.tolist() == [0, 250, 262, 512, 513] and sel[u.H1_NO_SELECTED] == -1 and all(seg[t] <= sel[t] < seg[t + 1] for t in (0, 1, 3))
    table, fig, weight = held_hypotheses("H1 L 513 T 4 G 683, ca, 6-state build", ctxs[6], 6, scene, ("h1", 6))
    assert np.isnan(fig[5:, :, u.H1_NO_SELECTED]).all() and not np.isnan(fig[:5]).any() and not np.isnan(fig[5:, :, [0, 1, 3]]).any()
    assert np.isnan(weight[140]) and weight[141] == 0.0 and np.isnan(table[:, :, 70]).all() and int(np.sum(table[3] > 0)) >= 50000


def test_h2_4096_candidates_against_129_targets_of_one_leaf_the_target_kernel_strides(ctxs):
    """H2, models/pv on the four-state build: 528 384 (g, t) cells of hyp_target_kernel.  Property 4 of tests/test_trial_hyp_gpu.py: with
    one leaf a target pcMean == pcWorst == pcSel == the table's pc bit for bit, and so the other figures."""
    scene = u.h2_scene(4)
    assert np.array_equal(scene[4], np.arange(u.H2_L)) and np.array_equal(scene[3], np.arange(u.H2_L + 1))
    table, fig, weight = held_hypotheses("H2 L 129 T 129 G 4096, pv, 4-state build", ctxs[4], 4, scene, ("h2", 4))
    leaf = np.tile(np.arange(u.H2_L), (u.H2_G, 1))
    assert all(np.array_equal(fig[f], table[3], equal_nan=True) for f in (0, 4, 5)) and (weight == 1.0).all()
    assert np.array_equal(fig[2], table[1], equal_nan=True) and np.array_equal(fig[6], table[1], equal_nan=True) and np.array_equal(fig[7], table[0], equal_nan=True)
    assert np.array_equal(fig[1], np.where(np.isnan(table[3]), -1, leaf)) and np.array_equal(fig[3], np.where(np.isnan(table[1]), -1, leaf))
    assert int(np.sum(table[3] > 0)) >= 64 * 20


def test_h3_524573_targets_the_weight_and_the_propagate_kernel_stride(ctxs):
    """H3, models/pv on the four-state build, table = NULL: 524 588 leaves of 524 573 targets, G = 1, K = 1.  hyp_weight_kernel's second
    trip is targets 524 288 .. 524 572, ten of them with two or three leaves of different cnllr; hyp_propagate_kernel's is leaves
    524 288 .. 524 587, planted beside the own ship.  The criterion is held_hypotheses' with the table taken from mht_trial_manoeuvres
    on the same leaves (the call has none): that table to the truth, every cell; check_figures -- whose fold is a Python loop over the
    targets -- on the targets from 524 280 on, the leaves 524 280 .. 524 587 with all the targets of several leaves among them; and
    for the 524 280 targets of one leaf before them property 4 on the whole rows, bit for bit: every figure is the leaf's cell, the
    weight is 1."""
    label = "H3 L 524588 T 524573 G 1, pv, 4-state build"
    x, P, cnllr, seg, sel, own, Sown, Phi, Q, cand, f64, truth = reference(label, lambda: u.h3(4))
    ctx, args = ctxs[4], (Phi, Q, K, DT, RADIUS, own, Sown, tref.TURN_RATE)
    with seam_time(label, ctx, "mht_trial_hypotheses"):
        rc, _, fig, weight, untouched = raw_hyp(ctx, x, P, cnllr, seg, sel, *args, cand, table=False, guard=GUARD)
    assert rc == 0 and not (fig == SENTINEL).any() and not (weight == SENTINEL).any() and (untouched == SENTINEL).all()
    rc, table, _ = raw_trial(ctx, x, P, *args, cand, guard=GUARD)
    assert rc == 0 and not (table == SENTINEL).any()
    got = eref.seam_dict(table)
    hold(label, got, truth, f64, DT, pc_scale=trial_scale(4))
    live_in_every_place(got["pc"][0])
    # the targets of one leaf in front: leaf l is target l
    t0 = 524280
    assert np.array_equal(seg[:t0 + 1], np.arange(t0 + 1)) and t0 < u.H3_MULTI[0] and np.isfinite(cnllr).all()
    leaf = np.arange(t0)
    nan = lambda row: np.isnan(row[0, :t0])
    assert all(np.array_equal(fig[f][:, :t0], table[3][:, :t0], equal_nan=True) for f in (0, 4, 5)) and (weight[:t0] == 1.0).all()
    assert np.array_equal(fig[2][:, :t0], table[1][:, :t0], equal_nan=True) and np.array_equal(fig[6][:, :t0], table[1][:, :t0], equal_nan=True)
    assert np.array_equal(fig[7][:, :t0], table[0][:, :t0], equal_nan=True)
    assert np.array_equal(fig[1][0, :t0], np.where(nan(table[3]), -1, leaf)) and np.array_equal(fig[3][0, :t0], np.where(nan(table[1]), -1, leaf))
    # the rest, behind the threshold but for eight leaves: the fold in np.longdouble, with the leaves numbered from t0 on
    t = time.perf_counter()
    tail = fig[:, :, t0:].copy()
    for f in (1, 3):
        tail[f] = np.where(tail[f] >= 0, tail[f] - t0, tail[f])
    r_mean, r_weight = check_figures(label, tail, weight[t0:], table[:, :, t0:], cnllr[t0:], seg[t0:] - t0, np.where(sel[t0:] >= 0, sel[t0:] - t0, -1))
    print("%s: check_figures on %d targets %.1f s" % (label, u.H3_T - t0, time.perf_counter() - t))
    several = [int(tt) for tt in u.H3_MULTI if np.nansum(weight[seg[tt]:seg[tt + 1]] > 0) >= 2 and fig[4][0, tt] > 0]
    assert len(several) >= 8 and all(0 < weight[seg[tt]:seg[tt + 1]].max() < 1 for tt in several)
