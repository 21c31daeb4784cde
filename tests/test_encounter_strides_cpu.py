"""CPU: the cases of tests/test_encounter_strides_gpu.py reach what they claim to reach, and none of them is vacuous.  The thresholds are
recomputed from the constants of csrc/mht_encounter.hip, mht_trial.h, mht_trial.hip and mht_trial_hyp.hip, read as text; the scenes of
tests/encounter_stride_util.py are checked on the float64 references alone."""
import os
import re

import numpy as np

import encounter_stride_util as u
import trial_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def constants(name):
    """The `constexpr int NAME = value;` of a file of csrc, the value an integer or another constant's name"""
    text = open(os.path.join(ROOT, "pymht_amd", "csrc", name)).read()
    return dict(re.findall(r"constexpr int (\w+) = (\w+);", text))


def ceil_div(a, b):
    return -(-a // b)


def test_every_case_lies_behind_the_threshold_it_is_there_for():
    enc, th, tr, hy = constants("mht_encounter.hip"), constants("mht_trial.h"), constants("mht_trial.hip"), constants("mht_trial_hyp.hip")
    tile, cap = int(enc["ENCOUNTER_THREADS"]), int(enc["ENCOUNTER_MAX_BLOCKS"])
    assert tr["TRIAL_THREADS"] == "TRIAL_TILE" and hy["HYP_THREADS"] == "TRIAL_TILE" and int(th["TRIAL_TILE"]) == tile == u.TILE
    assert int(tr["TRIAL_MAX_BLOCKS"]) == cap and int(hy["HYP_MAX_BLOCKS"]) == cap
    wave, most = int(tr["TRIAL_WAVE"]), int(th["TRIAL_MAX_CANDIDATES"])
    entries = cap * tile      # what one trip of a lane-per-entry kernel covers
    assert (cap, tile, wave, entries) == (2048, 256, 64, 524288)
    tiles = lambda rows, cols: rows * ceil_div(cols, tile)
    # E1: the smallest all-pairs call whose pair kernel strides
    assert tiles(u.E1_N, u.E1_N) == 2049 > cap >= tiles(u.E1_N - 1, u.E1_N - 1) and ceil_div(u.E1_N, tile) == 3 and tiles(3, u.E1_N) == 9
    # E2, T1: the propagate kernels stride, the second trip with more than one workgroup; one row strides; the summary's lanes stride
    assert u.BIG > entries + tile and ceil_div(u.BIG - entries, tile) == 2 and tiles(1, u.BIG) == 2050 > cap
    assert ceil_div(u.BIG, tile) > wave and ceil_div(ceil_div(u.BIG, tile), wave) == 33 and ceil_div(16384, tile) == wave
    assert (u.BIG - 1) // tile == 2049 and u.BIG - 2049 * tile == 44
    # T2: g changes from trip to trip (a trip's 2048 tiles are 1024 rows), one live lane in chunk 1, five workgroups of candidates
    assert tiles(u.T2_G, u.T2_N) == 2050 > cap >= tiles(u.T2_G - 1, u.T2_N) and u.T2_N - tile == 1 and ceil_div(u.T2_G, tile) == 5
    assert tiles(u.T2_G, u.T2_N - 1) <= cap and ceil_div(tile, tile) == 1 < ceil_div(tile + 1, tile)      # (G > 256: a second workgroup)
    # T3: the summary's grid strides (one workgroup a candidate), two trips a cell workgroup
    assert u.T3_G == most > cap and tiles(u.T3_G, 1) == 2 * cap
    # H1: 3 chunks, 2049 tiles; H2: the target kernel strides, and not with one target fewer
    L = sum(u.H1_SIZES)
    assert tiles(u.H1_G, L) == 2049 > cap >= tiles(u.H1_G - 1, L) and ceil_div(L, tile) == 3 and ceil_div(L - 1, tile) == 2
    assert u.H2_G == most and u.H2_G * u.H2_L == 528384 > entries >= u.H2_G * (u.H2_L - 1)
    assert tiles(u.H2_G, u.H2_L) == 4096 > cap
    # H3: the weight kernel (a target a lane) and the propagate kernel (a leaf a lane) stride; the targets of several leaves lie in the
    # weight kernel's second trip and their leaves, planted ones, in the propagate kernel's
    assert u.H3_T == 524573 > entries and u.BIG > entries + tile and (u.H3_MULTI >= entries).all() and len(u.H3_MULTI) >= 8
    assert set(u.H3_SIZES.tolist()) == {2, 3} and u.H3_T + int(np.sum(u.H3_SIZES - 1)) == u.BIG
    assert np.isin(np.arange(u.H3_MULTI[0], u.H3_MULTI[-1] + int(np.sum(u.H3_SIZES - 1)) + 1), u.PLANTED).all()
    # the planted entries and the ties sit where they are meant to
    assert {0, 1, 2047, 2048, 2049} <= set((u.PLANTED // tile).tolist()) and {255, 256, 257, 524287, 524288, 524289, u.BIG - 1} <= set(u.PLANTED.tolist())
    for a, b in u.TIES_SAME_LANE:
        assert b // tile == a // tile + wave and (a // tile) % wave == (b // tile) % wave
    for a, b in u.TIES_TWO_LANES:
        assert (a // tile, b // tile) == (wave - 1, wave)
    assert u.TIES_TWO_LANES[0] == (16383, 16384)
    assert not np.isin(np.ravel(u.TIES_SAME_LANE + u.TIES_TWO_LANES), u.PLANTED).any()


def test_e1_has_50000_cells_with_a_pc():
    f64 = u.e1(4, truth=False)[4]
    live = int(np.sum(f64["pc"] > 0))
    print("E1: %d cells with pc > 0" % live)
    assert live >= 50000


def live_in_every_place(pc):
    """At least 64 cells with pc > 0 in each of the four places -- in the last tile, which holds 44 entries, every one of them"""
    for name, m in u.places().items():
        live = int(np.sum(pc[m] > 0))
        print("%s: %d cells with pc > 0 of %d" % (name, live, int(m.sum())))
        assert live >= min(64, int(m.sum())), name
    assert int(np.sum(pc > 0)) < 400      # (the fleet is far away: the table takes no quadrature to speak of)


def test_e2_has_live_cells_in_the_four_places():
    f64 = u.e2(6, truth=False)[4]
    live_in_every_place(f64["pc"][0])
    assert np.isnan(f64["pc"][0, u.NAN_ENTRY]) and np.isnan(f64["pc"][0, 0])


def test_t1_has_live_cells_in_the_four_places_and_its_ties_are_the_rows_extremes():
    f64 = u.t1(4, truth=False)[6]
    live_in_every_place(f64["pc"][0])
    for ties, ev in ((u.TIES_SAME_LANE, f64), (u.TIES_TWO_LANES, u.permuted(f64, u.t1_swap()))):
        pc, dcpa = ev["pc"][0], ev["dcpa"][0]
        (p1, p2), (d1, d2) = ties
        assert np.flatnonzero(pc == np.nanmax(pc)).tolist() == [p1, p2] and np.flatnonzero(dcpa == np.nanmin(dcpa)).tolist() == [d1, d2]
        want = tref.fold(ev["pc"], ev["dcpa"])
        assert (want["pcArg"][0], want["dcpaArg"][0]) == (p1, d1) and 0 < pc[p1] and pc[d1] < pc[p1]
    x, P = u.t1_scene(4)[:2]
    for a, b in u.TIES_SAME_LANE:
        assert np.array_equal(x[a], x[b]) and np.array_equal(P[a], P[b])


def test_h3_has_live_cells_in_the_four_places_and_its_targets_of_several_leaves_are_live():
    x, P, cnllr, seg, sel, own, Sown, Phi, Q, cand, f64, _ = u.h3(4, truth=False)
    live_in_every_place(f64["pc"][0])
    assert len(seg) == u.H3_T + 1 and seg[-1] == u.BIG == len(x) and np.array_equal(np.diff(seg)[u.H3_MULTI], u.H3_SIZES) and int(np.diff(seg).max()) == 3
    assert np.array_equal(seg[:u.H3_MULTI[0] + 1], np.arange(u.H3_MULTI[0] + 1)) and ((seg[:-1] <= sel) & (sel < seg[1:])).all()
    good = 0
    for t in u.H3_MULTI:
        c, pc = cnllr[seg[t]:seg[t + 1]], f64["pc"][0, seg[t]:seg[t + 1]]
        good += len(set(c.tolist())) == len(c) and int(np.sum(pc > 0)) >= 2 and len(set(pc[pc > 0].tolist())) >= 2
    print("H3: %d targets behind 524 288 have two or three leaves of different cnllr with different pc > 0" % good)
    assert good >= 8


def test_the_candidate_scenes_are_as_stated():
    # T2, T3: the cycle of candidates, the NaN candidate, live cells in the last row and in chunk 1
    x, P, Phi, Q, own, Sown, cand, kind = u.t2_scene(6)
    assert cand.shape == (u.T2_G, 3) and x.shape == (u.T2_N, 6) and np.isnan(cand[u.T2_NAN, 0]) and kind[u.T2_NAN] == -1
    assert np.array_equal(cand[kind >= 0], tref.CANDIDATES[kind[kind >= 0]]) and all(int(np.sum(kind == k)) >= 204 for k in range(5))
    f64 = u.distinct_rows(x, P, Phi, Q, own, Sown, ("t2", 6), truth=False)[0]
    assert int(np.sum(f64["pc"][kind[-1]] > 0)) >= 20 and not np.isnan(f64["dcpa"][:, 256]).any() and kind[-1] == 1
    assert len({f64["pc"][k].tobytes() for k in range(5)}) >= 3      # (K = 1: a manoeuvre that begins at t = 5 or later is standing on)
    x, P, Phi, Q, own, Sown, cand, kind = u.t3_scene(4)
    assert cand.shape == (u.T3_G, 3) and x.shape == (1, 4) and np.array_equal(cand, tref.CANDIDATES[kind])
    f64 = u.distinct_rows(x, P, Phi, Q, own, Sown, ("t3", 4), truth=False)[0]
    assert ((f64["pc"] > 0.01) & (f64["pc"] < 0.99)).all() and len(np.unique(f64["pc"])) >= 3 and len(np.unique(f64["dcpa"])) >= 3
    # H1: the segments
    x, P, cnllr, seg, sel, own, Sown, Phi, Q, cand, kind = u.h1_scene(6)
    assert seg.tolist() == [0, 250, 262, 512, 513] and len(x) == 513 and cand.shape == (u.H1_G, 3)
    assert seg[1] < 256 < seg[2] and seg[3] == 512 and seg[4] - seg[3] == 1      # straddles 256; ends at 512; begins a tile alone
    assert sel[u.H1_NO_SELECTED] == -1 and all(seg[t] <= sel[t] < seg[t + 1] for t in (0, 1, 3))
    assert np.isnan(cnllr[140]) and np.isinf(cnllr[141]) and np.isnan(x[70]).any() and np.array_equal(x[130], x[131])
    f64 = u.distinct_rows(x, P, Phi, Q, own, Sown, ("h1", 6), truth=False)[0]
    assert sum(int(np.sum(f64["pc"][k] > 0)) * int(np.sum(kind == k)) for k in range(5)) >= 50000
    # H2: one leaf a target
    x, P, cnllr, seg, sel, own, Sown, Phi, Q, cand, kind = u.h2_scene(4)
    assert np.array_equal(seg, np.arange(u.H2_L + 1)) and np.array_equal(sel, np.arange(u.H2_L)) and np.isfinite(cnllr).all() and cand.shape == (u.H2_G, 3)
    f64 = u.distinct_rows(x, P, Phi, Q, own, Sown, ("h2", 4), truth=False)[0]
    assert sum(int(np.sum(f64["pc"][k] > 0)) * int(np.sum(kind == k)) for k in range(5)) >= 64 * 20
