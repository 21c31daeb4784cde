"""GPU: the ILP stage of a sector group (mht_group_step) with clusters placed on the boundaries of its code, every selection held to an
optimum computed outside the library.

Every test steps solo trackers and their grouped twins (SectorGroup) through the same crafted line scenes (tests/group_blp_util.py) under
one of three settings of the group's ILP stage, read at mht_group_create: `light` (MHT_BLP_LIGHT=1: blp_light_batch_kernel, then the narrow
launch of blp_batch_kernel over big_list), `batch0` (MHT_BLP_LIGHT=0: one launch) and `two_tier` (MHT_BLP_TWO_TIER=1: the 512-column /
256-row / 16-target tier first, what it leaves in a second launch) -- with 3 members and with 8, from where on the grow launch of a group
is the wavefront-per-target one.  Member 0 carries RUNS_EDGES, member 1 only lone targets (no multi-target cluster: every workgroup of a
second launch is idle), member 2 RUNS_MANY with one empty scan, members 3 to 7 _runs_mixed scenes of different sizes and seeds.  After
every scan, for every member, from the grouped tracker's own context:
  1  the member equals its solo tracker: the report rows and scan statistics test_sectors_gpu.py compares, cl_ptr, cl_members,
     cl_counts[:3], and at the end leafBatch() bit for bit;
  2  the cluster sizes are the runs;
  3  every multi-target cluster's selection is feasible;
  4  its objective is within 1e-9 * max(1, |obj|) of mht_oracle.solve_blp_exact's on the instance rebuilt from the read-back tables (the
     bound of the recorded-instance tests) -- for EVERY multi-target cluster: no column bound is needed and none is left out, HiGHS
     takes 0.04 s on the largest of the boundary scenes (24 targets, 8 663 columns), the deep test below (clusters of up to 23 644
     columns) takes 1.8 s in all, the slowest test 3 s, and an instance is solved once per process;
  5  light: cl_counts[4] is the number of clusters light_verdict defers, every cluster it finishes is CERTIFIED after 0 rounds with
     exactly the predicted minimisers, every cluster of 9 and more members is deferred, both outcomes occur for K <= 8, and on some scan
     more clusters are deferred than the second launch has workgroups per sector;
  6  two_tier: clusters occur inside (16 targets, 512 columns), beyond 16 targets, and beyond 512 columns with at most 16 targets.

The scenes have THREE scans.  Measured on the solo trackers (MI355X), per scan: multi-target clusters, the widest member (columns), what
light_verdict says, and (K, columns, widest member) of the clusters of 9 and more targets:
  RUNS_EDGES  scan 1: 11 clusters, widest   6, finished 2 deferred 9; (9, 49, 6) (9, 50, 6) (16, 92, 6) (17, 98, 6) (24, 140, 6)
              scan 2: 11 clusters, widest  49, finished 2 deferred 9; (9, 346, 48) (9, 365, 48) (16, 689, 48) (17, 746, 48) (24, 1080, 49)
              scan 3: 11 clusters, widest 405, finished 2 deferred 9; (9, 2534, 373) (9, 2692, 376) (16, 5386, 404) (17, 5887, 403) (24, 8663, 405)
              (finished: the first 8 and the 7; deferred for K <= 8: the two pairs, the second 8 and the triple, by their clash pairs; the
              widest member of a cluster of at most 8 has 355 columns on scan 3: the light pass's second loop runs from scan 3 on)
  RUNS_MANY   scan 1: 48 clusters, widest   6, finished 20 deferred 28 (the middle target of a triple has two link plots at 6 m: half of
                      the triples' pairs do not clash yet)
              scan 2 (empty): 48 clusters, widest 6, finished 20 deferred 28
              scan 3: 48 clusters, widest  35, finished 4 deferred 44 -- more than the 8 + TEAM_W = 40 workgroups of the narrow launch
A fourth scan is out of reach for these scenes: a hypothesis of four misses in a row has a gate of some 70 m, wider than the 60 m between
the runs, all targets of a member become ONE cluster (observed with 45, 36 and 26 targets) and RUNS_EDGES overflows the node pool (240 k children).  What a fourth
and fifth scan add -- roots that advance while the light pass finishes clusters -- is held by a second test on a smaller scene with its runs
250 m apart in one row (RUNS_DEEP, [3] * 12 with an empty fourth scan, lone targets), five scans, 3 members, the same checks:
  RUNS_DEEP   scans 1..5: 6 clusters, widest 6 / 48 / 377 / 2 597 / 3 059; finished 2 deferred 4 (scan 5: 3 and 3);
              the 9-target clusters (9, 49) (9, 50) / (9, 345) (9, 363) / (9, 2521) (9, 2674) / (9, 17748) (9, 19075) / (9, 23394) (9, 23644)
  [3] * 12    scans 1..5: 12 clusters, widest 6 / 30 / 155 / 155 / 172; finished 7, 3, 8, 8, 12; deferred 5, 9, 4, 4, 0"""
import functools

import numpy as np
import pytest

import mht_oracle as orc
from group_blp_util import (CERTIFIED, LIGHT_MAXK, PERIOD, _runs_mixed, _scene, _tracker, clusters_of, feasible, light_verdict, objective,
                            read_tables, selection)

pytestmark = pytest.mark.gpu

MODES = {"light": {"MHT_BLP_LIGHT": "1"}, "batch0": {"MHT_BLP_LIGHT": "0"}, "two_tier": {"MHT_BLP_TWO_TIER": "1"}}
N_SCANS = 3
T1_K, T1_H, TEAM_MIN_K = 16, 512, 24      # csrc/mht_blp.hip: blp_set_tier; csrc/mht_kernels.h (a cluster of TEAM_MIN_K targets is searched by a team)
NARROW_GRID = 8 + 32                      # csrc/mht_forest.hip: mht_group_step, 8 + TEAM_W workgroups per sector in the second launch
# both sides of LIGHT_MAXK; both sides of t1_k = 16; a team-sized cluster -- with a clash pair in every second multi-target run
RUNS_EDGES = [8, 9, 1, 7, 2, 8, 1, 9] + [16, 17, 1, 2] + [24, 3, 1]
CLASH_EDGES = (1, 4, 5, 8, 11, 13)        # the 9, the 2, the second 8, the 16, the second 2, the 3
assert max(RUNS_EDGES) == TEAM_MIN_K and T1_K in RUNS_EDGES and T1_K + 1 in RUNS_EDGES
# more deferred clusters than the second launch has workgroups: the issue's 40 triples, and 8 pairs behind them since 40 clusters cannot
# give more than 40 deferred ones; all but the first four runs carry a clash pair
RUNS_MANY = [3] * 40 + [2] * 8
CLASH_MANY = tuple(range(4, 48))
EMPTY_SCAN = 1                            # member 2 sees nothing on this scan
# four scans and more: the roots advance (N = 3) while the light pass finishes clusters.  A run of misses widens a hypothesis' gate to some
# 70 m by the fourth scan, so the runs lie DEEP_GAP apart in one row, and the scene is small: a member holds 2 000 to 3 000 columns then
RUNS_DEEP = [8, 9, 1, 7, 2, 8, 1, 9]
CLASH_DEEP = (1, 4, 5)
DEEP_SCANS, DEEP_GAP, DEEP_EMPTY_SCAN = 5, 250.0, 3


@functools.lru_cache(maxsize=None)
def _member_scene(q, deep=False):
    """(runs, x0, scans) of member q; computed once, nobody writes to it"""
    kw = dict(n_scans=DEEP_SCANS, gap=DEEP_GAP, width=1e9) if deep else dict(n_scans=N_SCANS)
    if q == 0:
        runs, clash = (RUNS_DEEP, CLASH_DEEP) if deep else (RUNS_EDGES, CLASH_EDGES)
    elif q == 1:
        runs, clash = [1] * 30, ()
    elif q == 2:
        runs, clash = ([3] * 12, tuple(range(2, 12))) if deep else (RUNS_MANY, CLASH_MANY)
    else:
        runs, clash = _runs_mixed(24 + 3 * q), ()
    x0, scans = _scene(runs, seed=5446 + 101 * q, clash=clash, **kw)
    if q == 2:
        scans = list(scans)
        scans[DEEP_EMPTY_SCAN if deep else EMPTY_SCAN] = np.zeros((0, 2), np.float32)
    return runs, x0, scans


_optimum_cache = {}


def _optimum(cl):
    """solve_blp_exact's value of the instance; the group's tables equal the solo tracker's in every mode, so one solve serves all tests"""
    key = cl.key()
    if key not in _optimum_cache:
        _optimum_cache[key] = orc.solve_blp_exact(*cl.instance())[1]
    return _optimum_cache[key]


def _same_state(a, b, what):
    sa, sb = a._sel[0], b._sel[0]
    for name in ("id", "status", "sel_meas", "sel_x", "sel_cnllr", "score", "root_scan", "root_meas", "root_x", "n_leaves", "cluster"):
        assert np.array_equal(sa[name], sb[name]), (what, name)
    assert a.nTargets == b.nTargets, what
    for k in ("L", "G", "M", "leaves_out", "clusters", "ilp"):
        assert a.lastScanStats[k] == b.lastScanStats[k], (what, k)


def _run(mode, n_members, monkeypatch, deep=False, **trk_kw):
    """Steps n_members solo trackers and their grouped twins through their scenes under the switches of `mode`, with checks 1 to 5 of the
    module's docstring after every scan; returns what occurred."""
    from pymht_amd.sectors import SectorGroup
    from pymht_amd.utils.classDefinitions import MeasurementList
    for name in ("MHT_BLP_LIGHT", "MHT_BLP_TWO_TIER", "MHT_FG_WAVE", "MHT_GROUP_BLP_DIV"):
        monkeypatch.delenv(name, raising=False)
    for name, v in MODES[mode].items():
        monkeypatch.setenv(name, v)      # (read at mht_group_create)
    scenes = [_member_scene(q, deep) for q in range(n_members)]
    n_scans = len(scenes[0][2])
    solo = [_tracker(x0, {}, mirror=True, **trk_kw) for _, x0, _ in scenes]
    grouped = [_tracker(x0, {}, mirror=True, **trk_kw) for _, x0, _ in scenes]
    grp = SectorGroup(grouped)
    seen = dict(multi=0, finished_small=0, deferred_small=0, deferred_max=0, inside=0, beyond_k=0, beyond_h=0, second_loop=0,
                big_checked={0: 0}, roots_moved=0, census=[])
    try:
        for k in range(n_scans):
            lists = [MeasurementList(PERIOD * (k + 1), sc[2][k]) for sc in scenes]
            for t, sl in zip(solo, lists):
                t.addMeasurementList(sl)
            grp.addMeasurementLists(lists)
            for q, (runs, _, _) in enumerate(scenes):
                what = "scan %d member %d" % (k, q)
                ts, tg = read_tables(solo[q]), read_tables(grouped[q])      # (before the next step: sel and cost are this scan's)
                # 1 -- the grouped member is its solo tracker
                _same_state(grouped[q], solo[q], what)
                for name in ("cl_ptr", "cl_members"):
                    assert np.array_equal(ts[name], tg[name]), (what, name)
                assert np.array_equal(ts["cl_counts"][:3], tg["cl_counts"][:3]), what
                # 2 -- the scene is the one meant
                assert np.diff(tg["cl_ptr"]).tolist() == list(runs), (what, np.diff(tg["cl_ptr"]).tolist()[:20])
                assert np.array_equal(tg["cl_members"], np.arange(sum(runs))), what
                assert tg["cl_counts"][:3].tolist() == [len(runs), sum(1 for r in runs if r >= 2), sum(1 for r in runs if r == 1)], what
                cls = clusters_of(tg)
                assert [c.K for c in cls] == [r for r in runs if r >= 2], what
                n_deferred = 0
                row = []
                for cl in cls:
                    sel = selection(tg, cl)
                    # 3 -- a selection of the ILP
                    assert feasible(cl, sel), (what, cl.c, cl.K, sel)
                    # 4 -- and an optimal one
                    seen["multi"] += 1
                    obj, best = objective(cl, sel), _optimum(cl)
                    assert abs(obj - best) <= 1e-9 * max(1.0, abs(obj)), (what, cl.c, cl.K, cl.nH, obj, best)
                    if cl.K >= T1_K:
                        seen["big_checked"][q] = seen["big_checked"].get(q, 0) + 1
                    verdict, mins = light_verdict(cl)
                    n_deferred += verdict == "deferred"
                    seen["second_loop"] += cl.K <= LIGHT_MAXK and max(cl.sizes) > 64
                    if cl.K <= T1_K and cl.nH <= T1_H:
                        seen["inside"] += 1
                    elif cl.K > T1_K:
                        seen["beyond_k"] += 1
                    else:
                        seen["beyond_h"] += 1
                    row.append((cl.K, cl.nH, max(cl.sizes), verdict[0]))
                    if mode != "light":
                        continue
                    # 5 -- routing of the light pass
                    if cl.K > LIGHT_MAXK:
                        assert verdict == "deferred"
                    else:
                        seen[verdict + "_small"] += 1
                    if verdict == "finished":
                        assert tg["cl_status"][cl.c] == CERTIFIED and tg["cl_iters"][cl.c] == 0, (what, cl.c, cl.K)
                        assert sel == mins, (what, cl.c, cl.K, sel, mins)
                if mode == "light":
                    assert int(tg["cl_counts"][4]) == n_deferred, (what, int(tg["cl_counts"][4]), n_deferred)
                    seen["deferred_max"] = max(seen["deferred_max"], n_deferred)
                seen["census"].append((k, q, row))
        seen["roots_moved"] = int(sum(np.count_nonzero(t._sel[0]["root_scan"] > 0) for t in grouped))
        for q in range(n_members):
            la, lb = grouped[q].leafBatch(), solo[q].leafBatch()
            for key in la:
                if key != "node":      # node indices are handles (block taken with an atomic)
                    assert np.array_equal(la[key], lb[key]), (q, key)
    finally:
        grp.close()
        for t in solo + grouped:
            t.close()
    for k, q, row in seen["census"]:
        if q in (0, 2):
            big = [r for r in row if r[0] >= 9]
            print("census scan %d member %d: %d multi, largest member %d columns, finished %d deferred %d, K>=9 (K, nH, widest): %s"
                  % (k, q, len(row), max(r[2] for r in row), sum(r[3] == "f" for r in row), sum(r[3] == "d" for r in row), [r[:3] for r in big]))
    print("census %s/%d: %s" % (mode, n_members, {k: v for k, v in seen.items() if k != "census"}))
    return seen


@pytest.mark.parametrize("n_members", [3, 8])
@pytest.mark.parametrize("mode", list(MODES))
def test_group_selections_are_exact_optima_at_the_boundaries(mode, n_members, monkeypatch):
    seen = _run(mode, n_members, monkeypatch)
    # what the scenes were built for did occur
    assert seen["big_checked"][0] >= 1, seen                 # (member 0 is the scene with clusters of 16 and more members)
    assert seen["second_loop"] >= 1, seen                    # a member with more than 64 columns: the light pass's second loop
    if mode == "light":
        assert seen["finished_small"] >= 1 and seen["deferred_small"] >= 1, seen
        assert seen["deferred_max"] > NARROW_GRID, seen      # a deferred list longer than the second launch's grid
    if mode == "two_tier":
        assert seen["inside"] >= 1 and seen["beyond_k"] >= 1 and seen["beyond_h"] >= 1, seen


@pytest.mark.parametrize("mode", list(MODES))
def test_group_selections_stay_exact_while_the_roots_advance(mode, monkeypatch):
    seen = _run(mode, 3, monkeypatch, deep=True, maxNodes=1 << 19)
    assert seen["roots_moved"] >= 40, seen                   # (87 targets; every root has advanced after five scans at N = 3)
    assert seen["second_loop"] >= 1, seen
    if mode == "light":
        assert seen["finished_small"] >= 1 and seen["deferred_small"] >= 1, seen
