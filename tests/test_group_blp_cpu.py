"""CPU: the host-side checker of tests/test_group_blp_gpu.py (tests/group_blp_util.py) is itself sensitive.

The instances come from the oracle (OracleTracker.ilp_recorder) on a small line scene -- runs [2, 3, 1, 4], 3 scans, N = 3,
merge_threshold = 0 so that neighbours 12 m apart are admitted -- and from hand-made clusters on the boundaries of the light pass:
nine members, a clash between two minimisers, a conflict-free cluster of eight, two equal costs."""
import numpy as np
import pytest

import mht_oracle as orc
from group_blp_util import LAMBDA_PHI, PERIOD, P_D, Cluster, _scene, feasible, from_instance, light_verdict, objective

RUNS = [2, 3, 1, 4]


@pytest.fixture(scope="module")
def recorded():
    x0, scans = _scene(RUNS, n_scans=3)
    ot = orc.OracleTracker(PERIOD, LAMBDA_PHI, 1e-4, P_d=P_D, N=3, eta2=5.99, merge_threshold=0.0)
    ot.ilp_recorder = []
    for x in x0:
        assert ot.initiate_target(0.0, x.copy(), orc.model_P0())
    for k, z in enumerate(scans):
        ot.add_scan(PERIOD * (k + 1), z)
        assert [len(c) for c in ot.clusters] == RUNS, k      # (the scene is the one meant)
    assert len(ot.ilp_recorder) == 3 * sum(1 for r in RUNS if r >= 2)
    return ot.ilp_recorder


def test_objective_of_the_oracles_selection_is_the_recorded_one(recorded):
    for inst in recorded:
        cl = from_instance(inst)
        assert (cl.K, cl.nH) == (len(inst["sizes"]), len(inst["cols"]))
        assert objective(cl, inst["sel"]) == inst["obj"]
        # (and the instance goes back into the solver as it came out of the recorder)
        cols, sizes, cost = cl.instance()
        assert cols == [sorted(c) for c in inst["cols"]] and sizes == list(inst["sizes"]) and np.array_equal(cost, np.asarray(inst["cost"]))


def test_feasible_accepts_the_oracles_selection(recorded):
    for inst in recorded:
        assert feasible(from_instance(inst), inst["sel"])


def test_feasible_rejects_a_member_moved_onto_a_neighbours_row(recorded):
    moved = 0
    for inst in recorded:
        cl = from_instance(inst)
        sel = list(inst["sel"])
        for k in range(cl.K):
            others = set().union(*[set(cl.cols[sel[j]].tolist()) for j in range(cl.K) if j != k])
            for h in range(int(cl.first[k]), int(cl.first[k + 1])):
                if set(cl.cols[h].tolist()) & others:
                    bad = list(sel)
                    bad[k] = h
                    assert not feasible(cl, bad), (k, h)
                    moved += 1
                    break
    assert moved >= len(recorded)      # (every cluster of the line scene has such a column: the link plots)


def test_feasible_rejects_a_column_outside_its_members_range_and_a_short_selection(recorded):
    cl = from_instance(recorded[-1])
    sel = list(recorded[-1]["sel"])
    assert not feasible(cl, sel[:-1])
    assert not feasible(cl, [sel[1]] + sel[1:])      # (member 0 on a column of member 1)
    assert not feasible(cl, sel[:-1] + [cl.nH])


def _disjoint(K, per=3):
    """K members with `per` columns each: column j of member k has the rows {k * per + j} and costs -(j + 1): the last one is the cheapest"""
    cols = [[k * per + j] for k in range(K) for j in range(per)]
    cost = [-(j + 1.0) for k in range(K) for j in range(per)]
    return cols, [per] * K, cost


def test_light_verdict_defers_nine_members():
    assert light_verdict(Cluster(*_disjoint(9))) == ("deferred", None)


def test_light_verdict_defers_a_clash_between_two_minimisers():
    cols, sizes, cost = _disjoint(8)
    cols[3 * 5 + 2] = [3 * 2 + 2, 40]      # member 5's cheapest column takes the row of member 2's cheapest one as well
    assert light_verdict(Cluster(cols, sizes, cost)) == ("deferred", None)
    cols[3 * 5 + 2] = [3 * 2 + 1, 40]      # ... the row of a column of member 2 that is not its minimiser: no clash
    assert light_verdict(Cluster(cols, sizes, cost)) == ("finished", [3 * k + 2 for k in range(8)])


def test_light_verdict_defers_a_member_without_a_column():
    cols, sizes, cost = _disjoint(3)
    assert light_verdict(Cluster(cols[:6], [3, 0, 3], cost[:6])) == ("deferred", None)


def test_light_verdict_finishes_a_conflict_free_cluster_of_eight():
    cl = Cluster(*_disjoint(8))
    verdict, mins = light_verdict(cl)
    assert verdict == "finished" and mins == [3 * k + 2 for k in range(8)]
    assert feasible(cl, mins) and objective(cl, mins) == -24.0
    sel, obj = orc.solve_blp_exact(*cl.instance())
    assert sel == mins and obj == -24.0      # (conflict-free minimisers are the optimum)


def test_light_verdict_gives_a_tie_to_the_lowest_index():
    cols, sizes, cost = _disjoint(2)
    cost[1] = cost[2] = -3.0                          # member 0: columns 1 and 2 equal
    assert light_verdict(Cluster(cols, sizes, cost)) == ("finished", [1, 5])
    cols[1] = [1, 3 + 2]                              # the lower of the two now clashes with member 1's minimiser: that one decides
    assert light_verdict(Cluster(cols, sizes, cost)) == ("deferred", None)
    cols[1], cols[2] = [1], [2, 3 + 2]                # the higher one clashing does not
    assert light_verdict(Cluster(cols, sizes, cost)) == ("finished", [1, 5])
