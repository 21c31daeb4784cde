"""CPU: the recorded sweep of 0-1 ILPs on the dispatch thresholds of csrc/mht_blp.hip (tests/golden/g24_ilp_sweep.npz, written by
oracle/gen_ilp_sweep.py) is what tests/test_blp_sweep_gpu.py takes it for: feasible optima that sum to their objectives, brute force in
agreement, every shape present, grid costs on the grid, and enough instances without a dual certificate."""
import numpy as np
import pytest

import mht_oracle as orc
from blp_sweep_util import FAMILIES, GAP, check_feasible, load_sweep

SMALL_K = (1, 2, 3, 4, 5, 8, 9, 10, 11, 12)
MIDDLE_K = (16, 23, 24, 25, 63, 64, 65)


@pytest.fixture(scope="module")
def sweep(gold_dir):
    return load_sweep(gold_dir)


def test_recorded_optima_are_feasible_and_sum_to_their_objective(sweep):
    for inst in sweep:
        check_feasible(inst, inst["sel"])
        s = float(np.sum(inst["cost"][inst["sel"]]))
        if inst["variant"] == "grid":
            assert s == inst["obj"], inst["index"]      # (exact in any order)
        else:
            assert abs(s - inst["obj"]) <= 1e-12 * max(1.0, abs(s)), inst["index"]
        # the LP relaxation bounds the optimum from below, the second-best point from above
        assert inst["lp"] <= inst["obj"] + 1e-9 * max(1.0, abs(inst["obj"])), inst["index"]
        assert inst["second"] >= inst["obj"] - 1e-12 * max(1.0, abs(inst["obj"])), inst["index"]
        assert inst["unique"] == (inst["second"] > inst["obj"] + 1e-9), inst["index"]
        # the tags describe the instance
        assert (inst["K"], inst["nH"]) == (len(inst["sizes"]), len(inst["cols"])) and int(np.sum(inst["sizes"])) == inst["nH"]
        assert inst["nR"] == len({int(r) for c in inst["cols"] for r in c}) and inst["PD"] == max(len(c) for c in inst["cols"])
        # the model: the last column of every target is the empty one at cost 0, every other column has rows and a negative cost
        ends = np.cumsum(inst["sizes"]) - 1
        for h, c in enumerate(inst["cols"]):
            if h in set(ends.tolist()):
                assert len(c) == 0 and inst["cost"][h] == 0.0
            else:
                assert 1 <= len(c) == len(set(c.tolist())) and -(len(c) + 1.5) - 2.0 ** -10 <= inst["cost"][h] <= -len(c)


def test_brute_force_agrees_wherever_it_was_run(sweep):
    """The generator ran the exhaustive search on every instance of at most 10^5 combinations and recorded its optimum and its count of
    optimal points; the smallest ones (at most 2 000 combinations) are searched again here."""
    ran = again = 0
    for inst in sweep:
        combos = float(np.prod(np.asarray(inst["sizes"], dtype=np.float64)))
        assert inst["bf"] == (combos <= 1e5 and inst["family"] in ("small", "depth")), inst["index"]
        if not inst["bf"]:
            continue
        ran += 1
        assert abs(inst["bf_obj"] - inst["obj"]) <= 1e-12 * max(1.0, abs(inst["obj"])), inst["index"]
        assert (inst["bf_ties"] == 1) or not inst["unique"], inst["index"]
        if combos <= 2000:
            again += 1
            bs, bo, ties = orc.solve_blp_bruteforce([c.tolist() for c in inst["cols"]], inst["sizes"], inst["cost"])
            assert abs(bo - inst["obj"]) <= 1e-12 * max(1.0, abs(bo)) and ties == inst["bf_ties"], inst["index"]
            if inst["unique"]:
                assert sorted(bs) == inst["sel"].tolist(), inst["index"]
    assert ran >= 100 and again >= 40, (ran, again)


def test_every_shape_is_present_in_both_cost_variants(sweep):
    def have(family, key):
        return {(key(i), i["variant"]) for i in sweep if i["family"] == family}

    def both(shapes):
        return {(s, v) for s in shapes for v in ("grid", "cont")}
    assert {i["family"] for i in sweep} == set(FAMILIES)
    # small: every K at the three depths (a column cannot be longer than the pool of R = max(2, floor(1.2 K)) rows)
    want = [(K, min(pd, max(2, (12 * K) // 10))) for K in SMALL_K for pd in (1, 4, 8)]
    assert have("small", lambda i: (i["K"], i["PD"])) == both(want)
    for K in SMALL_K:      # 8 .. 12 structures of every K
        assert 8 <= sum(1 for i in sweep if i["family"] == "small" and i["K"] == K and i["variant"] == "grid") <= 12
        assert all(2 <= s <= 6 for i in sweep if i["family"] == "small" and i["K"] == K for s in i["sizes"])
    assert have("wide", lambda i: (i["K"], i["nH"])) == both([(K, n) for K in (3, 10) for n in (511, 512, 513)])
    assert have("middle", lambda i: i["K"]) == both(MIDDLE_K)
    assert have("tier", lambda i: (i["K"], i["nH"])) == both([(256, 2048), (256, 2049), (257, 2056)])
    assert all(i["nR"] < 700 and i["PD"] <= 8 for i in sweep if i["family"] == "tier")      # (only K and nH decide the tier there)
    assert have("rowedge", lambda i: (i["K"], i["nR"])) == both([(128, n) for n in (1022, 1023, 1024, 1025)])
    assert all(i["nH"] <= 2048 and i["PD"] <= 8 for i in sweep if i["family"] == "rowedge")      # (only nR decides the tier there)
    assert have("depth", lambda i: (i["K"], i["PD"])) == both([(K, pd) for K in (6, 30) for pd in (8, 9, 15)])


def test_grid_costs_are_multiples_of_2_to_the_minus_10(sweep):
    n = {"grid": 0, "cont": 0}
    for inst in sweep:
        n[inst["variant"]] += 1
        on_grid = bool(np.all(inst["cost"] * 1024.0 == np.round(inst["cost"] * 1024.0)))
        assert on_grid == (inst["variant"] == "grid"), inst["index"]
    assert n["grid"] == n["cont"] > 0
    # the two variants of a structure follow each other and differ in their costs only, by at most half a grid step
    for a, b in zip(sweep[0::2], sweep[1::2]):
        assert (a["variant"], b["variant"]) == ("cont", "grid") and np.array_equal(a["sizes"], b["sizes"])
        assert all(np.array_equal(x, y) for x, y in zip(a["cols"], b["cols"]))
        assert np.max(np.abs(a["cost"] - b["cost"])) <= 2.0 ** -11


def test_enough_instances_have_no_dual_certificate(sweep):
    """Coverage condition: at least 30 % of the instances of every small-K and middle-K shape (a shape is a K) have obj - lp > 1e-6, so
    that the solver has to finish them by enumeration or branch and bound.  K = 1 is exempt: with one target the LP is integral."""
    for family, Ks in (("small", SMALL_K[1:]), ("middle", MIDDLE_K)):
        for K in Ks:
            mine = [i for i in sweep if i["family"] == family and i["K"] == K]
            gaps = sum(1 for i in mine if i["obj"] - i["lp"] > GAP)
            assert 10 * gaps >= 3 * len(mine), (family, K, gaps, len(mine))
    assert not any(i["gap"] for i in sweep if i["K"] == 1 or i["PD"] == 1)      # (one target / an assignment problem: integral)
    # the padded families lean on a core with a gap as well: the tier and row edges are crossed by clusters that have to branch
    for family in ("tier", "rowedge"):
        assert all(i["gap"] for i in sweep if i["family"] == family)
