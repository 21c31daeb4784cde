"""CPU: the scenes of tests/test_grow_workgroup_gpu.py reach, on the oracle alone, the conditions that test is about (grow_workgroup_util)."""
import numpy as np

import grow_workgroup_util as gw


def test_planted_scene_meets_its_plans():
    sc = gw.planted_scene()
    assert sc["children"] == [[p[k] for p in gw.PLANS] for k in range(len(gw.PLANS[0]))]
    kids = {c for row in sc["children"] for c in row}
    assert {63, 64, 65, 127, 128, 129, 192, 193} <= kids, "children counts on the wavefront edges of the emission"
    leaves = {n for row in sc["leaves_in"] for n in row}
    assert {1, 63, 64, 65} <= leaves and max(leaves) > 128, "leaf counts of the count phase's small paths, and one target of two passes"
    no_hit = [(k, t) for k in range(len(sc["children"])) for t in range(len(gw.PLANS)) if sc["children"][k][t] == sc["leaves_in"][k][t]]
    assert (0, 3) in no_hit and len(no_hit) >= 3, "targets without any hit: a single leaf, four leaves, 192 leaves"
    assert len(sc["scans"]) <= sc["N"], "nothing is pruned while the window fills: a target's children are its next leaves"
    assert all(z.dtype == np.float32 for z in sc["scans"])


def test_tail_scene_has_a_death_inside_a_cluster_four_state():
    sc = gw.tail_scene()
    assert gw.tail_conditions(sc) == 3


def test_tail_scene_has_a_death_inside_a_cluster_constant_turn():
    from pymht_amd.models import ct
    sc = gw.tail_scene(model=ct)
    assert sc["x0"].shape[1] == 6 and gw.tail_conditions(sc) == 3
