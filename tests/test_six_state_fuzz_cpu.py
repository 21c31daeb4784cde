"""CPU: the census of the scenes tests/test_six_state_fuzz_gpu.py runs through the linear six-state forest (Tracker(models.ca, ...)), taken
from the oracle alone (fuzz_util.oracle_run -- the same call the device tests take their expectations from).  A scene that stops reaching
a path -- multi-target ILPs, large clusters, terminations, scans of a thousand leaves, fused groups whose mean is a NEW covariance value
(three, five, six, seven hits and more), windows whose path records take 16 ints -- fails here, on any machine, and not silently on the
GPU.  The thresholds are conditions on the inputs, set at about half of what the oracle gave when the scenes were chosen."""
import pytest

import fuzz_util
from fuzz_util import CA_PLAIN_SEEDS as PLAIN_SEEDS, CA_SIMILAR_SEEDS as SIMILAR_SEEDS, CA_MAX_LEAVES as MAX_LEAVES


def slice_census(seeds, similar):
    total = {}
    for seed in seeds:
        fuzz_util.add_census(total, fuzz_util.oracle_run(fuzz_util.ca_scene(seed, similar), MAX_LEAVES)["census"])
    return total


def test_plain_slice_census():
    """24 seeds, leaf cap 1 500.  Oracle alone, seeds 320000..320023: 240 ILPs, largest cluster 40 targets,
    71 terminations, largest scan 5 068 leaves."""
    c = slice_census(PLAIN_SEEDS, False)
    print(c["ilp"], c["cluster"], c["dead"], c["L"])
    assert c["ilp"] >= 100 and c["cluster"] >= 16 and c["dead"] >= 30 and c["L"] >= 1000, (c["ilp"], c["cluster"], c["dead"], c["L"])
    assert not c["groups"]


def test_similar_slice_census():
    """24 seeds with similar-state pruning on three scans of four.  Oracle alone, seeds 370000..370023: 1 902 fused groups (1 876 of one
    hit, 24 of two, 2 of three: random scenes do not reach the large groups), 357 ILPs, largest cluster 56 targets, 125 terminations."""
    c = slice_census(SIMILAR_SEEDS, True)
    print(c["ilp"], c["cluster"], c["dead"], c["L"], fuzz_util.group_histogram(c["groups"]))
    assert len(c["groups"]) >= 500, len(c["groups"])


@pytest.mark.parametrize("model", ["ca", "pv"])
def test_crafted_scenes_census(model):
    """The three dense scenes, pruning on at every scan.  Group sizes on the oracle's side, over the three scenes: ca 34 groups of
    three hits, 19 of five, 6 of six, 8 of seven, 4 of eight and more, the largest 23; pv 32 of three, 21 of five, 20 of six, 11 of seven,
    32 of eight and more, the largest 20 (per scene in tests/test_six_state_fuzz_gpu.py)."""
    hist = {}
    for name in sorted(fuzz_util.CRAFTED):
        c = fuzz_util.oracle_run(fuzz_util.crafted_scene(name, model))["census"]
        h = fuzz_util.group_histogram(c["groups"])
        print(model, name, c["ilp"], c["cluster"], c["L"], c["merged_leaves"], h)
        assert c["merged_leaves"] > 0, name      # (merged nodes that are still leaves after the scan: what the device's covariances are held to)
        for s, n in h.items():
            hist[s] = hist.get(s, 0) + n
    assert hist.get(3, 0) >= 20, hist
    assert all(hist.get(s, 0) >= 1 for s in (5, 6, 7)), hist
    assert any(s >= 8 for s in hist) and any(s >= 16 for s in hist), hist


@pytest.mark.parametrize("N", [8, 9])
def test_long_window_census(N):
    """Windows of 8 and 9 scans over 12 scans, no leaf cap.  Oracle alone: N = 8: 17 ILPs, largest cluster 14 targets, largest scan
    3 887 leaves; N = 9: 16 ILPs, largest cluster 10 targets, largest scan 6 806 leaves."""
    c = fuzz_util.oracle_run(fuzz_util.long_window_scene(N))["census"]
    print(N, c["ilp"], c["cluster"], c["dead"], c["L"])
    assert c["scans"] == 12 and c["ilp"] >= 10 and c["L"] > 2000, (c["scans"], c["ilp"], c["L"])


def test_sharded_scene_has_a_large_cluster():
    """The scene of test_ca_cluster_sharded_equals_single_tracker: a plain-slice seed whose largest cluster has at least 16 targets."""
    c = fuzz_util.oracle_run(fuzz_util.ca_scene(fuzz_util.SHARDED_SEED), MAX_LEAVES)["census"]
    print(c["ilp"], c["cluster"], c["L"])
    assert c["cluster"] >= 16 and c["ilp"] >= 5, (c["cluster"], c["ilp"])
