"""CPU: the census of the scenes tests/test_ct_fuzz_gpu.py runs through the constant-turn forest (Tracker(models.ct, ...): fgrow_ct_kernel,
forest_ct_kernel, prune_similar_kernel's constant-turn branch), taken from the oracle alone (fuzz_util.oracle_run -- the call the device
tests take their expectations from; the figures per (target, scan) are fuzz_util.ct_grow_census: float64, nothing from a device).  What the
kernel's own paths depend on is asserted here, on any machine: the length of a target's candidate list (one to six words of hit mask per
leaf in LDS -- FG_HWC --, full-width masks in global memory past 384 candidates), a spilling target beside targets that do not spill, a
spilling target of several chunks, a chunk of more than FG_MAP = 1 024 children, fused groups whose mean covariance is a new value, path
records of 16 ints.  `cand` is a LOWER bound on the device's list, so the bands below are conditions on the inputs, not a statement of the
word count the device ends up with.  A scene that stops reaching its band -- another generator, another seed, another sigma -- fails here
and not silently on the GPU.  profiles/fuzz_ct_census.txt has the figures."""
import pytest

import fuzz_util
from fuzz_util import CT_PLAIN_SEEDS as PLAIN_SEEDS, CT_SIMILAR_SEEDS as SIMILAR_SEEDS, CA_MAX_LEAVES as MAX_LEAVES

BANDS = [(65, 128), (129, 192), (193, 256), (257, 320), (321, 384)]      # two to six words of 64 candidates
SPILL = 385                                                             # more than FG_HWC words


@pytest.fixture(scope="module")
def wide():
    """{name: census} of the wide-gate scenes."""
    return {name: fuzz_util.oracle_run(fuzz_util.wide_gate_scene(name))["census"] for name in sorted(fuzz_util.WIDE_GATE)}


def _rows(wide):
    return [(name, k, ti, g) for name, c in wide.items() for k, ti, g in fuzz_util.ct_grow_rows(c)]


def test_wide_gate_scenes_fill_every_mask_width(wide):
    """Oracle alone, (candidates, leaves) of the targets with more than 64 candidates, scan 1 | scan 2:
    a (416, 1) | (608, 333) (77, 8);  b (249, 1) | (150, 208);  c (239, 1) | (317, 192) (107, 14) (119, 16) (84, 11);
    d (322, 1) | (336, 262);  e (307, 1) | (176, 255)."""
    rows = _rows(wide)
    for name, c in wide.items():
        print(name, [[(g["cand"], g["leaves"], g["children"], g["chunk"]) for g in scan] for scan in c["grow"]])
        assert c["scans"] == 2, name
    for lo, hi in BANDS:
        assert any(lo <= g["cand"] <= hi for _, _, _, g in rows), (lo, hi)
    assert sum(g["cand"] >= SPILL for _, _, _, g in rows) >= 2


def test_wide_gate_scenes_mix_spilling_and_short_lists_in_one_launch(wide):
    """Scene a, scan 1: 416 candidates beside 9 and 17."""
    assert any(any(g["cand"] >= SPILL for g in scan) and any(g["cand"] <= 64 for g in scan) for c in wide.values() for scan in c["grow"])


def test_wide_gate_scenes_spill_over_several_chunks(wide):
    """Scene a, scan 2: 608 candidates on 333 leaves (three chunks, the count pass and the emission pass), 3 952 children in its fullest chunk."""
    rows = _rows(wide)
    assert any(g["cand"] >= SPILL and g["leaves"] > fuzz_util.CT_CHUNK for _, _, _, g in rows)
    assert any(g["chunk"] > 1024 for _, _, _, g in rows)
    # (the same in LDS, where the stride is the word count: a list of three and more words on more than one chunk)
    assert any(129 <= g["cand"] < SPILL and g["leaves"] > fuzz_util.CT_CHUNK for _, _, _, g in rows)


def test_wide_gate_scenes_terminate_tracks(wide):
    """Scene a: every track is gone after scan 2 (the terminations are part of what the device is compared on)."""
    assert wide["a"]["dead"] == 3 and sum(c["dead"] for c in wide.values()) >= 5, {n: c["dead"] for n, c in wide.items()}


def test_crafted_scenes_census():
    """The three dense scenes under models.ct, pruning on at every scan.  Oracle alone, group size: count --
    A {1: 75, 2: 33, 3: 8, 4: 4, 5: 1, 6: 1}, 13 ILPs, 112 merged leaves; B {1: 35, 2: 10, 3: 11, 4: 7, 5: 2, 6: 2, 7: 1}, 4 ILPs, 33 merged
    leaves; C {1: 2, 2: 4, 3: 7, 4: 9, 5: 6, 6: 10, 7: 6, 8: 8, 9: 1, 10: 3, 11: 1, 14: 1, 18: 1, 20: 1, 21: 1}, 2 ILPs, 8 merged leaves."""
    hist = {}
    for name in sorted(fuzz_util.CRAFTED):
        c = fuzz_util.oracle_run(fuzz_util.crafted_scene(name, "ct"))["census"]
        h = fuzz_util.group_histogram(c["groups"])
        print(name, c["ilp"], c["cluster"], c["L"], c["merged_leaves"], h)
        assert c["merged_leaves"] > 0, name
        for s, n in h.items():
            hist[s] = hist.get(s, 0) + n
    assert all(hist.get(s, 0) >= 1 for s in (3, 5, 6, 7)), hist
    assert any(s > 16 for s in hist), hist


def _slice_census(seeds, similar):
    total = {}
    for seed in seeds:
        fuzz_util.add_census(total, fuzz_util.oracle_run(fuzz_util.ct_scene(seed, similar), MAX_LEAVES)["census"])
    return total


def test_plain_slice_census():
    """12 seeds, leaf cap 1 500.  Oracle alone: 315 ILPs, largest cluster 50 targets, 157 terminations, largest scan 4 969 leaves, all
    five kinds of turn rate, 32 (target, scan) with more than 64 candidates (the longest list 98), the largest target 431 leaves."""
    c = _slice_census(PLAIN_SEEDS, False)
    print(c["ilp"], c["cluster"], c["dead"], c["L"], c["kinds"], sum(g["cand"] > 64 for g in c["grow"]), max(g["cand"] for g in c["grow"]),
          max(g["leaves"] for g in c["grow"]))
    assert c["kinds"] == list(range(fuzz_util.CT_KINDS)), c["kinds"]
    assert c["dead"] > 0 and c["ilp"] > 0 and c["cluster"] >= 5, (c["dead"], c["ilp"], c["cluster"])
    assert any(g["cand"] > 64 for g in c["grow"])
    assert not c["groups"]


def test_similar_slice_census():
    """12 seeds with similar-state pruning on three scans of four.  Oracle alone: 1 407 merged groups (1 370 of one hit, 35 of two, 2 of
    three), 344 ILPs, largest cluster 57 targets, 92 terminations, largest scan 2 513 leaves, the largest target 290 leaves."""
    c = _slice_census(SIMILAR_SEEDS, True)
    print(c["ilp"], c["cluster"], c["dead"], c["L"], c["kinds"], fuzz_util.group_histogram(c["groups"]), max(g["leaves"] for g in c["grow"]))
    assert c["kinds"] == list(range(fuzz_util.CT_KINDS)), c["kinds"]
    assert c["dead"] > 0 and c["ilp"] > 0 and c["cluster"] >= 5, (c["dead"], c["ilp"], c["cluster"])
    assert len(c["groups"]) >= 20 and max(c["groups"]) >= 3, fuzz_util.group_histogram(c["groups"])
    assert max(g["leaves"] for g in c["grow"]) > fuzz_util.CT_CHUNK      # (pruning inside a target of more than one chunk)


@pytest.mark.parametrize("N", [8, 9])
def test_long_window_census(N):
    """Windows of 8 and 9 scans under models.ct (fgrow_ct_kernel<4>: path records of 16 ints).  Oracle alone: N = 8: 12 scans, 17 ILPs,
    largest scan 2 544 leaves, the largest target 413 leaves; N = 9, stopped behind the first scan of more than 4 000 leaves: 10 scans,
    16 ILPs, largest scan 4 780 leaves, the largest target 1 272 leaves."""
    c = fuzz_util.oracle_run(fuzz_util.ct_long_window_scene(N), fuzz_util.CT_LONG_CAP[N])["census"]
    big = max(g["leaves"] for _, _, g in fuzz_util.ct_grow_rows(c))
    print(N, c["scans"], c["ilp"], c["cluster"], c["L"], big)
    assert c["scans"] > N and big > fuzz_util.CT_CHUNK and c["ilp"] > 0, (c["scans"], big, c["ilp"])
