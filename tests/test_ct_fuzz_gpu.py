"""GPU: the CONSTANT-TURN forest -- Tracker(pymht_amd.models.ct, ...): fgrow_ct_kernel (hit masks over the target's candidate list: one to
FG_HWC = 6 words per leaf in LDS, full-width masks in global memory past 384 candidates), forest_ct_kernel, prune_similar_kernel's
constant-turn branch -- held to the live oracle on scenes that stop on the leaf cap alone (fuzz_util.oracle_run / device_run; the random
slices of tests/test_fuzz_gpu.py and tests/test_ct_forest_gpu.py stop on a clock and never meet a candidate list of more than two words).
Decisions -- L, G, unused measurements, target ids and terminations, clusters member for member, selections, leaf ids and measurement
numbers, ILPs -- exact; states and covariances of all leaves 1e-6.  What every scene reaches is asserted from the oracle alone, without a
device, in tests/test_ct_fuzz_cpu.py; the figures in the docstrings below are that census (profiles/fuzz_ct_census.txt).

A gate decision the device takes the other way is a kernel bug unless the oracle's own NIS of that pair lies within float32 rounding of eta2
(Phi(T, w) one ulp off NumPy's): such a seed is replaced and the pair written down here.  None so far."""
import pytest

import fuzz_util
from fuzz_util import CT_PLAIN_SEEDS as PLAIN_SEEDS, CT_SIMILAR_SEEDS as SIMILAR_SEEDS, CA_MAX_LEAVES as MAX_LEAVES

pytestmark = pytest.mark.gpu

_RECORDS = {}


def _record(key, scene_of, cap=None):
    """(scene, the oracle's record), made once per module and only read afterwards."""
    if key not in _RECORDS:
        scene = scene_of()
        _RECORDS[key] = (scene, fuzz_util.oracle_run(scene, cap))
    return _RECORDS[key]


def _held(key, scene_of, cap=None, **kw):
    scene, rec = _record(key, scene_of, cap)
    ok, msg = fuzz_util.device_run(scene, rec, **kw)
    print(scene["desc"], msg)
    assert ok, scene["desc"] + ' ' + msg
    return rec["census"]


@pytest.mark.parametrize("seed", PLAIN_SEEDS)
def test_ct_fuzz_slice_against_oracle(seed):
    """12 random scenarios with random turn rates (exactly 0, below the straight-line threshold, gentle, up to 0.6 rad/s), looked at after
    every scan.  Census (oracle) of the slice: 315 ILPs, largest cluster 50 targets, 157 terminations, largest scan 4 969 leaves, 32
    (target, scan) with more than 64 candidates (at most 98), the largest target 431 leaves."""
    _held(("slice", seed, False), lambda: fuzz_util.ct_scene(seed, False), MAX_LEAVES)


@pytest.mark.parametrize("seed", SIMILAR_SEEDS)
def test_ct_fuzz_slice_with_similar_state_pruning(seed):
    """12 scenarios with similar-state pruning on three scans of four and a random merge radius.  Census (oracle) of the slice: 1 407 merged
    groups (1 370 of one hit, 35 of two, 2 of three), 344 ILPs, largest cluster 57 targets, 92 terminations, the largest target 290 leaves."""
    _held(("slice", seed, True), lambda: fuzz_util.ct_scene(seed, True), MAX_LEAVES)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_ct_similar_state_pruning_large_groups(name):
    """The dense scenes of the linear forests under models.ct, pruning on at every scan: the merged node keeps the missed-detection child's
    key, and a mean over n hits that is none of the hits' covariances is written over the parent's P_bar entry (csrc/mht_similar.hip).  The
    covariance of every merged leaf is held to the oracle's np.mean at 1e-6; no leaf carries flag 8.  Census (oracle), group size: count --
    A {1: 75, 2: 33, 3: 8, 4: 4, 5: 1, 6: 1}, 112 merged leaves; B {1: 35, 2: 10, 3: 11, 4: 7, 5: 2, 6: 2, 7: 1}, 33 merged leaves;
    C {3: 7, 4: 9, 5: 6, 6: 10, 7: 6, 8: 8, 10: 3, 14: 1, 18: 1, 20: 1, 21: 1} and 8 smaller, 8 merged leaves."""
    c = _held(("crafted", name), lambda: fuzz_util.crafted_scene(name, "ct"))
    assert c["merged_leaves"] > 0 and max(c["groups"]) >= 6


def test_ct_similar_state_pruning_with_forced_spill():
    """Crafted B once more with every target's hit masks in the global block (MHT_CT_SPILL=1): the same record."""
    _held(("crafted", "B"), lambda: fuzz_util.crafted_scene("B", "ct"), spill=True)


@pytest.mark.parametrize("spill", [False, True])
@pytest.mark.parametrize("name", sorted(fuzz_util.WIDE_GATE))
def test_ct_wide_gates(name, spill):
    """Two scans of dense clutter in which root 0 starts with a position variance of sigma^2: candidate lists of two to six words in LDS
    and, past 384 candidates, full-width masks in global memory -- in one launch with targets that stay in LDS (a, scan 1), over three chunks
    and two passes with several thousand children per chunk (a, scan 2).  spill: the same record with every target forced through the
    global block.  Census (oracle), (candidates, leaves) of the targets with more than 64 candidates, scan 1 | scan 2:
    a (416, 1) | (608, 333) (77, 8), all three tracks terminate;  b (249, 1) | (150, 208);  c (239, 1) | (317, 192) (107, 14) (119, 16) (84, 11);
    d (322, 1) | (336, 262);  e (307, 1) | (176, 255).  The candidate counts are lower bounds on the device's lists."""
    c = _held(("wide", name), lambda: fuzz_util.wide_gate_scene(name), spill=spill)
    assert c["scans"] == 2


@pytest.mark.parametrize("N", [8, 9])
def test_ct_long_window(N):
    """Windows of 8 and 9 scans (fgrow_ct_kernel<4>: path records of 16 ints; targets of several chunks).  Census (oracle): N = 8: 12 scans,
    17 ILPs, largest scan 2 544 leaves, the largest target 413 leaves; N = 9, stopped behind the first scan of more than 4 000 leaves: 10
    scans, 16 ILPs, largest scan 4 780 leaves, the largest target 1 272 leaves."""
    c = _held(("long", N), lambda: fuzz_util.ct_long_window_scene(N), fuzz_util.CT_LONG_CAP[N])
    assert max(g["leaves"] for _, _, g in fuzz_util.ct_grow_rows(c)) > fuzz_util.CT_CHUNK


def test_ct_streamed_slice_scene():
    """A host that streams the scans in and looks once at the end (the commits ride in the next scan's grow launch): the plain slice's
    scene with the longest candidate lists (98) and 4 969 leaves in its last scan."""
    seed = PLAIN_SEEDS[9]
    _held(("slice", seed, False), lambda: fuzz_util.ct_scene(seed, False), MAX_LEAVES, streamed=True)


def test_ct_streamed_wide_gate_scene():
    """Wide-gate scene a streamed: the spilling launch of scan 2 admits what scan 1 committed."""
    _held(("wide", "a"), lambda: fuzz_util.wide_gate_scene("a"), streamed=True)


def test_ct_forced_spill_in_a_pruned_target_of_several_chunks():
    """The similar-state slice's first scene (a target of 290 leaves, groups of up to three hits) with every target through the global block."""
    seed = SIMILAR_SEEDS[0]
    _held(("slice", seed, True), lambda: fuzz_util.ct_scene(seed, True), MAX_LEAVES, spill=True)
