"""CPU: the scene of tests/test_grow_claim_split_gpu.py reaches, on the oracle alone, the conditions that test is about
(grow_claim_split_util): the expected clusters are the oracle's own, found by mht_oracle.find_clusters on the sets the scan ran on."""
import numpy as np

import grow_claim_split_util as cs
import mht_oracle as orc


def _check(sc):
    cond = cs.shared_conditions(sc)
    n = len(sc["scans"])
    for k in range(n):      # the clusters recorded are what the oracle's clustering gives on the recorded sets
        want = orc.find_clusters(sc["assoc"][k])
        assert len(want) == len(sc["clusters"][k]) and all(np.array_equal(a, b) for a, b in zip(want, sc["clusters"][k])), k + 1
    for k in range(1, n):
        assert [c.tolist() for c in sc["clusters"][k]] == [[0, 1, 2], [3]], (k + 1, sc["clusters"][k])
    assert all(z.dtype == np.float32 and len(z) == 5 for z in sc["scans"])
    assert max(max(row) for row in sc["children"]) < (1 << 12), "the scene stays small"
    return cond


def test_shared_scene_four_state():
    sc = cs.shared_scene()
    cond = _check(sc)
    assert sc["N"] == 5 and (sc["N"] + cs.RING_EXTRA) * cs.SLOT_WORDS == 144, "the headline's bitset: 144 words, three chunks"
    assert max(cond["two_pass"]) >= 9 and max(cond["three_chunks"]) >= 9, "both at once in the late scans"
    # (b) in a scan of its own: the middle target's 87 leaves grow 254 children
    k = cond["last_wave"][0] - 1
    assert 64 < sc["leaves_in"][k][1] <= cs.CAP and sc["children"][k][1] > cs.LAST_WAVE_FROM


def test_shared_scene_constant_turn():
    from pymht_amd.models import ct
    sc = cs.shared_scene(model=ct)
    assert sc["x0"].shape[1] == 6
    _check(sc)
