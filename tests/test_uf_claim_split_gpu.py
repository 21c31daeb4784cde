"""GPU: the union-find's claim (csrc/mht_uf.h: uf_claim) walks ALL the words a lane owns (lane, lane + 64, ...) as one sequence of nodes and
sends up to four exchanges per lane and round counted over all 64-word chunks of the bitset together -- run through the probe library's
k_uf_claim (tests/devprobe/probe.hip, built by devprobe_util, both unchanged), which is shaped like the grow launch's target workgroup.

(The file's name is from the first form of the change, which split the claim in two around the workgroup's barrier; that form was measured
and dropped, profiles/claim_split.txt.)

Scenes, bit packing, forest check and the reference (mht_oracle.find_clusters) are those of tests/test_devprobe_gpu.py::test_uf_claim,
imported from devprobe_util unchanged; what is asserted is what that test asserts.  On top of its AW (one, two and three 64-word chunks of
the bitset) the headline's AW = 144 runs a scene of its own: targets with nodes in all three chunks of ONE lane (words L, L + 64, L + 128)
and with more than four nodes in a lane -- more than a lane sends in one round, spread over several words, so the second round starts in
the middle of the lane's walk."""
import numpy as np
import pytest

import devprobe_util as U
import mht_oracle

pytestmark = pytest.mark.gpu

HEADLINE_AW = 144


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (pymht_amd has no CPU fallback)")
    return U.build(tmp_path_factory.mktemp("devprobe_claim"), 4)      # (mht_uf.h does not depend on the state dimension)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64).copy()).to("cuda")


def headline_scene():
    """AW = 144: lane L < 16 owns words L, L + 64 and L + 128.  Three kinds of targets, 75 per lane, nodes drawn from the lane's words so that
    targets of a lane meet: seven nodes over all three chunks of the lane; a full third-chunk word (64 nodes in one lane) and a node in the
    first; one node in the second chunk and a few anywhere."""
    rng = np.random.default_rng(144)
    AW, sets = HEADLINE_AW, []
    pick = lambda w, k: (w * 64 + rng.choice(64, k, replace=False)).tolist()
    for t in range(1200):
        L, kind = t % 16, (t // 16) % 3
        if kind == 0:
            s = pick(L, 2) + pick(L + 64, 2) + pick(L + 128, 3)
        elif kind == 1:
            s = list(range((L + 128) * 64, (L + 128) * 64 + 64)) + pick(L, 1) if t < 48 else pick(L + 128, 6) + pick(L, 1)
        else:
            s = pick(L + 64, 1) + rng.choice(AW * 64, 3, replace=False).tolist()
        sets.append(sorted(set(s)))
    return sets


def _per_lane(s):
    """nodes per lane, and the chunks each lane's nodes lie in"""
    n, ch = {}, {}
    for m in s:
        lane = (m >> 6) & 63
        n[lane] = n.get(lane, 0) + 1
        ch.setdefault(lane, set()).add(m >> 12)
    return n, ch


def test_headline_scene_reaches_the_remainder_loop():
    sets = headline_scene()
    three, many, full = 0, 0, 0
    for s in sets:
        n, ch = _per_lane(s)
        three += any(len(c) == 3 for c in ch.values())
        many += max(n.values()) > 4
        full += max(n.values()) >= 64
    assert three >= 300 and many >= 600 and full >= 16, (three, many, full)
    sizes = [len(c) for c in mht_oracle.find_clusters(sets)]
    assert max(sizes) > 10 and sizes.count(1) > 0, "components of several targets, and targets alone"


def _claim(lib, d_owner, d_parent, bits, AW, epoch, cap):
    import torch
    T = len(bits)
    d_assoc = dev(bits.reshape(-1))
    d_nconf = torch.full((T,), -9, dtype=torch.int32, device="cuda")
    rc = lib.probe_uf_claim(d_assoc.data_ptr(), T, AW, d_owner.data_ptr(), d_parent.data_ptr(), epoch, cap, d_nconf.data_ptr())
    assert rc == 0, rc
    return d_parent.cpu().numpy().view(np.uint64), d_nconf.cpu().numpy()


def _scenes(AW):
    sc = dict(U.claim_scenes(AW))
    if AW == HEADLINE_AW:
        sc["three_chunks_of_a_lane"] = headline_scene()
    return sc


@pytest.mark.parametrize("AW", U.CLAIM_AW + (HEADLINE_AW,))
def test_uf_claim_split(lib, AW):
    """The components are the oracle's at every cap, 0 included; 0 <= nconf <= cap (the number depends on who came first), 0 where no two
    targets share a node; exactly the nodes in use carry the epoch."""
    import torch
    for name, sets in _scenes(AW).items():
        T, bits = len(sets), U.sets_as_bits(sets, AW)
        ref = U.labels_of_clusters(mht_oracle.find_clusters(sets), T)
        used = np.zeros(AW * 64, dtype=bool)
        used[[m for s in sets for m in s]] = True
        for cap in U.CLAIM_CAP:
            d_owner = torch.zeros(AW * 64, dtype=torch.int64, device="cuda")
            d_parent = torch.zeros(T, dtype=torch.int64, device="cuda")
            words, nconf = _claim(lib, d_owner, d_parent, bits, AW, 2, cap)
            assert ((nconf >= 0) & (nconf <= cap)).all(), (name, cap, nconf.min(), nconf.max())
            if name == "disjoint":
                assert (nconf == 0).all()
            try:
                U.check_forest(words, 2, ref)
            except AssertionError as e:
                raise AssertionError("AW %d, %s, cap %d: %s" % (AW, name, cap, e))
            owner = d_owner.cpu().numpy().view(np.uint64)
            assert ((owner >> np.uint64(32)) == np.where(used, 2, 0).astype(np.uint64)).all(), "owner words: exactly the nodes in use carry this epoch"


@pytest.mark.parametrize("AW", [1, 65, HEADLINE_AW])
def test_uf_claim_split_two_scans_on_the_same_arrays(lib, AW):
    """owner and parent words are never cleared: a scan under epoch 2, then other scenes under epochs 4 and 6 -- their labels are their own"""
    import torch
    sc = _scenes(AW)
    d_owner = torch.zeros(AW * 64, dtype=torch.int64, device="cuda")
    d_parent = torch.zeros(3000, dtype=torch.int64, device="cuda")
    order = [(2, "one_shared_node"), (4, "sparse"), (6, "dense_rows")] + ([(8, "three_chunks_of_a_lane")] if AW == HEADLINE_AW else [])
    for epoch, name in order:
        sets = sc[name]
        words, nconf = _claim(lib, d_owner, d_parent, U.sets_as_bits(sets, AW), AW, epoch, 3)
        assert ((nconf >= 0) & (nconf <= 3)).all()
        U.check_forest(words, epoch, U.labels_of_clusters(mht_oracle.find_clusters(sets), len(sets)))
