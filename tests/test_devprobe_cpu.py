"""No GPU: the probe library of the hot path's helper headers (tests/devprobe/probe.hip over csrc/mht_wave.h, mht_uf.h, mht_vtab.h)
cross-compiles in both builds with the library's own flags -- a header that drifts away from the probes shows here --, and the host
references tests/test_devprobe_gpu.py holds the helpers to check themselves: the pairwise tree against math.fsum, the host union-find
against the oracle's find_clusters on every graph of the GPU tests, the value generators against the number of distinct values they
state."""
import subprocess

import numpy as np
import pytest

import devprobe_util as U
import mht_oracle


@pytest.mark.parametrize("nx", [4, 6])
def test_probe_cross_compiles(tmp_path, nx):
    from pymht_amd import build as B
    so = str(tmp_path / "probe.so")
    cmd = U.build_command(so, nx)
    for f in ("--offload-arch=gfx950", "-ffp-contract=off", "-O3"):
        assert f in B.FLAGS and f in cmd
    assert ("-DMHT_NX=6" in cmd) == (nx == 6)
    assert not any(s.startswith("tests") or "devprobe" in s for s in B.SOURCES), "the probe is no part of the library"
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ("probe_scan_u32", "probe_scan_halves", "probe_sum_i32", "probe_min_i32", "probe_max_i32", "probe_box_i32", "probe_sum_f64", "probe_min_value",
                 "probe_row16_min_value", "probe_min_pair", "probe_row16_min_pair", "probe_uf_link", "probe_uf_claim", "probe_vt_insert", "probe_vt_load"):
        assert " T " + name + "\n" in syms, name


def test_pairwise_tree_against_fsum():
    """|tree - fsum| <= 6 * 2^-53 * sum|v| on the finite inputs of the GPU test and on 2 000 random vectors spanning 16 decades"""
    rng = np.random.default_rng(1)
    x = np.concatenate([U.sum_inputs(), rng.standard_normal((2000, 64)) * 10.0 ** rng.uniform(-8, 8, (2000, 64))])
    tree = U.pairwise_tree(x)
    exact, mag = U.fsum_rows(x)
    ok = mag > 0
    worst = np.max(np.abs(tree - exact)[ok] / mag[ok]) / 2.0 ** -53
    print("pairwise tree: worst |error| = %.2f * 2^-53 * sum|v| over %d rows" % (worst, len(x)))
    assert (np.abs(tree - exact) <= U.FSUM_BOUND * mag).all()
    # the tree is what it says: lane pairs first
    one = np.arange(64, dtype=np.float64)
    assert U.pairwise_tree(one) == 2016.0
    assert np.signbit(U.pairwise_tree(np.full(64, -0.0)))
    # ... and not the running sum: an input on which the two orders round differently
    y = np.array([1.0, 2.0 ** -53, 2.0 ** -53] + [0.0] * 61)
    assert U.pairwise_tree(y) != np.cumsum(y[::-1])[-1]


@pytest.mark.parametrize("name", sorted(U.link_graphs()))
def test_host_uf_against_oracle_link_graphs(name):
    T, ex, ey = U.link_graphs()[name]
    assert T <= 20000 and len(ex) == len(ey) <= 200000
    assert len(ex) == 0 or (0 <= min(ex.min(), ey.min()) and max(ex.max(), ey.max()) < T)
    lab = U.host_uf(T, ex, ey)
    assert (lab == U.labels_of_clusters(mht_oracle.find_clusters(U.edges_as_sets(T, ex, ey)), T)).all()
    n = len(np.unique(lab))
    print(name, "T", T, "E", len(ex), "components", n)
    if name == "sparse_random":
        assert 100 <= n <= 1000
    if name.startswith(("path", "star")):
        assert n == 1


def test_host_uf_against_oracle_epoch_graphs():
    for epoch, T, ex, ey in U.epoch_graphs():
        assert T == 20000 and ex.max() < T and ey.max() < T and min(ex.min(), ey.min()) >= 0
        assert (U.host_uf(T, ex, ey) == U.labels_of_clusters(mht_oracle.find_clusters(U.edges_as_sets(T, ex, ey)), T)).all()


@pytest.mark.parametrize("AW", U.CLAIM_AW)
def test_host_uf_against_oracle_claim_scenes(AW):
    sc = U.claim_scenes(AW)
    assert sorted(sc) == ["dense_rows", "disjoint", "one_shared_node", "sparse"]
    for name, sets in sc.items():
        T = len(sets)
        assert T <= 3000
        lab = U.labels_of_clusters(mht_oracle.find_clusters(sets), T)
        assert (U.host_uf(T, *U.sets_as_edges(sets)) == lab).all(), name
        bits = U.sets_as_bits(sets, AW)
        pop = np.array([[bin(int(w)).count("1") for w in row] for row in bits])
        assert (pop.sum(axis=1) == [len(s) for s in sets]).all()
        n = len(np.unique(lab))
        print("AW", AW, name, "T", T, "components", n, "most bits in a word", pop.max())
        if name == "dense_rows":
            assert pop.max() == 64 and ((pop > 4) & (pop < 64)).any()
        if name == "one_shared_node":
            assert n == 1 and T == 3000
        if name == "disjoint":
            assert n == T
        if name == "sparse" and AW > 1:
            assert n >= 100 and n < T - 100


@pytest.mark.parametrize("nx", [4, 6])
def test_value_generators(nx):
    for vals, distinct in ((U.random_f32_values(nx, 3000, 21), 3000), (U.random_f64_values(nx, 300, 22), 300), U.near_values(nx),
                           (U.random_f32_values(nx, 160, 23), 160), (U.random_f64_values(nx, 160, 24), 160), (U.collision_values(nx)[0], U.COLLISION_VALUES)):
        assert len(set(vals.keys())) == distinct
        assert vals.words.shape[1] == nx * nx
    r = U.requests(3000, 60, 4)
    assert (np.bincount(r) == 60).all() and len(r) == 180000


@pytest.mark.parametrize("nx", [4, 6])
def test_collision_values(nx):
    """the 40 values for 64 slots do what their generator says under the restated hash: twice one tag twice at one start slot -- values that
    differ in the last word only, and one covariance under two P_d --, chains over the end"""
    vals, pairs = U.collision_values(nx)
    for a, b in pairs:
        ta, la = vals.hash(a)
        tb, lb = vals.hash(b)
        assert ta == tb and (la & 63) == (lb & 63) and vals.key(a) != vals.key(b)
    (a, b), (c, d) = pairs
    pw = nx * nx // 2
    assert (vals.words[a, :pw - 1] == vals.words[b, :pw - 1]).all() and vals.words[a, pw - 1] != vals.words[b, pw - 1] and vals.pd[a] == vals.pd[b]
    assert (vals.words[c] == vals.words[d]).all() and vals.pd[c] != vals.pd[d] and 0.5 <= vals.pd[c] < 1 and 0.5 <= vals.pd[d] < 1
    start = [vals.hash(v)[1] & 63 for v in range(len(vals))]
    end = U.probe_slots(vals, 64)
    wrapped = sum(1 for s, e in zip(start, end) if e < s)
    longest = max((e - s) & 63 for s, e in zip(start, end))
    print("values that end in front of their start slot:", wrapped, "longest probe:", longest)
    assert wrapped >= 3 and sum(1 for s in start if s >= 61) >= 12
    assert len(vals) * 8 <= 64 * 5
    assert U.table_size(100) == 512 and U.table_size(3000) == 16384 and U.table_size(64) == 256
