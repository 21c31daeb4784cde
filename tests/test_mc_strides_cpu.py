"""CPU: the cases of tests/test_mc_strides_gpu.py reach what they claim to reach, each is the smallest of its kind, and none of them is
vacuous.  The thresholds are recomputed from the constants of csrc/mht_mc.h, mht_mc_seam.h, mht_mc_zone.h and mht_mc_domain.h, read as
text; the scenes of tests/mc_stride_util.py are run on the host twins and held to their own conditions -- counts behind the threshold
that are neither 0 nor S, columns that differ, statuses as stated; M1, the cheapest (16 s), is held to the NumPy reference as well, with
no borderline particle (the others were, once: profiles/mc_stride_shapes.txt)."""
import os
import time

import numpy as np
import pytest

import mc_domain_ref as dref
import mc_pair_ref as pref
import mc_ref as ref
import mc_stride_util as u
import mc_zone_ref as zref
from test_encounter_strides_cpu import ROOT, ceil_div, constants


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    d = tmp_path_factory.mktemp("mc_stride_twins")
    return dict(own=ref.build_twin(d), pair=pref.build_twin(d), zone=zref.build_twin(d), domain=dref.build_twin(d))


def timed(label, make):
    t = time.perf_counter()
    res = make()
    print("%s: %.1f s" % (label, time.perf_counter() - t))
    return res


def test_every_case_lies_behind_the_threshold_it_is_there_for_and_is_the_smallest_that_does():
    mc, seam, zone, dom = constants("mht_mc.h"), constants("mht_mc_seam.h"), constants("mht_mc_zone.h"), constants("mht_mc_domain.h")
    threads, cap = int(mc["MC_THREADS"]), int(seam["MC_MAX_BLOCKS"])
    G, K = int(mc["MC_MAX_PATHS"]), int(mc["MC_MAX_STEPS"])
    Z, ZV = int(zone["MC_ZONE_MAX_ZONES"]), int(zone["MC_ZONE_MAX_VERTS"])
    D, DV, DC = int(dom["MC_DOMAIN_MAX_DOMAINS"]), int(dom["MC_DOMAIN_MAX_VERTS"]), int(dom["MC_DOMAIN_MAX_CELLS"])
    text = open(os.path.join(ROOT, "pymht_amd", "csrc", "mht_mc.h")).read()
    assert "constexpr int MC_MAX_PARTICLES = 1 << 20;" in text and int(mc["MC_FILL"]) == ref.FILL and threads == ref.THREADS
    assert (cap, threads, cap * threads) == (2048, 256, u.TRIP) and (G, K) == (u.G_MAX, u.K_MAX) == (ref.MAX_PATHS, ref.MAX_STEPS)
    assert (Z, ZV, D, DV, DC) == (32, 1024, 4, 256, 64) == (zref.MAX_ZONES, zref.MAX_VERTS, dref.MAX_DOMAINS, dref.MAX_VERTS, dref.MAX_CELLS)
    fold = lambda words, items: (words + 1) * items      # what mc_fold_kernel strides over: the count words and the items' status
    # M1: every limit of the own ship; 124 targets are not behind the cap, 125 are (the case takes scene A's 70 nearly twice over)
    sc = u.m1()
    words = G * (K + 2)
    assert (len(sc["own"]), sc["K"], len(sc["first"]) - 1, sc["S"]) == (G, K, u.M1_T, 64) and sc["own"].shape == (G, K + 1, 2)
    assert fold(words, u.M1_T) == 549250 > u.TRIP >= fold(words, 124) and words * u.M1_T > u.TRIP
    assert G * (K + 1) * u.M1_T - u.TRIP == 24832 - G * u.M1_T == 16512      # `within` words behind the cap: end0 is crossed in trip 2
    assert ref.chunks(u.M1_T, 64) == (1, 256)
    # M2: 131 words a pair; 3 971 pairs are not behind the cap; firstAt ends, and ever lies, in trip 2: end1 is crossed there
    sc, pairs = u.m2()
    words = 2 * (K + 1) + 1
    assert pairs.shape == (u.M2_PAIRS, 2) and pairs.max() < u.M1_T and words * u.M2_PAIRS == 537100 > u.TRIP >= fold(words, 3971)
    assert (K + 1) * u.M2_PAIRS < u.TRIP < 2 * (K + 1) * u.M2_PAIRS and 2 * (K + 1) * u.M2_PAIRS - u.TRIP == 8712
    # M3: 32 zones, 1 024 vertices, 64 steps; 125 targets are not behind the cap
    sc, zones = u.m3()
    words = 2 * Z * (K + 1) + Z
    assert len(zones) == Z and sum(len(z) for z in zones) == ZV and sc["K"] == K and len(sc["first"]) - 1 == u.M1_T
    assert words * u.M1_T == 544960 > u.TRIP >= fold(words, 125) and Z * (K + 1) * u.M1_T < u.TRIP < 2 * Z * (K + 1) * u.M1_T
    # M4: 64 cells, 256 vertices, 64 steps; 62 targets are not behind the cap (the case takes scene A whole)
    sc, doms, poses = u.m4()
    words = 2 * DC * (K + 1) + DC
    assert len(doms) == D and sum(len(d) for d in doms) == DV and len(doms) * len(poses) == DC and poses.shape == (16, K + 1, 4)
    assert words * u.M4_T == 586880 > u.TRIP >= fold(words, 62) and 2 * DC * (K + 1) * u.M4_T + DC * u.M4_T - u.TRIP == 62592
    # F1: the factor's second trip is 300 components, two workgroups; mc_target_flags takes over a thousand trips a lane
    first = u.F1_FIRST
    assert u.F1_NCOMP - u.TRIP == 300 and ceil_div(300, threads) == 2 and first[-1] == u.F1_NCOMP
    assert first[u.F1_STRADDLES] < u.TRIP < first[u.F1_STRADDLES + 1] and (first[u.F1_BEHIND:] > u.TRIP).all()
    assert ceil_div(int(first[1] - first[0]), threads) == 1024 and ceil_div(int(first[2] - first[1]), threads) == 1025
    assert (u.F1_DEEP_AT - first[1]) // threads == 1024 and first[1] <= u.F1_DEEP_AT < first[2]
    assert first[u.F1_NAN] <= u.F1_NAN_AT < first[u.F1_NAN + 1] and first[u.F1_INDEFINITE] <= u.F1_INDEFINITE_AT < first[u.F1_INDEFINITE + 1]
    # C1: the NaN in the second trip of mc_target_flags, the indefinite P in the third
    assert u.C1_NAN_AT // threads == 1 and u.C1_INDEFINITE_AT // threads == 2 and u.C1_N > 2 * threads
    # P1: the limit; 512 chunks of 2 048 are eight trips of a workgroup's slab loop
    assert u.P1_S == ref.MAX_PARTICLES == 1 << 20 and ref.chunks(2, u.P1_S) == (512, 2048) and ref.chunks(1, u.P1_S) == (1024, 1024)
    assert 2048 // threads == 8 and ref.chunks(1, 65536) == (256, 256)      # (the largest S of the older tests: one trip a workgroup)


def test_m1_to_m4_have_live_counts_behind_the_threshold(twins):
    sc = u.m1()
    m1 = timed("M1 twin", lambda: ref.call_twin(twins["own"], sc))
    u.check_fold_scene("M1", m1, ("within", "ever"), u.M1_T, sc["S"])
    want = timed("M1 NumPy reference", lambda: ref.reference(sc))
    assert ref.same_counts(m1, want) and int(want["borderWithin"].sum()) == 0 and int(want["borderEver"].sum()) == 0
    sc, pairs = u.m2()
    out = timed("M2 twin", lambda: pref.call_twin(twins["pair"], sc, pairs))
    u.check_fold_scene("M2", out, ("within", "firstAt", "ever"), len(pairs), sc["S"], u.M2_LEAST, distinct=False)
    pref.check_invariants(out)
    assert int((out["ever"] > 0).sum()) >= 500
    sc, zones = u.m3()
    out = timed("M3 twin", lambda: zref.call_twin(twins["zone"], sc, zones))
    u.check_fold_scene("M3", out, ("inside", "firstAt", "ever"), u.M1_T, sc["S"])
    zref.check_invariants(out)
    sc, doms, poses = u.m4()
    out = timed("M4 twin", lambda: dref.call_twin(twins["domain"], sc, doms, poses))
    u.check_fold_scene("M4", out, ("inside", "firstAt", "ever"), u.M4_T, sc["S"])
    dref.check_invariants(out)


@pytest.mark.parametrize("N", [4, 6])
def test_f1_scores_the_targets_behind_the_threshold_and_its_radius_is_the_components_sigma(twins, N):
    sc = u.f1(N)
    out = timed("F1 twin, %d states" % N, lambda: ref.call_twin(twins["own"], sc))
    u.check_f1(out)
    # R of the size of the position sigma: a particle drawn without its factor -- at its component's mean -- would count differently
    sigma = np.sqrt(np.linalg.eigvalsh(sc["P"][u.TRIP + 10][:2, :2]))
    assert sigma[0] < sc["R"] < sigma[1] * 1.5 and sigma[1] > 0.5 * sc["R"], sigma
    flat = dict(sc, P=sc["P"] * 1e-12)
    flat["P"][u.F1_INDEFINITE_AT, 0, 0] = flat["P"][u.F1_DEEP_AT, 1, 1] = -1.0
    mean = ref.call_twin(twins["own"], flat)
    for t in (u.F1_STRADDLES, u.F1_BEHIND):
        assert (mean["ever"][:, t] != out["ever"][:, t]).all(), (t, mean["ever"][:, t], out["ever"][:, t])


@pytest.mark.parametrize("N", [4, 6])
def test_c1_statuses_and_a_count_that_depends_on_the_pick(twins, N):
    sc, near = u.c1(N), u.c1(N, far_weight=0.0)
    lo = u.C1_SCORED * u.C1_N
    cdf = sc["cdf"][lo:lo + u.C1_N]      # (no weight at either end: the pick's search must stop inside, and its uniforms end at 1 - 2^-33)
    assert cdf[0] == cdf[1] == 0.0 < cdf[2] and cdf[-3] > 1.0 - 1e-12 and (np.diff(cdf[1:-2]) > 0.0).all() and np.array_equal(sc["x"], near["x"], equal_nan=True)
    zones, (doms, poses) = u.c1_zones(), u.c1_domains()
    runs = dict(own=lambda s: ref.call_twin(twins["own"], s), pair=lambda s: pref.call_twin(twins["pair"], s, u.C1_PAIRS),
                zone=lambda s: zref.call_twin(twins["zone"], s, zones), domain=lambda s: dref.call_twin(twins["domain"], s, doms, poses))
    for seam, run in runs.items():
        a, b = run(sc), run(near)
        assert a["status"].tolist() == (u.C1_PAIR_STATUS if seam == "pair" else u.C1_STATUS) and np.array_equal(a["status"], b["status"]), seam
        mine = (lambda o: o["ever"][4:]) if seam == "pair" else (lambda o: o["ever"][..., u.C1_SCORED])
        print("C1, %d states, %s: ever %s, with the far components unpicked %s" % (N, seam, mine(a).ravel().tolist(), mine(b).ravel().tolist()))
        assert (mine(a) != mine(b)).all() and ((mine(a) > 0) & (mine(a) < sc["S"])).all(), seam


def test_p1_counts_near_a_million(twins):
    sc = u.p1()
    out = timed("P1 own ship twin", lambda: ref.call_twin(twins["own"], sc))
    assert out["valid"].tolist() == [u.P1_S] * 2 and (out["ever"][:, 0] == u.P1_S).all() and ((out["ever"][:, 1] > 100000) & (out["ever"][:, 1] < 200000)).all()
    sc, pairs = u.p1_pair()
    out = timed("P1 pair twin", lambda: pref.call_twin(twins["pair"], sc, pairs))
    pref.check_invariants(out)
    assert out["valid"].tolist() == [u.P1_S] and 100000 < out["ever"][0] < u.P1_S - 100000 and (out["within"][:, 0] > 1000).all()
