"""GPU: the four Monte-Carlo seams where their loops go round more than once.  mc_factor_kernel and mc_fold_kernel, which
`mht_mc_encounters`, `mht_mc_pair_encounters`, `mht_mc_zone_encounters` and `mht_mc_domain_encounters` share, launch at most 2048
workgroups of 256 lanes and stride over the rest; mc_target_flags, inline in every walk kernel, strides over a target's components by 256
lanes; a walk workgroup strides over its slab.  The other GPU tests of the family fold a few tens of thousands of words, factor 1 030
components, have targets of 67 components and 65 536 particles at the most: every one of them ends inside the first trip of the fold's,
the factor's and the flags' loop.  The cases (tests/mc_stride_util.py; tests/test_mc_strides_cpu.py recomputes their thresholds from the
sources and holds the scenes' own conditions on the twins):

    M1  own ship  G = 64, K = 64, T = 130, S = 64            549 250 fold words; every limit of mc_walk_kernel at once
    M2  pairs     K = 64, 4 100 pairs                        537 100 fold words: end1 crossed in trip 2
    M3  zones     32 x 32 vertices, K = 64, T = 130          544 960
    M4  domains   4 x 64 vertices x 16 paths, K = 64, T = 70 586 880
    F1  own ship  nComp = 524 588, on each build its own model   the factor's trip 2; mc_target_flags over 262 000 components
    C1  all four  targets of 600 components                  trips 2 and 3 of mc_target_flags, mc_pick over 600
    P1  own ship, pairs   S = 1 048 576                       eight trips of the slab loop, counts up to 2^20, folds over 512 and 1 024 chunks

The criterion is the family's: the counts EQUAL the host twin's (the NumPy reference and its borderline rule are called only if one
differs; every test prints the number of cells that do), no sentinel left, the seam's invariants.  Every call runs on a work buffer
filled with a pattern, with 4 KB of it behind the sizer's figure that must be untouched: a factor trip that did not run leaves a
component's status at 0xA5A5A5A5 -- scored -- and its factor at -1e-127, a fold trip that did not run leaves the sentinel.

profiles/mc_stride_shapes.txt records the seams' times and the mutation check."""
import time

import numpy as np
import pytest

import mc_domain_ref as dref
import mc_pair_ref as pref
import mc_ref as ref
import mc_stride_util as u
import mc_zone_ref as zref
from test_encounter_strides_gpu import seam_time
from test_mc_domain_gpu import _hold as hold_domain
from test_mc_domain_gpu import _raw as raw_domain
from test_mc_gpu import _hold as hold_own
from test_mc_gpu import _raw as raw_own
from test_mc_pair_gpu import _hold as hold_pair
from test_mc_pair_gpu import _raw as raw_pair
from test_mc_zone_gpu import _hold as hold_zone
from test_mc_zone_gpu import _raw as raw_zone

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def ctxs():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (pymht_amd has no CPU fallback)")
    from pymht_amd.device import Context
    c = {4: Context(0, nx=4), 6: Context(0, nx=6)}
    yield c
    for v in c.values():
        v.close()


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    d = tmp_path_factory.mktemp("mc_stride_twins")
    return dict(own=ref.build_twin(d), pair=pref.build_twin(d), zone=zref.build_twin(d), domain=dref.build_twin(d))


def twin_of(label, make):
    t = time.perf_counter()
    res = make()
    print("%s: twin %.1f s" % (label, time.perf_counter() - t))
    return res


# ---- the fold ------------------------------------------------------------------------------------------------------------------------
def test_m1_own_ship_at_every_limit_the_fold_strides(ctxs, twins):
    """M1: G = 64, K = 64, T = 130, S = 64.  (4224 + 1) * 130 = 549 250 words: the fold's second trip writes `within` from word 524 288
    on, all of `ever`, valid and status, and crosses end0; mc_walk_kernel's closing stores read cnt[63 * 65 + 64] and the last `ever`."""
    sc = u.m1()
    want = twin_of("M1", lambda: ref.call_twin(twins["own"], sc))
    for lib_nx in (4, 6):
        label = "M1 G 64 K 64 T 130 S 64, %d-state build" % lib_nx
        with seam_time(label, ctxs[lib_nx], "mht_mc_encounters"):
            rc, got = raw_own(ctxs[lib_nx], sc, guard=GUARD)
        assert rc == 0
        assert hold_own(label, got, want, sc) == 0
        assert (got["ever"] >= got["within"].max(axis=1)).all() and (got["valid"] == np.where(got["status"] == 0, sc["S"], 0)).all()
    u.check_fold_scene("M1", want, ("within", "ever"), u.M1_T, sc["S"])


def test_m2_4100_pairs_the_fold_strides_over_three_arrays(ctxs, twins):
    """M2: K = 64 and 4 100 pairs, 131 * 4 100 = 537 100 words: trip 2 writes the last rows of `firstAt` and all of `ever`, end1 crossed"""
    sc, pairs = u.m2()
    want = twin_of("M2", lambda: pref.call_twin(twins["pair"], sc, pairs))
    for lib_nx in (4, 6):
        label = "M2 K 64 4100 pairs S 64, %d-state build" % lib_nx
        with seam_time(label, ctxs[lib_nx], "mht_mc_pair_encounters"):
            rc, got = raw_pair(ctxs[lib_nx], sc, pairs, guard=GUARD)
        assert rc == 0
        assert hold_pair(label, got, want, sc, pairs) == 0
        assert (got["firstAt"].sum(axis=0, dtype=np.int64) == got["ever"]).all()
    u.check_fold_scene("M2", want, ("within", "firstAt", "ever"), len(pairs), sc["S"], u.M2_LEAST, distinct=False)


def test_m3_32_zones_of_32_vertices_the_fold_strides(ctxs, twins):
    """M3: Z = 32, 1 024 vertices, K = 64, T = 130: 4 192 * 130 = 544 960 words; the zone walk's closing stores read the last words of
    its LDS arrays"""
    sc, zones = u.m3()
    want = twin_of("M3", lambda: zref.call_twin(twins["zone"], sc, zones))
    for lib_nx in (4, 6):
        label = "M3 Z 32 nVert 1024 K 64 T 130 S 64, %d-state build" % lib_nx
        with seam_time(label, ctxs[lib_nx], "mht_mc_zone_encounters"):
            rc, got = raw_zone(ctxs[lib_nx], sc, zones, guard=GUARD)
        assert rc == 0
        assert hold_zone(label, got, want, sc, zones) == 0
    u.check_fold_scene("M3", want, ("inside", "firstAt", "ever"), u.M1_T, sc["S"])


def test_m4_64_cells_of_256_vertices_the_fold_strides(ctxs, twins):
    """M4: 4 domains of 64 vertices on 16 paths, K = 64, T = 70: 8 384 * 70 = 586 880 words; the domain walk's closing stores read
    cnt[2 * MC_DOMAIN_ROWS + 63]"""
    sc, doms, poses = u.m4()
    want = twin_of("M4", lambda: dref.call_twin(twins["domain"], sc, doms, poses))
    for lib_nx in (4, 6):
        label = "M4 4 x 16 cells nVert 256 K 64 T 70 S 64, %d-state build" % lib_nx
        with seam_time(label, ctxs[lib_nx], "mht_mc_domain_encounters"):
            rc, got, _ = raw_domain(ctxs[lib_nx], sc, doms, poses, guard=GUARD)
        assert rc == 0
        assert hold_domain(label, got, want, sc, doms, poses) == 0
    u.check_fold_scene("M4", want, ("inside", "firstAt", "ever"), u.M4_T, sc["S"])


# ---- the factor and the flags --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 6])
def test_f1_524588_components_the_factor_kernel_strides(ctxs, twins, N):
    """F1, the four-state scene on the four-state build and scene C's constant-turn model on the six-state build: components 524 288 ..
    524 587 are factored in trip 2 -- the second half of a straddling target, a scored target, a NaN and an indefinite one --, and two
    targets of more than 262 000 components take 1 024 trips a lane of mc_target_flags, the second with its indefinite P in trip 1 025."""
    sc = u.f1(N)
    want = twin_of("F1", lambda: ref.call_twin(twins["own"], sc))
    label = "F1 nComp 524588 T 7 S 4096, %d states, %d-state build" % (N, N)
    with seam_time(label, ctxs[N], "mht_mc_encounters"):
        rc, got = raw_own(ctxs[N], sc, guard=GUARD)
    assert rc == 0
    assert hold_own(label, got, want, sc) == 0
    u.check_f1(got)


@pytest.mark.parametrize("N", [4, 6])
def test_c1_targets_of_600_components_in_all_four_seams(ctxs, twins, N):
    """C1: a NaN at local component 300 (trip 2 of mc_target_flags), an indefinite P at 520 (trip 3) with nothing else wrong, both in one
    target -- 1 wins --, and a scored target whose count depends on the pick among 600 components, of which the ends have no weight"""
    sc = u.c1(N)
    S = sc["S"]
    partial = lambda a: bool(((a > 0) & (a < S)).any())
    zones, (doms, poses) = u.c1_zones(), u.c1_domains()
    want = dict(own=ref.call_twin(twins["own"], sc), pair=pref.call_twin(twins["pair"], sc, u.C1_PAIRS), zone=zref.call_twin(twins["zone"], sc, zones),
                domain=dref.call_twin(twins["domain"], sc, doms, poses))
    for lib_nx in (4, 6):
        ctx, label = ctxs[lib_nx], "C1 600 components, %d states, %d-state build" % (N, lib_nx)
        rc, got = raw_own(ctx, sc, guard=GUARD)
        assert rc == 0 and hold_own(label + ", own ship", got, want["own"], sc) == 0
        assert got["status"].tolist() == u.C1_STATUS and partial(got["ever"][:, u.C1_SCORED])
        rc, got = raw_pair(ctx, sc, u.C1_PAIRS, guard=GUARD)
        assert rc == 0 and hold_pair(label + ", pairs", got, want["pair"], sc, u.C1_PAIRS) == 0
        assert got["status"].tolist() == u.C1_PAIR_STATUS and partial(got["ever"][4:]) and got["ever"][4] == got["ever"][5]
        rc, got = raw_zone(ctx, sc, zones, guard=GUARD)
        assert rc == 0 and hold_zone(label + ", zones", got, want["zone"], sc, zones) == 0
        assert got["status"].tolist() == u.C1_STATUS and partial(got["ever"][:, u.C1_SCORED])
        rc, got, _ = raw_domain(ctx, sc, doms, poses, guard=GUARD)
        assert rc == 0 and hold_domain(label + ", domains", got, want["domain"], sc, doms, poses) == 0
        assert got["status"].tolist() == u.C1_STATUS and partial(got["ever"][:, :, u.C1_SCORED])


# ---- the particle limit --------------------------------------------------------------------------------------------------------------
def test_p1_a_million_particles(ctxs, twins):
    """P1, S = 1 048 576, the limit: the own ship with two targets is 512 chunks of 2 048 -- eight trips of a workgroup's slab loop, a
    fold over 512 chunks, a count of 2^20 --, one pair 1 024 chunks of 1 024"""
    sc = u.p1()
    assert ref.chunks(2, u.P1_S) == (512, 2048) and ref.chunks(1, u.P1_S) == (1024, 1024)
    want = twin_of("P1 own ship", lambda: ref.call_twin(twins["own"], sc))
    for lib_nx in (4, 6):
        label = "P1 S 1048576 T 2, %d-state build" % lib_nx
        with seam_time(label, ctxs[lib_nx], "mht_mc_encounters"):
            rc, got = raw_own(ctxs[lib_nx], sc, guard=GUARD)
        assert rc == 0
        assert hold_own(label, got, want, sc) == 0
        assert got["valid"].tolist() == [u.P1_S] * 2 and got["status"].tolist() == [0, 0] and (got["ever"][:, 0] == u.P1_S).all()
        assert ((got["ever"][:, 1] > 100000) & (got["ever"][:, 1] < 200000)).all()
    sc, pairs = u.p1_pair()
    want = twin_of("P1 pair", lambda: pref.call_twin(twins["pair"], sc, pairs))
    for lib_nx in (4, 6):
        label = "P1 S 1048576 one pair, %d-state build" % lib_nx
        with seam_time(label, ctxs[lib_nx], "mht_mc_pair_encounters"):
            rc, got = raw_pair(ctxs[lib_nx], sc, pairs, guard=GUARD)
        assert rc == 0
        assert hold_pair(label, got, want, sc, pairs) == 0
        assert got["valid"].tolist() == [u.P1_S] and (got["firstAt"].sum(axis=0, dtype=np.int64) == got["ever"]).all() and 0 < got["ever"][0] < u.P1_S
