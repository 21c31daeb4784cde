"""The scenes of tests/test_mc_strides_gpu.py and tests/test_mc_strides_cpu.py: the smallest calls of the four Monte-Carlo seams --
`mht_mc_encounters`, `mht_mc_pair_encounters`, `mht_mc_zone_encounters`, `mht_mc_domain_encounters` -- that put something worth reading
behind the first trip of the loops they share.  mc_factor_kernel and mc_fold_kernel launch at most MC_MAX_BLOCKS = 2048 workgroups of
256 lanes, 524 288 components or words a trip, and stride over the rest; mc_target_flags strides over a target's components by 256; a
walk workgroup strides over its slab by 256 particles.  The fold is indexed word-major with the item (a target, a pair) fastest, and
the items' status words follow: its second trip is the last words of every item.

    M1  own ship  G = 64, K = 64, T = 130, S = 64         549 250 fold words: `within` from 524 288 on, all of `ever`, valid, status
    M2  pairs     K = 64, 4 100 pairs of M1's targets     537 100: the last rows of `firstAt`, all of `ever`
    M3  zones     32 zones of 32 vertices, K = 64, T = 130   544 960: the end of `firstAt`, all of `ever`
    M4  domains   4 x 64 vertices, 16 paths, K = 64, T = 70  586 880: 62 592 words of `firstAt` and `ever`
    F1  own ship  nComp = 524 588, G = 2, K = 7, S = 4 096    the factor kernel's second trip (300 components); a target of 262 000
                  components: 1 024 trips a lane of mc_target_flags
    C1  all four  targets of 600 components, S = 1 024        the second and third trips of mc_target_flags, mc_pick over 600
    P1  own ship, pairs   S = 1 048 576                        512 chunks of 2 048 (eight trips of the slab loop); 1 024 chunks of 1 024

Every scene is made of mc_ref.scene_a() / scene_c() through mc_ref.scene: no state is drawn here but the offsets of F1's and C1's
components about entry 12 of scene A."""
import numpy as np

import mc_domain_ref as dref
import mc_pair_ref as pref
import mc_ref as ref
import mc_zone_ref as zref

TRIP = 2048 * 256                        # MC_MAX_BLOCKS * MC_THREADS, recomputed from the sources in tests/test_mc_strides_cpu.py
G_MAX, K_MAX = 64, 64
M_S = 64
M1_T, M2_PAIRS, M4_T = 130, 4100, 70
M2_LEAST = dict(within=500, firstAt=100, ever=500)
M3_SEED = ref.SEED + 1                   # (under mc_ref.SEED two targets have one count each behind TRIP, the same one)
F1_NCOMP = TRIP + 300
# F1's targets, [first, end): two of more than 260 000 components -- the second with an indefinite P in its last trip of
# mc_target_flags, trip 1 025 --, one that straddles component 524 288, one wholly behind it, one with a NaN component, one with an
# indefinite P, and a last good one
F1_FIRST = np.array([0, 262000, 524280, 524300, 524500, 524510, 524520, F1_NCOMP], dtype=np.int32)
F1_STRADDLES, F1_BEHIND, F1_NAN, F1_INDEFINITE = 2, 3, 4, 5
F1_NAN_AT, F1_INDEFINITE_AT, F1_DEEP_AT = 524505, 524517, 524275
F1_STATUS = [0, 2, 0, 0, 1, 2, 0]
F1_R = 12.0
C1_N, C1_S = 600, 1024
C1_NAN_AT, C1_INDEFINITE_AT = 300, 520      # local components: the second and the third trip of mc_target_flags
C1_SCORED = 3                            # the targets: 0 NaN, 1 indefinite, 2 both, 3 scored, 4 one good component (the pairs' partner)
C1_PAIRS = np.array([[0, 3], [3, 1], [2, 3], [1, 0], [3, 4], [4, 3]], dtype=np.int32)
C1_PAIR_STATUS = [1, 2, 1, 1, 0, 0]
P1_S = 1 << 20

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def candidates(G):
    """The G candidates of tests/test_mc_gpu.py's "G=64" kind"""
    return np.array([[0.02 * (g - G // 2), 1.0 - 0.005 * g, 2.0 * (g % 3)] for g in range(G)])


def fold_words(out, names):
    """The count words of a set of outputs in the fold's order: the arrays one after the other, each word-major with the item fastest"""
    return np.concatenate([out[k].reshape(-1) for k in names])


# ---- M1 .. M4: the fold --------------------------------------------------------------------------------------------------------------
def m1():
    """Own ship: 130 one-component targets (scene A's, cyclically), 64 own paths from entry 12 over 64 steps of 35 / 64 s"""
    def make():
        a = ref.scene_a()
        idx = np.arange(M1_T) % 70
        dt = 35.0 / K_MAX
        sc = ref.scene(a["x"][idx], a["P"][idx], np.arange(M1_T + 1), np.ones(M1_T), a["Phi"], a["Q"],
                       ref.own_paths(a["x"][12, :4], candidates(G_MAX), K_MAX, dt), S=M_S)
        return dref._with_step(sc, K_MAX, M_S)
    return _once("m1", make)


def m2():
    """(scene, pairs): the first 4 100 of all pairs of M1's targets"""
    return m1(), pref.all_pairs(M1_T)[:M2_PAIRS]


def m3():
    """(scene, zones): M1's targets against 32 zones of 32 vertices about the targets' median, every other one in reversed order"""
    def make():
        ctr = zref.centre_of(ref.scene_a())
        return [zref.reg(32, 120.0 + 15.0 * z, ctr + 60.0 * np.array([np.cos(z), np.sin(2.0 * z)]), 0.1 * z)[::1 - 2 * (z % 2)].copy() for z in range(32)]
    return dict(m1(), seed=M3_SEED), _once("m3 zones", make)


def m4():
    """(scene, domains, poses): scene A's 70 targets against 4 domains of 64 vertices on 16 own paths, 64 cells"""
    def make():
        a = ref.scene_a()
        sc = dref._with_step(dict(a, S=M_S), K_MAX, M_S)
        cand = np.array([(psi, f, 0.0) for psi in np.linspace(-1.2, 1.2, 8) for f in (0.6, 1.0)])
        doms = [zref.reg(64, 150.0 + 60.0 * i, (20.0, 80.0), 0.05 * i) for i in range(4)]
        return sc, doms, dref.poses_of(a["x"][0, :4].copy(), cand, K_MAX, sc["dt"])
    return _once("m4", make)


def check_fold_scene(label, out, names, items, S, least=500, distinct=True):
    """The conditions on M1 .. M4, on a set of counts.  In each output array that has words behind TRIP at least `least` = 500 of them
    are neither 0 nor S -- M2 passes 100 for firstAt and 500 for the case: what lies behind TRIP of a pair call's firstAt are steps 62
    to 64 alone, where few pairs meet for the first time (134 words at R = 80 m, never more than 474 at any radius from 80 m to
    1 500 m), and its `ever` carries the case.  And no two items have equal columns among the second trip's words -- of the items
    with a word strictly between 0 and S there: a target that never comes near, one that is not scored and one that is inside with
    every particle have columns of 0 and S alone, alike by nature, which a store into the wrong column shows as well as any other.
    At least 16 items must have such a column (a slip in a stride moves every column, and 16 distinct ones cannot all land on their
    like).  distinct False, M2: a pair's column behind TRIP is three words -- firstAt at steps 63 and 64, and ever -- and 744 pairs
    with a partial count cannot all differ in them; there at least 500 columns must differ from their right-hand neighbour's.
    Prints the figures and returns the number of non-zero words behind TRIP."""
    least = least if isinstance(least, dict) else {k: least for k in names}
    at, live, total = 0, 0, 0
    for k in names:
        flat = out[k].reshape(-1)
        behind = flat[min(max(TRIP - at, 0), len(flat)):]
        at += len(flat)
        if len(behind):
            partial = int(((behind > 0) & (behind < S)).sum())
            print("%s: %s has %d words behind %d, %d of them neither 0 nor S" % (label, k, len(behind), TRIP, partial))
            assert partial >= least[k], (label, k, partial)
            live, total = live + int((behind > 0).sum()), total + partial
    assert at > TRIP and total >= 500, (label, total)
    rows = fold_words(out, names)[-(-TRIP // items) * items:].reshape(-1, items)      # the whole words (rows of `items`) behind TRIP
    cols = [rows[:, j].tobytes() for j in range(items) if ((rows[:, j] > 0) & (rows[:, j] < S)).any()]
    print("%s: %d non-zero count words behind %d; %d of %d columns have a partial count" % (label, live, TRIP, len(cols), items))
    if distinct:
        assert len(rows) >= 64 and len(set(cols)) == len(cols) and len(cols) >= 16, (label, "two items have equal columns, or too few have any count")
    else:
        assert int((rows[:, 1:] != rows[:, :-1]).any(axis=0).sum()) >= 500, (label, "too few neighbouring columns differ")
    return live


# ---- F1: the factor kernel and mc_target_flags over a long range ---------------------------------------------------------------------
def f1(N=4):
    """Own ship, nComp = 524 588 in seven targets (F1_FIRST), every component entry 12 of scene A (N = 6: of scene C) moved by up to 25 m,
    under two own paths from entry 12's own state, R = 12 m: of the size of the components' position sigma.  Equal weights."""
    def make():
        base = ref.scene_a() if N == 4 else ref.scene_c()
        rng = np.random.default_rng(524588)
        n = F1_NCOMP
        x, P = np.tile(base["x"][12], (n, 1)), np.tile(base["P"][12], (n, 1, 1))
        x[:, :2] += rng.uniform(-25.0, 25.0, (n, 2))
        x[F1_NAN_AT, 1] = np.nan
        P[F1_INDEFINITE_AT, 0, 0] = -1.0
        P[F1_DEEP_AT, 1, 1] = -1.0
        return ref.scene(x, P, F1_FIRST, np.ones(n), base["Phi"], base["Q"], ref.own_paths(ref.scene_a()["x"][12, :4], ref.CANDIDATES, ref.K, ref.DT),
                         ct=base["ct"], R=F1_R, S=4096)
    return _once(("f1", N), make)


def check_f1(out, S=4096):
    assert out["status"].tolist() == F1_STATUS and out["valid"].tolist() == [0 if st else S for st in F1_STATUS]
    for t in (F1_STRADDLES, F1_BEHIND):
        assert ((out["ever"][:, t] > 0) & (out["ever"][:, t] < S)).all(), (t, out["ever"][:, t])
    idle = np.flatnonzero(F1_STATUS)
    assert not out["within"][:, :, idle].any() and not out["ever"][:, idle].any()


# ---- C1: targets of 600 components ---------------------------------------------------------------------------------------------------
def c1(N=4, far_weight=1.0):
    """Three targets of 600 components with a NaN at local 300, an indefinite P at local 520, and both; a scored target of 600 whose
    components lie alternately beside entry 12 and 20 km off, with zero weight at both ends; a fifth target of one good component.
    far_weight = 0: the same scene with the far components never picked."""
    def make():
        base = ref.scene_a() if N == 4 else ref.scene_c()
        rng = np.random.default_rng(600)
        n = 4 * C1_N + 1
        x, P = np.tile(base["x"][12], (n, 1)), np.tile(base["P"][12], (n, 1, 1))
        x[:, :2] += rng.uniform(-60.0, 60.0, (n, 2))
        w = rng.uniform(0.1, 1.0, n)
        x[C1_NAN_AT, 1] = np.nan
        P[C1_N + C1_INDEFINITE_AT, 0, 0] = -1.0
        x[2 * C1_N + C1_NAN_AT, 0] = np.nan
        P[2 * C1_N + C1_INDEFINITE_AT, 1, 1] = -1.0
        lo = C1_SCORED * C1_N
        far = lo + np.arange(1, C1_N, 2)
        x[far, :2] += [2e4, -2e4]
        w[far] *= far_weight
        w[[lo, lo + 1, lo + C1_N - 2, lo + C1_N - 1]] = 0.0
        x[n - 1, :2] = base["x"][12, :2] + [40.0, -30.0]
        first = np.append(np.arange(5) * C1_N, n)
        return ref.scene(x, P, first, w, base["Phi"], base["Q"], ref.own_paths(ref.scene_a()["x"][12, :4], ref.CANDIDATES, ref.K, ref.DT),
                         ct=base["ct"], S=C1_S)
    return _once(("c1", N, far_weight), make)


def c1_zones():
    return _once("c1 zones", lambda: [zref.reg(7, 90.0, ref.scene_a()["x"][12, :2] + [30.0, 10.0], 0.2), zref.reg(64, 200.0, ref.scene_a()["x"][12, :2], 0.1)[::-1].copy()])


def c1_domains():
    """(domains, poses): mc_domain_ref.DOMAINS on three own paths from a ship 150 m west and 60 m south of entry 12, with its velocity"""
    def make():
        a = ref.scene_a()
        own = np.concatenate([a["x"][12, :2] - (150.0, 60.0), a["x"][0, 2:4]])
        return dref.DOMAINS, dref.poses_of(own, dref.CANDIDATES[:3], ref.K, ref.DT)
    return _once("c1 domains", make)


C1_STATUS = [1, 2, 1, 0, 0]


# ---- P1: the particle limit ----------------------------------------------------------------------------------------------------------
def p1():
    """Own ship: entries 12 and 20 of scene A under two own paths from entry 12's state, S = 2^20"""
    def make():
        a = ref.scene_a()
        return ref.scene(a["x"][[12, 20]], a["P"][[12, 20]], [0, 1, 2], [1.0, 1.0], a["Phi"], a["Q"], ref.own_paths(a["x"][12, :4], ref.CANDIDATES, ref.K, ref.DT), S=P1_S)
    return _once("p1", make)


def p1_pair():
    """(scene, pairs): entries 62 and 27 of scene A, which come inside at every step and not with every particle, as the two targets of
    a scene at S = 2^20, and the pair (0, 1) -- T = 2, so that the NumPy reference, which keeps every target's paths, fits in 1 GB"""
    def make():
        a = ref.scene_a()
        return ref.scene(a["x"][[62, 27]], a["P"][[62, 27]], [0, 1, 2], [1.0, 1.0], a["Phi"], a["Q"], a["own"], S=P1_S)
    return _once("p1 pair", make), np.array([[0, 1]], dtype=np.int32)
