"""CPU: the encounter figures (csrc/mht_encounter.h: encounter_propagate / encounter_cell, what a lane of the kernels of
mht_encounter.hip runs per entry and per cell) compiled for the host and held to the criterion of tests/test_encounter_gpu.py; the
rule of pc against the exact probability; the properties of the figures; and the refusals that need no GPU.

Criterion, the project's: per output family e = max |got - truth| / (1 + |truth|) over the cells that are not NaN in the truth,
e <= 8 max(e_np, eps64), truth the reference's np.longdouble evaluation (pc: mpmath at 30 digits, the same 64 nodes) and e_np its
float64 evaluation's error; the NaN cells and the exact zeros of pc are the truth's exactly.  tpc is an arg max: encounter_ref.hold_tpc
says what it is held to where steps tie.  The measured figures are in the docstrings of the tests."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import mpmath as mp
import numpy as np
import pytest

import encounter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 8.0
SENTINEL = -7.03125e10      # (a value no case here produces)
N_ENTRIES = 70
RADIUS = 80.0
RULE_BOUND = 1e-6      # what the rule is documented to be good to: 4 x the 2.4e-7 the float64 reference measures against ncx2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    so = str(tmp_path_factory.mktemp("encounter_host") / "libencounter_host.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "encounter_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.encounters_host.restype = C.c_int
    lib.encounters_host.argtypes = [C.c_int32] * 4 + [C.c_double] * 2 + [C.c_void_p] * 6
    lib.encounter_pc_host.restype = None
    lib.encounter_pc_host.argtypes = [C.c_int32] + [C.c_void_p] * 4
    lib.encounter_rule_host.restype = None
    lib.encounter_rule_host.argtypes = [C.c_void_p] * 2
    return lib


def host_encounters(lib, x, P, Phi, Q, K, dt, R, first=None):
    """The twin on x [n, N], P [n, N, N]: (encounter_ref's dict, pos [K + 1, 2, n], S [K + 1, 3, n]); every cell is written."""
    n, N = x.shape
    first = n if first is None else first
    xp, Pp = ref.pack(x, P)
    Phi, Q = np.ascontiguousarray(Phi, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    out, work = np.full((5, first, n), SENTINEL), np.full(5 * (K + 1) * n, SENTINEL)
    assert lib.encounters_host(N, n, first, K, dt, R, Phi.ctypes.data, Q.ctypes.data, xp.ctypes.data, Pp.ctypes.data, out.ctypes.data, work.ctypes.data) == 0
    assert not (out == SENTINEL).any() and not (work == SENTINEL).any()
    return ref.seam_dict(out), work[:2 * (K + 1) * n].reshape(K + 1, 2, n), work[2 * (K + 1) * n:].reshape(K + 1, 3, n)


def host_pc(lib, dx, dy, a, b, c, R):
    dx, dy, a, b, c, R = [np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(dx, dy, a, b, c, R)]
    d, S, R = np.ascontiguousarray(np.stack([dx, dy], axis=-1)), np.ascontiguousarray(np.stack([a, b, c], axis=-1)), np.ascontiguousarray(R)
    pc = np.full(dx.shape, SENTINEL)
    lib.encounter_pc_host(dx.size, d.ctypes.data, S.ctypes.data, R.ctypes.data, pc.ctypes.data)
    return pc


_pc_case = {}


def pc_case(N):
    """The case pc and tpc are held to mpmath on, shared with tests/test_encounter_gpu.py and computed once: encounter_ref.make_batch of
    models/pv (N = 4) or models/ca (N = 6), 70 entries, first = 4, K = 4, dt = 5, R = 80 -- 270 pairs, about a fifth of them with a pc
    that is not 0 by the rule.  Returns (x, P, Phi, Q, K, dt, truth, f64, e_np of pc)."""
    if N not in _pc_case:
        from pymht_amd.models import ca, pv
        model = pv if N == 4 else ca
        K, dt = 4, 5.0
        x, P = ref.make_batch(model, N_ENTRIES, seed=3)
        Phi, Q = ref.model_matrices(model, dt)
        truth, f64 = ref.encounters(x, P, Phi, Q, K, dt, RADIUS, first=4, truth=True), ref.encounters(x, P, Phi, Q, K, dt, RADIUS, first=4)
        e_np = ref.ratios([f64], [truth], [f64], ("pc",))["pc"][1]
        _pc_case[N] = (x, P, Phi, Q, K, dt, truth, f64, e_np)
    return _pc_case[N]


def hold(label, got, truth, f64, dt, names=ref.NAMES, pc_scale=None):
    """The criterion on one evaluation.  pc_scale None: pc and tpc against a truth that carries mpmath's pc.  Else the truth's pc is the
    float64 reference's, and pc is held to it with e_np = pc_scale, the float64 reference's own error on pc_case."""
    eps = float(np.finfo(np.float64).eps)
    res = ref.ratios([got], [truth], [f64], [k for k in names if k != "tpc"])
    if pc_scale is not None and "pc" in res:
        e = res["pc"][0]
        res["pc"] = (e, pc_scale, e / max(pc_scale, eps))
    print(label + ": " + " | ".join("%s e %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert ref.same_nan([got], [truth], names), "the NaN cells are not the truth's"
    for k, (e, e_np, ratio) in res.items():
        assert np.isfinite(e) and ratio <= FACTOR, (k, e, e_np, ratio)
    if "pc" in names:
        zero = truth["pc"] == 0      # (by the rule in mpmath's truth; the float64 stand-in's zeros may also be products that underflow)
        assert (got["pc"][zero] <= (0 if pc_scale is None else 1e-290)).all(), "a pc that is 0 by the rule is not 0"
        assert (truth["pc"][(got["pc"] == 0) & ~zero] < 1e-290).all(), "a pc that is not 0 by the rule is 0"
        cells = ref.hold_tpc(got, truth, dt, FACTOR, res["pc"][1])
        print(label + ": tpc held in %d cells, %d of them with pc > 0" % (cells, int(np.sum(truth["pc"] > 0))))
    return res


def test_rule_table_is_the_gauss_legendre_rule_to_20_digits(lib):
    """The table of csrc/mht_encounter.h, read from its text, against nodes computed here to 38 digits: 32 symmetric pairs, ascending,
    every figure within 5e-20 relative; and the doubles the compiler makes of them are the nearest ones."""
    text = open(os.path.join(ROOT, "pymht_amd", "csrc", "mht_encounter.h")).read()
    xs, ws = ref.gauss_legendre(64)
    with mp.workdps(40):
        for name, want in (("x", xs), ("w", ws)):
            body = re.search(r"static constexpr double %s\[32\] = \{(.*?)\};" % name, text, re.S).group(1)
            got = [mp.mpf(v) for v in re.findall(r"[0-9.]+", body)]
            assert len(got) == 32 and all(abs(g - w) <= mp.mpf("5e-20") * w for g, w in zip(got, want)), name
        assert abs(2 * sum(ws) - 2) < mp.mpf("1e-36")
    x, w = np.zeros(32), np.zeros(32)
    lib.encounter_rule_host(x.ctypes.data, w.ctypes.data)
    assert np.array_equal(x, [float(v) for v in xs]) and np.array_equal(w, [float(v) for v in ws]) and (np.diff(x) > 0).all()


@pytest.mark.parametrize("N", [4, 6])
def test_pc_and_tpc_on_the_host_against_mpmath(lib, N):
    """pc_case(N): every figure of the twin against the truth, pc's from mpmath.  Measured, host build (g++ -O2 -mfma), ratios
    e / max(e_np, eps64) for tcpa / dcpa / md2 / pc:
        N 4   1 / 1 / 1 / 1   (e_np 1.1e-13 / 1.6e-15 / 1.7e-15 / 6.1e-16), 260 of the 262 pairs with pc > 0
        N 6   1 / 1 / 1 / 1   (e_np 5.7e-13 / 2.6e-15 / 6.1e-16 / 1.0e-15), 262 of 262
    -- the twin and the float64 reference do the same operations in the same order, and their largest errors are the same cells'."""
    assert np.finfo(np.longdouble).eps < 1e-18
    x, P, Phi, Q, K, dt, truth, f64, e_np = pc_case(N)
    got, _, _ = host_encounters(lib, x, P, Phi, Q, K, dt, RADIUS, first=4)
    hold("host build, pc case N %d" % N, got, truth, f64, dt)
    assert int(np.sum(truth["pc"] > 0)) >= 30 and int(np.sum((truth["pc"] > 1e-3) & (truth["pc"] < 0.999))) >= 8
    hold("float64 reference, pc case N %d" % N, f64, truth, f64, dt)


@pytest.mark.parametrize("N,K", [(4, 1), (4, 7), (6, 1), (6, 7)])
def test_encounters_on_the_host_meet_the_accuracy_criterion(lib, N, K):
    """encounter_ref.make_batch, 70 entries, all 2415 pairs, dt = 5, R = 80: tcpa, dcpa and md2 against the np.longdouble truth; pc
    against the float64 reference with e_np from pc_case; the propagated positions and covariances against the longdouble ones under
    the same criterion; the special pairs as the reference has them; rows of a first = 3 call are those of the full call bit for bit.
    Measured, host build, ratios for tcpa / dcpa / md2 / pc / pos / S:
        N 4 K 1   1 / 1 / 1 / 1.01 / 1 / 0.89       N 4 K 7   1 / 1 / 1 / 1.01 / 1 / 1
        N 6 K 1   1 / 1 / 1 / 0.997 / 1 / 0.85      N 6 K 7   1 / 1 / 1 / 0.997 / 1 / 1
    with e_np 4.6e-13 / 7.8e-14 / 1.7e-15 / 6.1e-16 at N 4 K 7.  At K = 1 two thirds of the pairs have a pc that is 0 by the rule (763 and
    940 of 2277 are not), at K = 7 none."""
    from pymht_amd.models import ca, pv
    model = pv if N == 4 else ca
    dt = 5.0
    x, P = ref.make_batch(model, N_ENTRIES, seed=3)
    Phi, Q = ref.model_matrices(model, dt)
    got, pos, S = host_encounters(lib, x, P, Phi, Q, K, dt, RADIUS)
    truth, f64 = ref.encounters(x, P, Phi, Q, K, dt, RADIUS, truth=True, pc_mp=False), ref.encounters(x, P, Phi, Q, K, dt, RADIUS)
    hold("host build, N %d K %d" % (N, K), got, truth, f64, dt, pc_scale=pc_case(N)[8])
    for ev in (got, truth, f64):
        ref.check_special_cells(ev, K, dt)
    want, mine = ref.propagate(x, P, Phi, Q, K, np.longdouble), ref.propagate(x, P, Phi, Q, K)
    prop = lambda p, s: dict(pos=np.asarray(p), S=np.asarray(s))
    res = ref.ratios([prop(np.moveaxis(pos, 1, 2), np.moveaxis(S, 1, 2))], [prop(*want)], [prop(*mine)], ("pos", "S"))
    print("propagation N %d K %d: " % (N, K) + " | ".join("%s e %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert all(np.isfinite(e) and ratio <= FACTOR for e, _, ratio in res.values())
    for e in (ref.NAN_X, ref.NAN_P):
        assert np.isnan(pos[:, :, e]).all() and np.isnan(S[:, :, e]).all()
    assert np.isfinite(np.delete(pos, [ref.NAN_X, ref.NAN_P], axis=2)).all()
    for first in (3, 1):
        part, _, _ = host_encounters(lib, x, P, Phi, Q, K, dt, RADIUS, first=first)
        assert all(np.array_equal(part[k], got[k][:first], equal_nan=True) for k in ref.NAMES)


def test_cpa_of_a_constant_velocity_pair_is_the_closed_form_bit_for_bit(lib):
    """models/pv's Phi with Q = 0: the piecewise-linear CPA is the CPA, t* = clamp(-d . v / |v|^2, 0, T) and |d + t* v|.  On cases whose
    arithmetic is exact in float64 -- integer positions, relative velocities with |v|^2 a power of two, dt = 2 and 0.5 -- the twin
    gives the closed form's bits: CPAs inside the horizon, on a joint of two segments, beyond the horizon, at t = 0, and a pair
    without relative motion (t* = 0)."""
    rel_v = [(4, 0), (0, -2), (4, 4), (-1, 1), (8, -8), (0, 0), (-16, 0)]
    rel_d = [(-37, 5), (3, 40), (-100, -60), (7, -9), (-50, 90), (12, 5), (1000, 3), (0, 0), (-4, -4)]
    x = [np.array([11.0, -9.0, 3.0, -5.0])]
    for v in rel_v:
        for d in rel_d:
            x.append(x[0] - np.array([d[0], d[1], v[0], v[1]], dtype=np.float64))      # (d = x_0 - x_j, v likewise)
    x = np.array(x)
    n = len(x)
    P = np.tile(np.eye(4), (n, 1, 1))
    from pymht_amd.models import pv
    inside = 0
    for K, dt in ((8, 2.0), (24, 0.5), (1, 2.0)):
        Phi = ref.model_matrices(pv, dt)[0]
        got, _, _ = host_encounters(lib, x, P, Phi, np.zeros((4, 4)), K, dt, 10.0, first=1)
        T = K * dt
        j = 1
        for v in rel_v:
            for d in rel_d:
                vv = float(v[0] * v[0] + v[1] * v[1])
                t = min(max(-(d[0] * v[0] + d[1] * v[1]) / vv, 0.0), T) if vv > 0 else 0.0
                dist = np.sqrt((d[0] + t * v[0]) ** 2 + (d[1] + t * v[1]) ** 2)
                assert got["tcpa"][0, j] == t and got["dcpa"][0, j] == dist, (K, dt, v, d, got["tcpa"][0, j], t, got["dcpa"][0, j], dist)
                inside += 0 < t < T
                j += 1
    assert inside > 30


def test_the_rule_against_the_exact_probability():
    """The float64 reference of the rule against scipy's ncx2 (exact for an isotropic Sigma) on encounter_ref.isotropic_grid: 800
    fixed-seed cases, R over 1 .. 1000, s / R over 10^-2.5 .. 10^1.5, the offset up to R + 6 s.  The bound is 1e-6, four times the
    2.4e-7 the rule was measured at when it was chosen; measured here: worst |error| 2.29e-07 (at s / R = 0.0064, the offset 1.00 R).
    The reference sets this scale, not the code under test.  ncx2 itself is held to the rule at 400 nodes and a clip of 12 in
    mpmath on a subsample (worst difference 2.2e-16)."""
    dx, dy, s, R = ref.isotropic_grid()
    got = ref.pc_rule(dx, dy, s * s, 0.0, s * s, R)
    exact = ref.pc_exact_isotropic(np.hypot(dx, dy), s, R)
    err = np.abs(got - exact)
    w = int(np.argmax(err))
    print("rule against ncx2: worst |error| %.3g at s / R %.3g, offset / R %.3g" % (err[w], s[w] / R[w], np.hypot(dx[w], dy[w]) / R[w]))
    assert err.max() <= RULE_BOUND
    sub = np.arange(0, len(R), 40)
    fine = np.array([float(ref.pc_rule_mp(*[mp.mpf(float(v)) for v in (dx[i], dy[i], s[i] ** 2, 0.0, s[i] ** 2, R[i])], nodes=400, clip=12)) for i in sub])
    print("ncx2 against the rule at 400 nodes, clip 12: worst difference %.3g" % np.abs(fine - exact[sub]).max())
    assert np.abs(fine - exact[sub]).max() < 1e-11


def test_the_twin_follows_the_rule_where_the_rule_was_measured(lib):
    """The twin's encounter_pc on the isotropic grid and on an anisotropic one (s2 / s1 log-uniform over 1 .. 100, any orientation)
    against the float64 reference of the rule: the same operations, so the difference is that of exp, erfc and the trigonometric
    functions of two libraries -- measured 6.3e-15 and 9.8e-15 -- and is held to 8 x 64 eps64, the rule's 64 terms.  Hence the twin
    meets the 1e-6 against the exact probability as the reference does."""
    dx, dy, s, R = ref.isotropic_grid()
    rng = np.random.default_rng(12)
    ratio, phi = 10.0 ** rng.uniform(0, 2, len(R)), rng.uniform(0, np.pi, len(R))
    l1, l2 = s * s, s * s * ratio * ratio
    a = l1 * np.sin(phi) ** 2 + l2 * np.cos(phi) ** 2
    c = l1 * np.cos(phi) ** 2 + l2 * np.sin(phi) ** 2
    b = (l2 - l1) * np.sin(phi) * np.cos(phi)
    bound = FACTOR * 64 * float(np.finfo(np.float64).eps)
    for label, args in (("isotropic", (dx, dy, s * s, 0.0 * s, s * s, R)), ("anisotropic", (dx * ratio, dy * ratio, a, b, c, R))):
        got, want = host_pc(lib, *args), ref.pc_rule(*args)
        print("twin against the float64 rule, %s: worst difference %.3g, %d cases not 0" % (label, np.abs(got - want).max(), int(np.sum(want > 0))))
        assert np.array_equal(got == 0, want == 0) and np.abs(got - want).max() <= bound and int(np.sum(want > 1e-3)) > 100
    assert np.abs(host_pc(lib, dx, dy, s * s, 0.0 * s, s * s, R) - ref.pc_exact_isotropic(np.hypot(dx, dy), s, R)).max() <= RULE_BOUND


def test_properties_of_pc(lib):
    """pc is non-decreasing in R (to the 1e-6 the rule is good to: the exact probability is monotone, the rule follows it that
    closely), pc -> 1 for R >> |d| + 8 s2 (held to the same 1e-6; measured 6.2e-15), and every figure is the same bits under a swap
    of the pair's two entries."""
    rng = np.random.default_rng(4)
    m = 300
    s1, ratio, phi = 10.0 ** rng.uniform(0, 1.5, m), 10.0 ** rng.uniform(0, 1.5, m), rng.uniform(0, np.pi, m)
    l1, l2 = s1 * s1, s1 * s1 * ratio * ratio
    a = l1 * np.sin(phi) ** 2 + l2 * np.cos(phi) ** 2
    c = l1 * np.cos(phi) ** 2 + l2 * np.sin(phi) ** 2
    b = (l2 - l1) * np.sin(phi) * np.cos(phi)
    dx, dy = rng.normal(size=m) * 3 * s1 * ratio, rng.normal(size=m) * 3 * s1 * ratio
    radii = s1[None, :] * np.geomspace(0.05, 400, 40)[:, None]
    pcs = np.array([host_pc(lib, dx, dy, a, b, c, R) for R in radii])
    assert (pcs >= 0).all() and (pcs <= 1 + RULE_BOUND).all() and (np.diff(pcs, axis=0) >= -RULE_BOUND).all()
    assert (pcs[0] < 0.5).all() and int(np.sum((pcs > 0.01) & (pcs < 0.99))) > 500
    big = 10.0 * (np.hypot(dx, dy) + 8 * s1 * ratio)
    one = host_pc(lib, dx, dy, a, b, c, big)
    print("pc at R = 10 (|d| + 8 s2): worst |pc - 1| %.3g" % np.abs(one - 1).max())
    assert np.abs(one - 1).max() <= RULE_BOUND
    from pymht_amd.models import ca
    x, P = ref.make_batch(ca, N_ENTRIES, seed=3)
    Phi, Q = ref.model_matrices(ca, 5.0)
    full, _, _ = host_encounters(lib, x, P, Phi, Q, 5, 5.0, RADIUS)
    order = np.arange(N_ENTRIES)[::-1]
    back, _, _ = host_encounters(lib, x[order], P[order], Phi, Q, 5, 5.0, RADIUS)
    for k in ref.NAMES:      # entry e sits at n - 1 - e: cell (i, j) of the one call is cell (n - 1 - j, n - 1 - i) of the other
        assert np.array_equal(back[k], full[k][::-1, ::-1].T, equal_nan=True), k
    assert int(np.sum(full["pc"] > 0)) > 100


def test_refusals_that_need_no_gpu_and_what_the_docstrings_say(lib):
    from pymht_amd import evaluation
    from pymht_amd.models import ca, ct, pv
    from pymht_amd.tracker import Tracker
    a = np.zeros(256)
    p = a.ctypes.data
    for nx, n, first, K, dt, R in ((5, 2, 2, 3, 1.0, 1.0), (4, 2, 2, 0, 1.0, 1.0), (4, 2, 2, 65, 1.0, 1.0), (4, 2, 2, 3, 0.0, 1.0), (4, 2, 2, 3, 1.0, 0.0),
                                   (6, 2, 2, 3, -1.0, 1.0), (6, 2, 2, 3, 1.0, float("nan")), (4, 2, 3, 3, 1.0, 1.0), (4, 2, -1, 3, 1.0, 1.0), (4, -1, 0, 3, 1.0, 1.0)):
        assert lib.encounters_host(nx, n, first, K, dt, R, p, p, p, p, p, p) == -1
    assert (a == 0).all()
    x, P = np.zeros((3, 4)), np.tile(np.eye(4), (3, 1, 1))
    Phi, Q = ref.model_matrices(pv, 2.5)
    for bad in (dict(x=np.zeros((3, 5))), dict(x=np.zeros(4)), dict(P=np.zeros((3, 4, 3))), dict(P=np.zeros((2, 4, 4))), dict(Phi=np.eye(6)), dict(Q=np.eye(3)),
                dict(steps=0), dict(steps=65), dict(steps=2.5), dict(steps=True), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(radius=0.0),
                dict(radius=float("inf")), dict(first=4), dict(first=-1), dict(first=1.5), dict(Phi=np.full((4, 4), np.nan))):
        kw = dict(x=x, P=P, Phi=Phi, Q=Q, steps=4, dt=2.5, radius=50.0)
        kw.update(bad)
        with pytest.raises(ValueError, match="encounters"):
            evaluation.encounters(**kw)
    # fewer than two entries, or no rows: empty arrays, no device
    for xs, first, shape in ((x[:1], None, (1, 1)), (x[:0], None, (0, 0)), (x, 0, (0, 3))):
        out = evaluation.encounters(xs, P[:len(xs)], Phi, Q, 4, 2.5, 50.0, first=first)
        assert sorted(out) == sorted(ref.NAMES) and all(v.shape == shape and np.isnan(v).all() for v in out.values())
    with pytest.raises(NotImplementedError, match="ct"):
        evaluation.encounter_model(ct, 2.5)
    nx, A, W = evaluation.encounter_model(ca, 7.0)
    assert nx == 6 and A.dtype == np.float64 and np.array_equal(A, ref.model_matrices(ca, 7.0)[0]) and np.array_equal(W, ref.model_matrices(ca, 7.0)[1])
    sig = inspect.signature(Tracker.getEncounters).parameters
    assert list(sig) == ["self", "horizon", "radius", "ownShip", "ownCovariance", "steps"] and all(sig[k].default is None for k in ("ownShip", "ownCovariance", "steps"))
    assert "encounter_model" in inspect.getsource(Tracker.getEncounters)
    doc = " ".join(Tracker.getEncounters.__doc__.split())
    assert "AIS-aided filter's state is NOT used" in doc and "NotImplementedError" in doc and "1e-6" in doc and "independent" in doc
    doc = " ".join(evaluation.encounters.__doc__.split())
    assert "1e-6" in doc and "not exact" in doc and "cross-correlation" in doc
