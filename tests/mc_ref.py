"""NumPy restatement of what `mht_mc_encounters` computes (include/mht_amd.h, csrc/mht_mc.h), vectorised over the particles of a target:
Philox4x32-10, the uniforms and Box-Muller normals, the Cholesky factor with the zero-pivot rule, the pick of a component, the walk
(linear and constant turn), and the counts within[G, K + 1, T] and ever[G, T] against the own ship's paths -- every sum in the order
the header writes it, so that only log, sin and cos differ from a host build of the header.  Shared by tests/test_mc_cpu.py (the host
twin tests/hostmath/mc_host.cpp against this file) and tests/test_mc_gpu.py (the seam against the twin).

THE BORDERLINE RULE, which every comparison of counts uses (hold_counts).  The reference marks a (particle, step) borderline where
| |d_k| - R | < 1e-9 R, and a particle borderline for `ever` where the smallest distance of its whole piecewise-linear path is that
close to R.  The libm of the host, NumPy's and the device's sin, cos and log differ in the last bits, and only such a particle can
legitimately land on the other side: a count may differ from the reference's by at most the number of borderline particles in its cell.
Their share is capped at 1e-6 of all (particle, step) pairs -- a condition on the inputs; the scenes here were chosen to have NONE, so
the counts are expected to be equal and the rule only makes a last-bit difference read as what it is."""
import os

import numpy as np

import encounter_ref as eref
import trial_ref as tref

EPS = float(np.finfo(np.float64).eps)
P_TOL, Q_TOL = 64.0 * EPS, 2.0 ** -20
PICK_STEP = 0xFFFFFFFF
MAX_PATHS, MAX_STEPS, MAX_PARTICLES, WARP, THREADS, FILL = 64, 64, 1 << 20, 64, 256, 1024
BORDER = 1e-9
BORDER_SHARE = 1e-6
SENTINEL = 0xDEADBEEF
M32 = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10: the counter words (arrays or ints) and the key -> four uint32 arrays"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
    return [v.astype(np.uint32) for v in c]


def uniform(r):
    return (np.asarray(r).astype(np.float64) + 0.5) * 2.0 ** -32


def box_muller(r0, r1):
    rad, ang = np.sqrt(-2.0 * np.log(uniform(r0))), 6.283185307179586 * uniform(r1)
    return rad * np.cos(ang), rad * np.sin(ang)


def normals(N, particle, step, target, seed):
    """z [N, len(particle)] of (particle, step, target) under the seed"""
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    a = philox(particle, step, target, 0, k0, k1)
    z = list(box_muller(a[0], a[1])) + list(box_muller(a[2], a[3]))
    if N == 6:
        b = philox(particle, step, target, 1, k0, k1)
        z += list(box_muller(b[0], b[1]))
    return np.array(z)


def pick_uniform(particle, target, seed):
    return uniform(philox(particle, PICK_STEP, target, 0, seed & 0xFFFFFFFF, seed >> 32)[0])


def factor(A, own=False):
    """(L [N, N] lower, status) of a symmetric matrix whose upper triangle is read, by the header's rule: own=False a component's P
    (tol = 64 eps max_i A_ii), own=True Q (tol_j = 2^-20 |A_jj|)"""
    A = np.asarray(A, dtype=np.float64)
    N = len(A)
    top = A[0, 0]
    for i in range(1, N):
        top = np.fmax(top, A[i, i])
    L, status = np.zeros((N, N)), 0
    for j in range(N):
        tol = Q_TOL * abs(A[j, j]) if own else P_TOL * top
        d = A[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        live = d > tol
        if not live and not d >= -tol:
            status = 2
        root = np.sqrt(d) if live else 1.0
        L[j, j] = root if live else 0.0
        for i in range(j + 1, N):
            a = A[j, i]
            for k in range(j):
                a = a - L[i, k] * L[j, k]
            L[i, j] = a / root if live else 0.0
    return L, status


def chunks(T, S):
    """(chunks, slab) of the header's mc_chunks"""
    most, fill = (S + THREADS - 1) // THREADS, (FILL + T - 1) // T
    want = min(most, fill)
    slab = ((S + want - 1) // want + THREADS - 1) // THREADS * THREADS
    return (S + slab - 1) // slab, slab


def ct_entries(dt, w):
    s, c = np.sin(w * dt), np.cos(w * dt)
    small = np.abs(w) < 1e-9
    with np.errstate(all="ignore"):
        sw, cw = np.where(small, dt, s / np.where(small, 1.0, w)), np.where(small, 0.0, (1.0 - c) / np.where(small, 1.0, w))
    return sw, cw, c, s


def step(X, z, Phi, F, dt, ct):
    """One step of the walk on X [N, S]"""
    N = len(X)
    if ct:
        sw, cw, c, s = ct_entries(dt, X[4])
        Y = [(X[0] + sw * X[2]) + (-cw) * X[3], (X[1] + cw * X[2]) + sw * X[3], c * X[2] + (-s) * X[3], s * X[2] + c * X[3], X[4] + dt * X[5], X[5]]
    else:
        Y = []
        for i in range(N):
            acc = Phi[i, 0] * X[0]
            for l in range(1, N):
                acc = acc + Phi[i, l] * X[l]
            Y.append(acc)
    out = []
    for i in range(N):
        acc = Y[i]
        for j in range(i + 1):
            acc = acc + F[i, j] * z[j]
        out.append(acc)
    return np.array(out)


def segment_min2(px, py, dx, dy):
    ex, ey = dx - px, dy - py
    ee = ex * ex + ey * ey
    with np.errstate(all="ignore"):
        sp = np.where(ee > 0.0, np.fmin(np.fmax(-(px * ex + py * ey) / np.where(ee > 0.0, ee, 1.0), 0.0), 1.0), 0.0)
    cx, cy = px + sp * ex, py + sp * ey
    return cx * cx + cy * cy


def component_status(x, P, cdf):
    """Per component: 1 for a NaN in x, the upper triangle of P or cdf, else the factor's status; and the factors [nComp, N, N]"""
    n, N = x.shape
    iu = np.triu_indices(N)
    st, Ls = np.zeros(n, dtype=np.int32), np.zeros((n, N, N))
    for c in range(n):
        with np.errstate(all="ignore"):
            Ls[c], f = factor(P[c])
        st[c] = 1 if (np.isnan(x[c]).any() or np.isnan(P[c][iu]).any() or np.isnan(cdf[c])) else f
    return st, Ls


def pick(cdf, lo, hi, u):
    """The header's binary search, per particle"""
    lo, hi = np.full(len(u), lo), np.full(len(u), hi)
    while (lo < hi).any():
        mid = lo + (hi - lo) // 2
        go = lo < hi
        left = go & (u < cdf[mid])
        hi = np.where(left, mid, hi)
        lo = np.where(go & ~left, mid + 1, lo)
    return lo


def encounters(x, P, first, cdf, Phi, Q, own, K, dt, R, S, seed, ct=False, keep_paths=False):
    """x [nComp, N], P [nComp, N, N], first [T + 1], cdf [nComp], own [G, K + 1, 2]: dict of within [G, K + 1, T], ever [G, T], valid,
    status [T] (uint32, int32 as the seam's), borderWithin, borderEver (the borderline particles per cell) and pairs (particle-steps
    walked)."""
    x, P, cdf, own = [np.asarray(v, dtype=np.float64) for v in (x, P, cdf, own)]
    N, T, G = x.shape[1], len(first) - 1, len(own)
    F, fq = factor(Q, own=True)
    assert fq == 0, "Q is not positive semidefinite"
    Phi = None if ct else np.asarray(Phi, dtype=np.float64)
    cst, Ls = component_status(x, P, cdf)
    within, ever = np.zeros((G, K + 1, T), dtype=np.uint32), np.zeros((G, T), dtype=np.uint32)
    bw, be = np.zeros((G, K + 1, T), dtype=np.int64), np.zeros((G, T), dtype=np.int64)
    valid, status = np.zeros(T, dtype=np.uint32), np.zeros(T, dtype=np.int32)
    R2, pairs, paths = R * R, 0, {}
    part = np.arange(S, dtype=np.uint64)
    for t in range(T):
        cs = cst[first[t]:first[t + 1]]
        status[t] = 1 if (cs == 1).any() else (2 if (cs == 2).any() else 0)
        if status[t]:
            continue
        valid[t] = S
        comp = pick(cdf, int(first[t]), int(first[t + 1]) - 1, pick_uniform(part, t, seed))
        z = normals(N, part, 0, t, seed)
        X = []
        for i in range(N):
            acc = Ls[comp, i, 0] * z[0]
            for j in range(1, i + 1):
                acc = acc + Ls[comp, i, j] * z[j]
            X.append(x[comp, i] + acc)
        X = np.array(X)
        came, low2 = np.zeros((G, S), dtype=bool), np.full((G, S), np.inf)
        prev = None
        track = [X[:2].copy()]
        for k in range(K + 1):
            if k:
                X = step(X, normals(N, part, k, t, seed), Phi, F, dt, ct)
                track.append(X[:2].copy())
            for g in range(G):
                dx, dy = X[0] - own[g, k, 0], X[1] - own[g, k, 1]
                d2 = dx * dx + dy * dy
                inside = d2 < R2
                within[g, k, t] = inside.sum()
                bw[g, k, t] = (np.abs(np.sqrt(d2) - R) < BORDER * R).sum()
                m2 = d2
                if k:
                    m2 = np.minimum(d2, segment_min2(prev[0] - own[g, k - 1, 0], prev[1] - own[g, k - 1, 1], dx, dy))
                came[g] |= m2 < R2
                low2[g] = np.minimum(low2[g], m2)
            prev = (X[0], X[1])
            pairs += S
        ever[:, t] = came.sum(axis=1)
        be[:, t] = (np.abs(np.sqrt(low2) - R) < BORDER * R).sum(axis=1)
        if keep_paths:
            paths[t] = (comp, np.array(track))
    out = dict(within=within, ever=ever, valid=valid, status=status, borderWithin=bw, borderEver=be, pairs=pairs)
    if keep_paths:
        out["paths"] = paths
    return out


def hold_counts(label, got, ref):
    """The borderline rule.  Returns the number of cells that differ (expected 0 on the scenes here)."""
    assert ref["borderWithin"].sum() <= BORDER_SHARE * max(ref["pairs"], 1), (label, "the scene has too many borderline pairs", int(ref["borderWithin"].sum()))
    dw = np.abs(got["within"].astype(np.int64) - ref["within"].astype(np.int64))
    de = np.abs(got["ever"].astype(np.int64) - ref["ever"].astype(np.int64))
    assert (dw <= ref["borderWithin"]).all(), (label, "within", np.argwhere(dw > ref["borderWithin"])[:5])
    assert (de <= ref["borderEver"]).all(), (label, "ever", np.argwhere(de > ref["borderEver"])[:5])
    assert (got["valid"] == ref["valid"]).all() and (got["status"] == ref["status"]).all(), label
    return int((dw > 0).sum() + (de > 0).sum())


def same_counts(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and (a[k] == b[k]).all() for k in ("within", "ever", "valid", "status"))


# ---- the scenes --------------------------------------------------------------------------------------------------------------------
DT, K, R, S, SEED = 5.0, 7, 80.0, 4096, 12345
CANDIDATES = np.array([[0.0, 1.0, 0.0], [tref.DEG40, 1.0, 10.0]])


def own_paths(own, cand, K, dt, w=tref.TURN_RATE):
    """[G, K + 1, 2]: trial_ref.candidate_path's positions"""
    return np.ascontiguousarray(tref.candidate_path(own, np.zeros(3), w, cand, K, dt)[0].transpose(1, 0, 2))


def scene(x, P, first, weight, Phi, Q, own, ct=False, K=K, dt=DT, R=R, S=S, seed=SEED):
    """The arguments of one call as a dict; cdf from the weights as evaluation.mc_encounters builds it"""
    first = np.asarray(first, dtype=np.int32)
    cdf = np.zeros(len(x))
    for t in range(len(first) - 1):
        w = np.asarray(weight[first[t]:first[t + 1]], dtype=np.float64)
        cdf[first[t]:first[t + 1]] = np.cumsum(w / w.sum())
        cdf[first[t + 1] - 1] = 1.0
    return dict(x=np.asarray(x, dtype=np.float64), P=np.asarray(P, dtype=np.float64), first=first, cdf=cdf, Phi=np.asarray(Phi, dtype=np.float64),
                Q=np.asarray(Q, dtype=np.float64), own=np.ascontiguousarray(own, dtype=np.float64), ct=ct, K=K, dt=dt, R=R, S=S, seed=seed)


_cache = {}


def scene_a():
    """70 one-component targets of models/pv, two own paths from entry 0's state: standing on, and 40 degrees after 10 s"""
    if "a" not in _cache:
        from pymht_amd.models import pv
        x, P = eref.make_batch(pv, 70, seed=3)
        Phi, Q = eref.model_matrices(pv, DT)
        _cache["a"] = scene(x, P, np.arange(71), np.ones(70), Phi, Q, own_paths(x[0, :4], CANDIDATES, K, DT))
    return _cache["a"]


def scene_c():
    """Scene A lifted to the constant-turn model's six states"""
    if "c" not in _cache:
        from pymht_amd.models import ct
        a = scene_a()
        n = len(a["x"])
        x, P = np.zeros((n, 6)), np.zeros((n, 6, 6))
        x[:, :4], x[:, 4] = a["x"], np.linspace(-0.05, 0.05, n)
        P[:, :4, :4] = a["P"]
        P[:, 4, 4], P[:, 5, 5] = 1e-4, 1e-6
        Q = np.asarray(ct.Q(DT), dtype=np.float32).astype(np.float64)
        _cache["c"] = scene(x, P, a["first"], np.ones(n), np.asarray(ct.Phi(DT, 0.0), dtype=np.float64), Q, a["own"], ct=True)
    return _cache["c"]


def scene_stride():
    """Targets 2, 37 and 38 of scene A against THREE own paths over K = 5 steps, S = 768: several chunks (3 of 256 particles), several
    paths and several targets at once, with K + 1 = 6 != G = 3 -- the smallest call in which a word of a workgroup's slab stored with
    a wrong stride (the chunk's, the path's or the target's) lands in another cell."""
    a = scene_a()
    idx = [2, 37, 38]
    cand = np.array([[0.0, 1.0, 0.0], [tref.DEG40, 1.0, 10.0], [-tref.DEG40, 1.0, 0.0]])
    return scene(a["x"][idx], a["P"][idx], np.arange(4), np.ones(3), a["Phi"], a["Q"], own_paths(a["x"][0, :4], cand, 5, DT), K=5, S=768)


def check_stride_counts(o):
    """scene_stride's own conditions on a set of counts: every (path, target) comes inside R with some and not with all particles, and
    no two targets and not all paths have the same counts, so that a transposed or mis-strided store cannot pass."""
    assert chunks(3, 768) == (3, 256)
    assert o["within"].shape == (3, 6, 3) and o["ever"].shape == (3, 3) and o["valid"].tolist() == [768] * 3 and o["status"].tolist() == [0] * 3
    assert ((o["ever"] > 0) & (o["ever"] < 768)).all() and (o["within"].sum(axis=1) > 0).all() and (o["ever"] >= o["within"].max(axis=1)).all()
    for name in ("within", "ever"):
        c = o[name]
        assert all(not np.array_equal(c[..., s], c[..., t]) for s in range(3) for t in range(s)), name      # every two targets differ
        assert sum(not np.array_equal(c[g], c[h]) for g in range(3) for h in range(g)) >= 2, name           # at least two paths differ


def reference(sc, name=None):
    """encounters() of a scene, computed once per name"""
    if name is not None and ("ref", name) in _cache:
        return _cache[("ref", name)]
    out = encounters(sc["x"], sc["P"], sc["first"], sc["cdf"], sc["Phi"], sc["Q"], sc["own"], sc["K"], sc["dt"], sc["R"], sc["S"], sc["seed"], sc["ct"])
    if name is not None:
        _cache[("ref", name)] = out
    return out


def outputs(G, K, T):
    """The seam's output arrays preset to a sentinel"""
    return dict(within=np.full((G, K + 1, T), SENTINEL, dtype=np.uint32), ever=np.full((G, T), SENTINEL, dtype=np.uint32),
                valid=np.full(T, SENTINEL, dtype=np.uint32), status=np.full(T, -7, dtype=np.int32))


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_twin(directory, sanitize=False):
    """tests/hostmath/mc_host.cpp compiled into `directory`; the ctypes library"""
    import ctypes as C
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(str(directory), "libmc_host.so")
    subprocess.check_call([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(root, "tests", "hostmath", "mc_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    vp, i32, u32, dbl = C.c_void_p, C.c_int32, C.c_uint32, C.c_double
    lib.mc_encounters_host.restype = C.c_int
    lib.mc_encounters_host.argtypes = [i32] * 7 + [C.c_uint64, dbl, dbl] + [vp] * 11
    lib.mc_philox_host.restype = None
    lib.mc_philox_host.argtypes = [u32] * 6 + [vp]
    lib.mc_normals_host.restype = None
    lib.mc_normals_host.argtypes = [i32, u32, u32, u32, C.c_uint64, vp]
    lib.mc_factor_host.restype = C.c_int
    lib.mc_factor_host.argtypes = [i32, i32, vp, vp]
    lib.mc_path_host.restype = C.c_int
    lib.mc_path_host.argtypes = [i32, i32, i32, dbl, vp, vp, vp, C.c_uint64, u32, u32, vp]
    lib.mc_chunks_host.restype = None
    lib.mc_chunks_host.argtypes = [i32, i32, vp]
    return lib


def call_twin(lib, sc, expect=0):
    """The twin on a scene: the dict of its outputs (sentinels where it refuses)"""
    N, T, G = sc["x"].shape[1], len(sc["first"]) - 1, len(sc["own"])
    xp, Pp = eref.pack(sc["x"], sc["P"])
    o = outputs(G, sc["K"], T)
    Phi, Q = np.ascontiguousarray(sc["Phi"]), np.ascontiguousarray(sc["Q"])
    rc = lib.mc_encounters_host(N, 1 if sc["ct"] else 0, len(sc["x"]), T, G, sc["K"], sc["S"], sc["seed"], sc["dt"], sc["R"], Phi.ctypes.data, Q.ctypes.data,
                                xp.ctypes.data, Pp.ctypes.data, sc["first"].ctypes.data, sc["cdf"].ctypes.data, sc["own"].ctypes.data,
                                o["within"].ctypes.data, o["ever"].ctypes.data, o["valid"].ctypes.data, o["status"].ctypes.data)
    assert rc == expect, rc
    return o


def dump(sc, path):
    """A scene as the file tests/hostmath/mc_host_main.cpp reads (the stand-alone program for a sanitizer build of the twin)"""
    N, T, G = sc["x"].shape[1], len(sc["first"]) - 1, len(sc["own"])
    xp, Pp = eref.pack(sc["x"], sc["P"])
    with open(path, "wb") as fh:
        fh.write(np.array([N, 1 if sc["ct"] else 0, len(sc["x"]), T, G, sc["K"], sc["S"], 0], dtype=np.int32).tobytes())
        fh.write(np.array([sc["seed"]], dtype=np.uint64).tobytes())
        fh.write(np.array([sc["dt"], sc["R"]], dtype=np.float64).tobytes())
        for a in (sc["Phi"], sc["Q"], xp, Pp, sc["cdf"], sc["own"]):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(sc["first"], dtype=np.int32).tobytes())
