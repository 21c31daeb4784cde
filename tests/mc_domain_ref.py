"""NumPy restatement of what `mht_mc_domain_encounters` computes (include/mht_amd.h, csrc/mht_mc_domain.h), built ON tests/mc_ref.py's own
particles through mc_pair_ref.target_paths: positions [K + 1, 2, S] of target t's particles -- the same particle the own-ship, the pair
and the zone engine are tested with.  Per (domain, path, target): the body-frame point of X_k under pose (g, k), in the header's order
    dx = X_k[0] - ox, dy = X_k[1] - oy, qx = dx * uy - dy * ux, qy = dx * ux + dy * uy
and then tests/mc_zone_ref.py's geometry on the body-frame path q_0 .. q_K (point_in, segment_crosses; q_{k-1} is the point under pose
k - 1, so the path between two steps is the STRAIGHT chord the header defines), WITHOUT the header's skip of a far cell.  Shared by
tests/test_mc_domain_cpu.py (the host twin tests/hostmath/mc_domain_host.cpp against this file) and tests/test_mc_domain_gpu.py (the
seam against the twin).

THE BORDERLINE RULE is tests/mc_zone_ref.py's, threshold and all (flags, hold_counts): tol = 1e-9 x (the domain's box diagonal); a
(particle, step) is borderline for `inside` when its body-frame point is within tol of the domain's boundary, a particle for `ever` and
`firstAt` when any of its steps is or when a vertex of the domain is within tol of one of its body-frame segments.  The cells
(domain, path) take the place of the zones.  The scenes here have NO borderline particle (tests/test_mc_domain_cpu.py asserts it), so
the counts are expected to be equal."""
import os

import numpy as np

import encounter_ref as eref
import mc_pair_ref as pref
import mc_ref as ref
import mc_zone_ref as zref
import trial_ref as tref

SENTINEL = ref.SENTINEL
COUNTS = ("inside", "firstAt", "ever", "valid", "status")
MAX_DOMAINS, MAX_VERTS, MAX_CELLS, MIN_VERTS = 4, 256, 64, 3
IDENTITY = (0.0, 0.0, 0.0, 1.0)      # the pose under which the body frame is the frame of the states

# Bow-up: (to starboard, ahead).  A pointed bow, a longer starboard side than port side
INNER = np.array([(-60, -80), (90, -80), (110, 120), (20, 330), (-70, 120)], dtype=np.float64)
OUTER = np.array([(-220, -200), (330, -200), (380, 300), (60, 820), (-10, 560), (-260, 300)], dtype=np.float64)      # concave at (-10, 560)
DOMAINS = [INNER, OUTER]
# (dpsi, f, t0): stand on; one turn to each side; one that slows; a turn with a slow-down; a hard turn after 5 s
CANDIDATES = np.array([[0.0, 1.0, 0.0], [tref.DEG40, 1.0, 10.0], [-tref.DEG40, 1.0, 0.0], [0.0, 0.5, 0.0], [0.5 * tref.DEG40, 0.7, 5.0],
                       [-2.0 * tref.DEG40, 1.0, 5.0]])


def poses_of(own, cand, K, dt, w=tref.TURN_RATE):
    from pymht_amd import evaluation
    return evaluation.mc_own_poses(own, cand, w, K, dt)


def fixed_poses(pose, K, G=1):
    """The same pose at every step of G paths"""
    return np.ascontiguousarray(np.tile(np.asarray(pose, dtype=np.float64), (G, K + 1, 1)))


def scene_d(ct=False, S=1024):
    """(scene, domains, poses): mc_ref.scene_a() or its constant-turn lift scene_c() at S = 1024 -- 70 targets, entries 5 and 9 NaN --,
    two domains and six own paths from entry 0's state"""
    sc = dict(ref.scene_c() if ct else ref.scene_a(), S=S)
    return sc, DOMAINS, poses_of(sc["x"][0, :4], CANDIDATES, sc["K"], sc["dt"])


# ---- the scenes the device is held on: tests/test_mc_domain_cpu.py asserts that none of them has a borderline particle --------------
ROUND = zref.reg(12, 250.0, (30.0, 60.0), 0.1)[::-1].copy()      # in reversed order
KINDS = ["S=64", "S=320", "T=1, S=65536", "T=1030", "K=1", "K=64", "G=1", "1 x 64", "4 x 16", "256 vertices", "67 components", "every target far",
         "near and far lanes in every wavefront"]


def _with_step(sc, K, S):
    """The scene at K steps over the same 35 s, with Phi and Q of its own step"""
    from pymht_amd.models import ct, pv
    dt = 35.0 / K
    if sc["ct"]:
        return dict(sc, K=K, dt=dt, S=S, Q=np.asarray(ct.Q(dt), dtype=np.float32).astype(np.float64))
    Phi, Q = eref.model_matrices(pv, dt)
    return dict(sc, K=K, dt=dt, S=S, Phi=Phi, Q=Q)


def shape_scene(kind):
    """(scene, domains, poses) of a shape at which the kernel takes another path"""
    a, c = ref.scene_a(), ref.scene_c()
    own = a["x"][0, :4].copy()
    beside = lambda x, off=(150.0, 60.0): np.concatenate([x[:2] - off, own[2:]])      # an own ship beside a target, with entry 0's velocity
    both = lambda sc, doms, cand, o=own: (sc, doms, poses_of(o, cand, sc["K"], sc["dt"]))
    if kind == "S=64":
        return both(dict(a, S=64), DOMAINS, CANDIDATES)
    if kind == "S=320":
        return both(dict(c, S=320), DOMAINS, CANDIDATES)
    if kind == "T=1, S=65536":
        return both(ref.scene(a["x"][12:13], a["P"][12:13], [0, 1], [1.0], a["Phi"], a["Q"], a["own"], S=65536), DOMAINS, CANDIDATES[:3],
                    beside(a["x"][12], (400.0, 300.0)))      # (the target starts 500 m ahead, about the outer domain's bow, and closes)
    if kind == "T=1030":
        idx = np.arange(1030) % 70
        return both(ref.scene(c["x"][idx], c["P"][idx], np.arange(1031), np.ones(1030), c["Phi"], c["Q"], c["own"], ct=True, S=128), [OUTER], CANDIDATES[:2])
    if kind == "K=1":
        return both(_with_step(c, 1, 512), DOMAINS, CANDIDATES)
    if kind == "K=64":
        return both(_with_step(a, 64, 256), DOMAINS, CANDIDATES[:3])
    if kind == "G=1":
        return both(dict(a, S=512), DOMAINS, CANDIDATES[1:2])
    if kind == "1 x 64":
        cand = np.array([(psi, f, 5.0) for psi in np.linspace(-1.4, 1.4, 16) for f in (0.4, 0.8, 1.0, 1.3)])
        return both(dict(c, S=256), [OUTER], cand)
    if kind == "4 x 16":
        cand = np.array([(psi, f, 0.0) for psi in np.linspace(-1.2, 1.2, 8) for f in (0.6, 1.0)])
        return both(dict(a, S=256), [INNER, OUTER, ROUND, zref.U_SHAPE + np.array([0.0, 100.0])], cand)
    if kind == "256 vertices":
        return both(dict(a, S=256), [zref.reg(256, 300.0, (20.0, 80.0), 0.05)], CANDIDATES[:2])
    rng = np.random.default_rng(67)
    if kind == "67 components":
        n = 67
        x, P = np.tile(a["x"][12], (n + 2, 1)), np.tile(a["P"][12], (n + 2, 1, 1))
        x[:n, :2] += rng.uniform(-120, 120, (n, 2))
        x[n + 1, :2] += [60.0, -40.0]
        w = np.append(rng.uniform(0, 1, n), [1.0, 1.0])
        w[[5, 66]] = 0.0
        return both(ref.scene(x, P, [0, n, n + 1, n + 2], w, a["Phi"], a["Q"], a["own"], S=1024), DOMAINS, CANDIDATES[:3], beside(a["x"][12]))
    if kind == "every target far":
        return both(dict(a, S=256), DOMAINS, CANDIDATES, own + [5e4, 5e4, 0.0, 0.0])
    assert kind.startswith("near and far")
    # three targets of two components each, one beside the own ship and one 20 km away, equal weights: a wavefront's 64 particles
    # pick both (all 64 alike: 2^-63)
    x, P = np.tile(c["x"][12], (6, 1)), np.tile(c["P"][12], (6, 1, 1))
    x[:, :2] += rng.uniform(-60, 60, (6, 2))
    x[1::2, :2] += [2e4, -2e4]
    return both(ref.scene(x, P, [0, 2, 4, 6], np.ones(6), c["Phi"], c["Q"], c["own"], ct=True, S=512), DOMAINS, CANDIDATES[:3], beside(c["x"][12]))


def pack(domains):
    return zref.pack(domains)


def body(pose, x, y):
    """pose [K + 1, 4], x and y [K + 1, S] -> (qx, qy) in the header's order"""
    ox, oy, ux, uy = (pose[:, i][:, None] for i in range(4))
    dx, dy = x - ox, y - oy
    return dx * uy - dy * ux, dx * ux + dy * uy


def encounters(sc, domains, poses, name=None):
    """The domain engine's counts of a scene (a dict of tests/mc_ref.scene) for a list of [V, 2] domains and poses [G, K + 1, 4]: inside,
    firstAt [D, G, K + 1, T], ever [D, G, T], valid [T] (uint32), status [T] (int32), borderInside, borderEver (the borderline
    particles per cell), border (their sum over ever's cells) and walked (the (cell, particle) pairs walked)."""
    tstatus, paths = pref.target_paths(sc, name)
    K, S, T, D, G = sc["K"], sc["S"], len(sc["first"]) - 1, len(domains), len(poses)
    inside, first_at = np.zeros((D, G, K + 1, T), dtype=np.uint32), np.zeros((D, G, K + 1, T), dtype=np.uint32)
    ever, valid, status = np.zeros((D, G, T), dtype=np.uint32), np.zeros(T, dtype=np.uint32), np.asarray(tstatus, dtype=np.int32).copy()
    bi, be = np.zeros((D, G, K + 1, T), dtype=np.int64), np.zeros((D, G, T), dtype=np.int64)
    walked = 0
    for t in range(T):
        if status[t]:
            continue
        valid[t] = S
        for g in range(G):
            qx, qy = body(poses[g], paths[t][:, 0], paths[t][:, 1])
            q = np.stack([qx, qy], axis=1)
            for d, poly in enumerate(domains):
                i, hit, first, near_step, near = zref.flags(poly, q)
                inside[d, g, :, t], first_at[d, g, :, t], ever[d, g, t] = i.sum(axis=1), first.sum(axis=1), hit.any(axis=0).sum()
                bi[d, g, :, t], be[d, g, t] = near_step.sum(axis=1), near.sum()
                walked += S
    return dict(inside=inside, firstAt=first_at, ever=ever, valid=valid, status=status, borderInside=bi, borderEver=be, border=int(be.sum()), walked=walked)


def cells(o):
    """A set of counts with the two cell axes as one: what tests/mc_zone_ref.py's rules take"""
    flat = lambda a, tail: a.reshape((-1,) + a.shape[-tail:])
    out = dict(o)
    for k in ("inside", "firstAt", "borderInside"):
        if k in o:
            out[k] = flat(o[k], 2)
    for k in ("ever", "borderEver"):
        if k in o:
            out[k] = flat(o[k], 1)
    return out


def hold_counts(label, got, want):
    """tests/mc_zone_ref.py's borderline rule over the cells.  Returns the number of cells that differ (expected 0 on the scenes here)."""
    return zref.hold_counts(label, cells(got), cells(want))


def same_counts(a, b):
    return zref.same_counts(a, b)


def check_invariants(out):
    zref.check_invariants(cells(out))


def outputs(D, G, K, T):
    """The seam's output arrays preset to a sentinel"""
    return dict(inside=np.full((D, G, K + 1, T), SENTINEL, dtype=np.uint32), firstAt=np.full((D, G, K + 1, T), SENTINEL, dtype=np.uint32),
                ever=np.full((D, G, T), SENTINEL, dtype=np.uint32), valid=np.full(T, SENTINEL, dtype=np.uint32), status=np.full(T, -7, dtype=np.int32))


def untouched(out):
    return zref.untouched(out)


def work_bytes(nx, nComp, T, G, D, K, S):
    """The layout of a domain call restated (csrc/mht_mc.hip's mc_layout with 2 nCell (K + 1) + nCell words per target, nCell = D G): the
    factors, the chunks' counts, the components' and the targets' status"""
    chunks, n = ref.chunks(T, S)[0], D * G
    return (nx * (nx + 1) // 2 * nComp * 8 + chunks * (2 * n * (K + 1) + n) * T * 4 + nComp * 4 + T * 4 + 255) // 256 * 256


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_twin(directory):
    """tests/hostmath/mc_domain_host.cpp compiled into `directory`; the ctypes library"""
    import ctypes as C
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(str(directory), "libmc_domain_host.so")
    subprocess.check_call([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(root, "tests", "hostmath", "mc_domain_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    vp, i32, dbl = C.c_void_p, C.c_int32, C.c_double
    lib.mc_domain_encounters_host.restype = C.c_int
    lib.mc_domain_encounters_host.argtypes = [i32] * 9 + [C.c_uint64, dbl] + [vp] * 9 + [i32] + [vp] * 5
    lib.mc_domain_body_host.restype = None
    lib.mc_domain_body_host.argtypes = [vp, dbl, dbl, vp]
    return lib


def call_twin(lib, sc, domains, poses, expect=0, packed=None, skip=True):
    """The twin on a scene, domains and poses: the dict of its outputs (sentinels where it refuses).  packed: (domFirst, domXY) as they
    are.  skip False: every cell's edge loop is run."""
    df, dxy = packed if packed is not None else pack(domains)
    df, dxy = np.ascontiguousarray(df, dtype=np.int32), np.ascontiguousarray(dxy, dtype=np.float64)
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    N, T, D, G = sc["x"].shape[1], len(sc["first"]) - 1, len(df) - 1, len(poses)
    xp, Pp = eref.pack(sc["x"], sc["P"])
    o = outputs(D, G, sc["K"], T)
    Phi, Q = np.ascontiguousarray(sc["Phi"]), np.ascontiguousarray(sc["Q"])
    rc = lib.mc_domain_encounters_host(N, 1 if sc["ct"] else 0, len(sc["x"]), T, G, D, len(dxy), sc["K"], sc["S"], sc["seed"], sc["dt"], Phi.ctypes.data, Q.ctypes.data,
                                       xp.ctypes.data, Pp.ctypes.data, sc["first"].ctypes.data, sc["cdf"].ctypes.data, poses.ctypes.data, df.ctypes.data,
                                       dxy.ctypes.data, 1 if skip else 0, o["inside"].ctypes.data, o["firstAt"].ctypes.data, o["ever"].ctypes.data,
                                       o["valid"].ctypes.data, o["status"].ctypes.data)
    assert rc == expect, rc
    return o


def twin_body(lib, pose, x, y):
    pose, out = np.ascontiguousarray(pose, dtype=np.float64), np.zeros(2)
    lib.mc_domain_body_host(pose.ctypes.data, float(x), float(y), out.ctypes.data)
    return out


def dump(sc, domains, poses, path):
    """A scene as the file tests/hostmath/mc_domain_host_main.cpp reads (the stand-alone program for a sanitizer build)"""
    df, dxy = pack(domains)
    N, T = sc["x"].shape[1], len(sc["first"]) - 1
    xp, Pp = eref.pack(sc["x"], sc["P"])
    with open(path, "wb") as fh:
        fh.write(np.array([N, 1 if sc["ct"] else 0, len(sc["x"]), T, len(poses), len(domains), len(dxy), sc["K"], sc["S"], 0], dtype=np.int32).tobytes())
        fh.write(np.array([sc["seed"]], dtype=np.uint64).tobytes())
        fh.write(np.array([sc["dt"], 0.0], dtype=np.float64).tobytes())
        for a in (sc["Phi"], sc["Q"], xp, Pp, sc["cdf"], dxy, poses):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(sc["first"], dtype=np.int32).tobytes())
        fh.write(df.tobytes())
