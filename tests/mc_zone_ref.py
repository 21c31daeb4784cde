"""NumPy restatement of what `mht_mc_zone_encounters` computes (include/mht_amd.h, csrc/mht_mc_zone.h), built ON
tests/mc_ref.encounters(..., keep_paths=True) through mc_pair_ref.target_paths: positions [K + 1, 2, S] of target t's particles -- the
same particle the own-ship and the pair engine are tested with, so particle identity is asserted and not assumed.  Per (zone, target):
in_k (X_k in the zone's box and an odd crossing number), cross_k (the segment X_{k-1} -> X_k against every edge: boxes, then the signs
of o1, o2 and of o3, o4), hit_k = in_k | cross_k, inside[k], firstAt[k] (the smallest k with hit_k) and ever -- every operation in the
header's order, vectorised over the particles, one edge at a time, WITHOUT the header's skip of a far zone.  Shared by
tests/test_mc_zone_cpu.py (the host twin tests/hostmath/mc_zone_host.cpp against this file) and tests/test_mc_zone_gpu.py (the seam
against the twin).

THE BORDERLINE RULE (hold_counts).  With tol = 1e-9 x (the zone's box diagonal): a (particle, step) is borderline for `inside` when X_k
is within tol of the zone's boundary; a particle is borderline for `ever` and `firstAt` when any of its steps is, or when any vertex of
the zone is within tol of one of its segments (a segment that grazes a corner).  The host's libm, NumPy's and the device's sin, cos and
log differ in the last bits, and only such a particle can legitimately land on the other side: a count may differ from the reference's
by at most the borderline particles of its cell -- for firstAt the `ever` figure of its (zone, target), one such particle can move
one count out of one firstAt cell and into another.  Their share is capped at mc_ref.BORDER_SHARE of the (zone, particle) pairs walked;
the scenes here have NONE, so the counts are expected to be equal."""
import os

import numpy as np

import encounter_ref as eref
import mc_pair_ref as pref
import mc_ref as ref

SENTINEL = ref.SENTINEL
COUNTS = ("inside", "firstAt", "ever", "valid", "status")
MAX_ZONES, MAX_VERTS, MIN_VERTS = 32, 1024, 3


def reg(n, r, centre, rot):
    """The regular n-gon centre + r (cos, sin)(rot + 2 pi i / n)"""
    a = rot + 2.0 * np.pi * np.arange(n) / n
    return np.asarray(centre, dtype=np.float64) + r * np.stack([np.cos(a), np.sin(a)], axis=1)


U_SHAPE = np.array([(-300, -300), (300, -300), (300, 300), (150, 300), (150, -150), (-150, -150), (-150, 300), (-300, 300)], dtype=np.float64)
SLIVER = np.array([(-2000, -1), (2000, -0.5), (2000, 0.5), (-2000, 1)], dtype=np.float64)
CONTAINING, FAR, CONVEX = 3, 4, (0, 5)      # scene Z's zones by what they are for


def centre_of(sc):
    c = np.median(sc["x"][:, :2], axis=0)
    assert np.isfinite(c).all()
    return c


def zones_z(sc):
    """Scene Z's six zones about c, the median of the targets' positions: a pentagon, a concave U, a 2 m sliver, a square that holds
    every scored particle at every step, a triangle nothing touches, and a 64-gon in reversed order"""
    c = centre_of(sc)
    return [reg(5, 400.0, c, 0.1), c + U_SHAPE, c + np.array([0.0, 37.3]) + SLIVER, np.array([(-1e5, -1e5), (1e5, -1e5), (1e5, 1e5), (-1e5, 1e5)]),
            reg(3, 50.0, c + np.array([5e4, 5e4]), 0.1), reg(64, 250.0, c + np.array([120.0, -80.0]), 0.1)[::-1].copy()]


def scene_z(ct=False):
    """(scene, zones): mc_ref.scene_a() or its constant-turn lift scene_c() at S = 1024, with zones_z"""
    sc = dict(ref.scene_c() if ct else ref.scene_a(), S=1024)
    return sc, zones_z(sc)


STRIDE_ZONES = [reg(3, 150.0, (-870.0, -370.0), 0.3), reg(4, 120.0, (-830.0, -395.0), 1.0), reg(7, 130.0, (-770.0, -310.0), 2.0)]


def scene_stride():
    """Targets 2, 37 and 38 of scene A, K = 5, S = 768 (three chunks), three zones: Z = T = 3 != K + 1 = 6, every (zone, target) hit by
    some and not all particles, no two targets and no two zones with the same counts -- a transposed or mis-strided store cannot pass"""
    a = ref.scene_a()
    idx = [2, 37, 38]
    return ref.scene(a["x"][idx], a["P"][idx], np.arange(4), np.ones(3), a["Phi"], a["Q"], np.zeros((1, 6, 2)), K=5, S=768), STRIDE_ZONES


def check_stride_counts(o):
    assert ref.chunks(3, 768) == (3, 256)
    assert o["inside"].shape == (3, 6, 3) and o["firstAt"].shape == (3, 6, 3) and o["ever"].shape == (3, 3)
    assert o["valid"].tolist() == [768] * 3 and o["status"].tolist() == [0] * 3
    assert ((o["ever"] > 0) & (o["ever"] < 768)).all()
    for name in ("inside", "firstAt", "ever"):
        c = o[name]
        assert all(not np.array_equal(c[..., s], c[..., t]) for s in range(3) for t in range(s)), name      # every two targets differ
        assert all(not np.array_equal(c[g], c[h]) for g in range(3) for h in range(g)), name                # every two zones differ


def pack(zones):
    """A list of [V, 2] arrays -> (zoneFirst int32 [nZone + 1], zoneXY float64 [nVert, 2])"""
    zones = [np.asarray(z, dtype=np.float64).reshape(-1, 2) for z in zones]
    first = np.concatenate([[0], np.cumsum([len(z) for z in zones])]).astype(np.int32)
    return first, np.ascontiguousarray(np.concatenate(zones, axis=0) if zones else np.zeros((0, 2)))


# ---- the geometry, vectorised over points ----------------------------------------------------------------------------------------------
def edges(poly):
    """(a, b) of every edge, the closing one included"""
    poly = np.asarray(poly, dtype=np.float64)
    return list(zip(poly, np.roll(poly, -1, axis=0)))


def box_of(poly):
    poly = np.asarray(poly, dtype=np.float64)
    return poly[:, 0].min(), poly[:, 1].min(), poly[:, 0].max(), poly[:, 1].max()


def point_in(poly, px, py):
    """in_k of the header for points (px, py) of any shape"""
    x0, y0, x1, y1 = box_of(poly)
    odd = np.zeros(np.shape(px), dtype=bool)
    for (ax, ay), (bx, by) in edges(poly):
        straddle = (ay > py) != (by > py)
        with np.errstate(all="ignore"):
            xi = (bx - ax) * (py - ay) / (by - ay) + ax
        odd ^= straddle & (px < xi)
    return (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1) & odd


def _part(a, b):
    return ((a >= 0) & (b <= 0)) | ((a <= 0) & (b >= 0))


def segment_crosses(poly, px, py, qx, qy):
    """cross_k of the header for segments p -> q of any shape"""
    met = np.zeros(np.shape(px), dtype=bool)
    ex, ey = qx - px, qy - py
    for (ax, ay), (bx, by) in edges(poly):
        boxes = (np.minimum(px, qx) <= max(ax, bx)) & (np.maximum(px, qx) >= min(ax, bx)) & (np.minimum(py, qy) <= max(ay, by)) & (np.maximum(py, qy) >= min(ay, by))
        fx, fy = bx - ax, by - ay
        o1, o2 = ex * (ay - py) - ey * (ax - px), ex * (by - py) - ey * (bx - px)
        o3, o4 = fx * (py - ay) - fy * (px - ax), fx * (qy - ay) - fy * (qx - ax)
        met |= boxes & _part(o1, o2) & _part(o3, o4)
    return met


def _dist_point_segment(px, py, ax, ay, bx, by):
    """The distance of points p from the segment a -> b (either may be the array)"""
    fx, fy = bx - ax, by - ay
    ff = fx * fx + fy * fy
    with np.errstate(all="ignore"):
        s = np.where(ff > 0, np.clip(((px - ax) * fx + (py - ay) * fy) / np.where(ff > 0, ff, 1.0), 0.0, 1.0), 0.0)
    return np.hypot(px - (ax + s * fx), py - (ay + s * fy))


def boundary_distance(poly, px, py):
    d = np.full(np.shape(px), np.inf)
    for (ax, ay), (bx, by) in edges(poly):
        d = np.minimum(d, _dist_point_segment(px, py, ax, ay, bx, by))
    return d


def vertex_distance(poly, px, py, qx, qy):
    """The smallest distance of a vertex of the polygon from the segments p -> q"""
    d = np.full(np.shape(px), np.inf)
    for vx, vy in np.asarray(poly, dtype=np.float64):
        d = np.minimum(d, _dist_point_segment(vx, vy, px, py, qx, qy))
    return d


def half_plane_inside(poly, px, py):
    """A CONVEX polygon by an independent rule: strictly on one side of every edge (either orientation)"""
    poly = np.asarray(poly, dtype=np.float64)
    area2 = np.sum(poly[:, 0] * np.roll(poly[:, 1], -1) - np.roll(poly[:, 0], -1) * poly[:, 1])
    sign = 1.0 if area2 > 0 else -1.0
    ok = np.ones(np.shape(px), dtype=bool)
    for (ax, ay), (bx, by) in edges(poly):
        ok &= sign * ((bx - ax) * (py - ay) - (by - ay) * (px - ax)) > 0
    return ok


def flags(poly, pos):
    """pos [K + 1, 2, S] -> (in, hit, first [K + 1, S], near_step [K + 1, S], near_particle [S]) for one zone"""
    x, y = pos[:, 0], pos[:, 1]
    inside = point_in(poly, x, y)
    cross = np.zeros_like(inside)
    cross[1:] = segment_crosses(poly, x[:-1], y[:-1], x[1:], y[1:])
    hit = inside | cross
    before = np.zeros_like(hit)
    before[1:] = np.logical_or.accumulate(hit, axis=0)[:-1]
    x0, y0, x1, y1 = box_of(poly)
    tol = ref.BORDER * np.hypot(x1 - x0, y1 - y0)
    near_step = boundary_distance(poly, x, y) < tol
    near = near_step.any(axis=0) | (vertex_distance(poly, x[:-1], y[:-1], x[1:], y[1:]) < tol).any(axis=0)
    return inside, hit, hit & ~before, near_step, near


def encounters(sc, zones, name=None):
    """The zone engine's counts of a scene (a dict of tests/mc_ref.scene) for a list of [V, 2] zones: inside, firstAt [Z, K + 1, T], ever
    [Z, T], valid [T] (uint32), status [T] (int32), borderInside [Z, K + 1, T], borderEver [Z, T], border (the borderline
    (zone, particle) pairs) and walked (the (zone, particle) pairs walked)."""
    tstatus, paths = pref.target_paths(sc, name)
    K, S, T, Z = sc["K"], sc["S"], len(sc["first"]) - 1, len(zones)
    inside, first_at = np.zeros((Z, K + 1, T), dtype=np.uint32), np.zeros((Z, K + 1, T), dtype=np.uint32)
    ever, valid, status = np.zeros((Z, T), dtype=np.uint32), np.zeros(T, dtype=np.uint32), np.asarray(tstatus, dtype=np.int32).copy()
    bi, be = np.zeros((Z, K + 1, T), dtype=np.int64), np.zeros((Z, T), dtype=np.int64)
    walked = 0
    for t in range(T):
        if status[t]:
            continue
        valid[t] = S
        for z, poly in enumerate(zones):
            i, hit, first, near_step, near = flags(poly, paths[t])
            inside[z, :, t], first_at[z, :, t], ever[z, t] = i.sum(axis=1), first.sum(axis=1), hit.any(axis=0).sum()
            bi[z, :, t], be[z, t] = near_step.sum(axis=1), near.sum()
            walked += S
    return dict(inside=inside, firstAt=first_at, ever=ever, valid=valid, status=status, borderInside=bi, borderEver=be, border=int(be.sum()), walked=walked)


def hold_counts(label, got, want):
    """The borderline rule.  Returns the number of cells that differ (expected 0 on the scenes here)."""
    assert want["border"] <= ref.BORDER_SHARE * max(want["walked"], 1), (label, "the scene has too many borderline particles", want["border"])
    diff = lambda k: np.abs(got[k].astype(np.int64) - want[k].astype(np.int64))
    di, df, de = diff("inside"), diff("firstAt"), diff("ever")
    for k, d in (("inside", di), ("firstAt", df), ("ever", de)):
        if d.any():
            print("%s: %s differs in cells %s" % (label, k, np.argwhere(d > 0)[:8].tolist()))
    assert (di <= want["borderInside"]).all(), (label, "inside", np.argwhere(di > want["borderInside"])[:5])
    assert (de <= want["borderEver"]).all(), (label, "ever", np.argwhere(de > want["borderEver"])[:5])
    assert (df <= want["borderEver"][:, None, :]).all(), (label, "firstAt", np.argwhere(df > want["borderEver"][:, None, :])[:5])
    assert (got["valid"] == want["valid"]).all() and (got["status"] == want["status"]).all(), label
    return int((di > 0).sum() + (df > 0).sum() + (de > 0).sum())


def same_counts(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and (a[k] == b[k]).all() for k in COUNTS)


def check_invariants(out):
    """What holds by construction: sum_k firstAt == ever, ever >= max_k inside, valid is 0 exactly where the status is not"""
    assert (out["firstAt"].sum(axis=1, dtype=np.int64) == out["ever"]).all()
    assert (out["ever"] >= out["inside"].max(axis=1)).all()
    assert ((out["valid"] == 0) == (out["status"] != 0)).all()
    idle = out["status"] != 0
    assert not out["inside"][:, :, idle].any() and not out["firstAt"][:, :, idle].any() and not out["ever"][:, idle].any()


def outputs(Z, K, T):
    """The seam's output arrays preset to a sentinel"""
    return dict(inside=np.full((Z, K + 1, T), SENTINEL, dtype=np.uint32), firstAt=np.full((Z, K + 1, T), SENTINEL, dtype=np.uint32),
                ever=np.full((Z, T), SENTINEL, dtype=np.uint32), valid=np.full(T, SENTINEL, dtype=np.uint32), status=np.full(T, -7, dtype=np.int32))


def untouched(out):
    return all((out[k] == SENTINEL).all() for k in ("inside", "firstAt", "ever", "valid")) and (out["status"] == -7).all()


def work_bytes(nx, nComp, T, Z, K, S):
    """The layout of a zone call restated (csrc/mht_mc.hip's mc_layout with 2 Z (K + 1) + Z words per target): the factors, the chunks'
    counts (inside, firstAt and ever of every zone and target), the components' and the targets' status"""
    chunks = ref.chunks(T, S)[0]
    return (nx * (nx + 1) // 2 * nComp * 8 + chunks * (2 * Z * (K + 1) + Z) * T * 4 + nComp * 4 + T * 4 + 255) // 256 * 256


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_twin(directory):
    """tests/hostmath/mc_zone_host.cpp compiled into `directory`; the ctypes library"""
    import ctypes as C
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(str(directory), "libmc_zone_host.so")
    subprocess.check_call([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(root, "tests", "hostmath", "mc_zone_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    vp, i32, u32, dbl = C.c_void_p, C.c_int32, C.c_uint32, C.c_double
    lib.mc_zone_encounters_host.restype = C.c_int
    lib.mc_zone_encounters_host.argtypes = [i32] * 8 + [C.c_uint64, dbl] + [vp] * 13
    lib.mc_zone_path_host.restype = C.c_int
    lib.mc_zone_path_host.argtypes = [i32] * 7 + [C.c_uint64, dbl] + [vp] * 8 + [i32, u32, i32, vp, vp]
    lib.mc_zone_test_host.restype = C.c_int
    lib.mc_zone_test_host.argtypes = [i32, vp, dbl, dbl, dbl, dbl, i32, vp]
    return lib


def call_twin(lib, sc, zones, expect=0, packed=None):
    """The twin on a scene and zones: the dict of its outputs (sentinels where it refuses).  packed: (zoneFirst, zoneXY) as they are"""
    zf, zxy = packed if packed is not None else pack(zones)
    zf, zxy = np.ascontiguousarray(zf, dtype=np.int32), np.ascontiguousarray(zxy, dtype=np.float64)
    N, T, Z = sc["x"].shape[1], len(sc["first"]) - 1, len(zf) - 1
    xp, Pp = eref.pack(sc["x"], sc["P"])
    o = outputs(Z, sc["K"], T)
    Phi, Q = np.ascontiguousarray(sc["Phi"]), np.ascontiguousarray(sc["Q"])
    rc = lib.mc_zone_encounters_host(N, 1 if sc["ct"] else 0, len(sc["x"]), T, Z, len(zxy), sc["K"], sc["S"], sc["seed"], sc["dt"], Phi.ctypes.data, Q.ctypes.data,
                                     xp.ctypes.data, Pp.ctypes.data, sc["first"].ctypes.data, sc["cdf"].ctypes.data, zf.ctypes.data, zxy.ctypes.data,
                                     o["inside"].ctypes.data, o["firstAt"].ctypes.data, o["ever"].ctypes.data, o["valid"].ctypes.data, o["status"].ctypes.data)
    assert rc == expect, rc
    return o


def twin_path(lib, sc, zones, t, p, skip=True):
    """One particle of the twin: states [K + 1, nx], inside and first [Z, K + 1] and came [Z]"""
    zf, zxy = pack(zones)
    N, T, K, Z = sc["x"].shape[1], len(sc["first"]) - 1, sc["K"], len(zones)
    xp, Pp = eref.pack(sc["x"], sc["P"])
    Phi, Q = np.ascontiguousarray(sc["Phi"]), np.ascontiguousarray(sc["Q"])
    states, fl = np.full((K + 1, N), np.nan), np.full(Z * (K + 1) * 2 + Z, -1, dtype=np.int32)
    rc = lib.mc_zone_path_host(N, 1 if sc["ct"] else 0, len(sc["x"]), T, Z, len(zxy), K, sc["seed"], sc["dt"], Phi.ctypes.data, Q.ctypes.data, xp.ctypes.data,
                               Pp.ctypes.data, sc["first"].ctypes.data, sc["cdf"].ctypes.data, zf.ctypes.data, zxy.ctypes.data, int(t), int(p), 1 if skip else 0,
                               states.ctypes.data, fl.ctypes.data)
    assert rc == 0, rc
    per = fl[:Z * (K + 1) * 2].reshape(Z, K + 1, 2)
    return dict(states=states, inside=per[..., 0].astype(bool), first=per[..., 1].astype(bool), came=fl[Z * (K + 1) * 2:].astype(bool))


def twin_test(lib, poly, p, q=None):
    """The header's predicates on one polygon: (in of q, cross of p -> q); q None: the point p alone, (in, False)"""
    poly = np.ascontiguousarray(poly, dtype=np.float64)
    out = np.full(2, -1, dtype=np.int32)
    a, b = (p, p) if q is None else (p, q)
    rc = lib.mc_zone_test_host(len(poly), poly.ctypes.data, float(a[0]), float(a[1]), float(b[0]), float(b[1]), 0 if q is None else 1, out.ctypes.data)
    assert rc == 0, rc
    return bool(out[0]), bool(out[1])


def dump(sc, zones, path):
    """A scene and its zones as the file tests/hostmath/mc_zone_host_main.cpp reads (the stand-alone program for a sanitizer build)"""
    zf, zxy = pack(zones)
    N, T = sc["x"].shape[1], len(sc["first"]) - 1
    xp, Pp = eref.pack(sc["x"], sc["P"])
    with open(path, "wb") as fh:
        fh.write(np.array([N, 1 if sc["ct"] else 0, len(sc["x"]), T, len(zones), len(zxy), sc["K"], sc["S"]], dtype=np.int32).tobytes())
        fh.write(np.array([sc["seed"]], dtype=np.uint64).tobytes())
        fh.write(np.array([sc["dt"], 0.0], dtype=np.float64).tobytes())
        for a in (sc["Phi"], sc["Q"], xp, Pp, sc["cdf"], zxy):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(sc["first"], dtype=np.int32).tobytes())
        fh.write(zf.tobytes())
