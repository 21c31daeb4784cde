"""NumPy restatement of what `mht_mc_pair_encounters` computes (include/mht_amd.h, csrc/mht_mc_pair.h), built ON
tests/mc_ref.encounters(..., keep_paths=True): its paths[t][1] is [K + 1, 2, S], the positions of target t's particles -- the same
particle the own-ship engine is tested with.  A pair's counts come from paths[a] - paths[b]: within[k] (inside R at step k), hit_k
(inside at step k, or on the segment k - 1 -> k at mht_encounter.h's clamped s*, tests/mc_ref.segment_min2), ever (any hit_k) and
firstAt[k] (the smallest k with hit_k).  Shared by tests/test_mc_pair_cpu.py (the host twin tests/hostmath/mc_pair_host.cpp against
this file) and tests/test_mc_pair_gpu.py (the seam against the twin).

THE BORDERLINE RULE is tests/mc_ref.py's (hold_counts here): borderWithin[k][j] counts the particles with | |d_k| - R | < 1e-9 R,
borderEver[j] the same for the smallest distance over all steps and segments, and borderFirst[j] the particles with ANY per-step or
per-segment minimum that close to R -- one such particle can move one count out of one firstAt cell and into another.  Their share is
capped at 1e-6 of the scene's pair-particle-steps; the scenes here have NONE, so the counts are expected to be equal."""
import os

import numpy as np

import encounter_ref as eref
import mc_ref as ref

SENTINEL = ref.SENTINEL
COUNTS = ("within", "firstAt", "ever", "valid", "status")
MAX_PAIRS = 1 << 20


def all_pairs(T):
    """The T (T - 1) / 2 pairs a < b, ascending: int32 [n, 2]"""
    a, b = np.triu_indices(T, 1)
    return np.ascontiguousarray(np.stack([a, b], axis=1), dtype=np.int32)


def target_paths(sc, name=None):
    """mc_ref.encounters of a scene with its paths kept, computed once per name: (status [T], {t: positions [K + 1, 2, S]})"""
    key = ("pair paths", name, sc["S"], sc["K"], sc["seed"])
    if name is not None and key in ref._cache:
        return ref._cache[key]
    own = sc.get("own")
    if own is None or own.shape[1] != sc["K"] + 1:      # (the own paths do not enter a pair's counts)
        own = np.zeros((1, sc["K"] + 1, 2))
    out = ref.encounters(sc["x"], sc["P"], sc["first"], sc["cdf"], sc["Phi"], sc["Q"], own, sc["K"], sc["dt"], sc["R"], sc["S"], sc["seed"], sc["ct"], keep_paths=True)
    got = (out["status"], {t: v[1] for t, v in out["paths"].items()})
    if name is not None:
        ref._cache[key] = got
    return got


def encounters(sc, pairs, name=None):
    """The pair engine's counts of a scene (a dict of tests/mc_ref.scene) for pairs [n, 2] of target indices: within, firstAt
    [K + 1, n], ever, valid [n] (uint32), status [n] (int32), borderWithin [K + 1, n], borderEver, borderFirst [n], border (the
    borderline pair-particle-steps, steps and segments) and steps (the pair-particle-steps walked)."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    tstatus, paths = target_paths(sc, name)
    K, S, R = sc["K"], sc["S"], sc["R"]
    n, R2, tol = len(pairs), R * R, ref.BORDER * R
    within, first_at = np.zeros((K + 1, n), dtype=np.uint32), np.zeros((K + 1, n), dtype=np.uint32)
    ever, valid, status = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    bw, be, bf = np.zeros((K + 1, n), dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    border = steps = 0
    for j, (a, b) in enumerate(pairs):
        sa, sb = int(tstatus[a]), int(tstatus[b])
        status[j] = 1 if 1 in (sa, sb) else (2 if 2 in (sa, sb) else 0)
        if status[j]:
            continue
        valid[j] = S
        d = paths[int(a)] - paths[int(b)]      # [K + 1, 2, S]
        dx, dy = d[:, 0], d[:, 1]
        d2 = dx * dx + dy * dy
        inside = d2 < R2
        seg = np.full_like(d2, np.inf)
        seg[1:] = ref.segment_min2(dx[:-1], dy[:-1], dx[1:], dy[1:])
        hit = inside | (seg < R2)
        before = np.zeros_like(hit)
        before[1:] = np.logical_or.accumulate(hit, axis=0)[:-1]
        within[:, j], first_at[:, j], ever[j] = inside.sum(axis=1), (hit & ~before).sum(axis=1), hit.any(axis=0).sum()
        near_step, near_seg = np.abs(np.sqrt(d2) - R) < tol, np.abs(np.sqrt(seg) - R) < tol
        bw[:, j] = near_step.sum(axis=1)
        be[j] = (np.abs(np.sqrt(np.minimum(d2, seg).min(axis=0)) - R) < tol).sum()
        bf[j] = (near_step | near_seg).any(axis=0).sum()
        border += int((near_step | near_seg).sum())
        steps += S * (K + 1)
    return dict(within=within, firstAt=first_at, ever=ever, valid=valid, status=status, borderWithin=bw, borderEver=be, borderFirst=bf, border=border, steps=steps)


def hold_counts(label, got, want):
    """The borderline rule.  Returns the number of cells that differ (expected 0 on the scenes here)."""
    assert want["border"] <= ref.BORDER_SHARE * max(want["steps"], 1), (label, "the scene has too many borderline pair-particle-steps", want["border"])
    diff = lambda k: np.abs(got[k].astype(np.int64) - want[k].astype(np.int64))
    dw, df, de = diff("within"), diff("firstAt"), diff("ever")
    assert (dw <= want["borderWithin"]).all(), (label, "within", np.argwhere(dw > want["borderWithin"])[:5])
    assert (de <= want["borderEver"]).all(), (label, "ever", np.argwhere(de > want["borderEver"])[:5])
    assert (df <= want["borderFirst"][None, :]).all(), (label, "firstAt", np.argwhere(df > want["borderFirst"][None, :])[:5])
    assert (got["valid"] == want["valid"]).all() and (got["status"] == want["status"]).all(), label
    return int((dw > 0).sum() + (df > 0).sum() + (de > 0).sum())


def same_counts(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and (a[k] == b[k]).all() for k in COUNTS)


def check_invariants(out):
    """What holds by construction: sum_k firstAt == ever, ever >= max_k within, valid is 0 exactly where the status is not"""
    assert (out["firstAt"].sum(axis=0, dtype=np.int64) == out["ever"]).all()
    assert (out["ever"] >= out["within"].max(axis=0)).all()
    assert ((out["valid"] == 0) == (out["status"] != 0)).all()
    idle = out["status"] != 0
    assert not out["within"][:, idle].any() and not out["firstAt"][:, idle].any() and not out["ever"][idle].any()


def outputs(K, n):
    """The seam's output arrays preset to a sentinel"""
    return dict(within=np.full((K + 1, n), SENTINEL, dtype=np.uint32), firstAt=np.full((K + 1, n), SENTINEL, dtype=np.uint32),
                ever=np.full(n, SENTINEL, dtype=np.uint32), valid=np.full(n, SENTINEL, dtype=np.uint32), status=np.full(n, -7, dtype=np.int32))


def untouched(out):
    return all((out[k] == SENTINEL).all() for k in ("within", "firstAt", "ever", "valid")) and (out["status"] == -7).all()


def work_bytes(nx, nComp, T, nPair, K, S):
    """csrc/mht_mc.hip's layout of a pair call restated: the factors, the chunks' counts (within, firstAt and ever of every pair), the components'
    and the pairs' status"""
    chunks = ref.chunks(nPair, S)[0]
    return (nx * (nx + 1) // 2 * nComp * 8 + chunks * (2 * (K + 1) + 1) * nPair * 4 + nComp * 4 + nPair * 4 + 255) // 256 * 256


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_twin(directory):
    """tests/hostmath/mc_pair_host.cpp compiled into `directory`; the ctypes library"""
    import ctypes as C
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(str(directory), "libmc_pair_host.so")
    subprocess.check_call([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(root, "tests", "hostmath", "mc_pair_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    vp, i32, u32, dbl = C.c_void_p, C.c_int32, C.c_uint32, C.c_double
    lib.mc_pair_encounters_host.restype = C.c_int
    lib.mc_pair_encounters_host.argtypes = [i32] * 7 + [C.c_uint64, dbl, dbl] + [vp] * 12
    lib.mc_pair_path_host.restype = C.c_int
    lib.mc_pair_path_host.argtypes = [i32] * 5 + [C.c_uint64, dbl, dbl] + [vp] * 6 + [i32, i32, u32] + [vp] * 3
    lib.mc_pair_chunks_host.restype = None
    lib.mc_pair_chunks_host.argtypes = [i32, i32, vp]
    return lib


def call_twin(lib, sc, pairs, expect=0):
    """The twin on a scene and pairs [n, 2]: the dict of its outputs (sentinels where it refuses)"""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    N, T = sc["x"].shape[1], len(sc["first"]) - 1
    xp, Pp = eref.pack(sc["x"], sc["P"])
    o = outputs(sc["K"], len(pairs))
    Phi, Q = np.ascontiguousarray(sc["Phi"]), np.ascontiguousarray(sc["Q"])
    rc = lib.mc_pair_encounters_host(N, 1 if sc["ct"] else 0, len(sc["x"]), T, len(pairs), sc["K"], sc["S"], sc["seed"], sc["dt"], sc["R"], Phi.ctypes.data,
                                     Q.ctypes.data, xp.ctypes.data, Pp.ctypes.data, sc["first"].ctypes.data, sc["cdf"].ctypes.data, pairs.ctypes.data,
                                     o["within"].ctypes.data, o["firstAt"].ctypes.data, o["ever"].ctypes.data, o["valid"].ctypes.data, o["status"].ctypes.data)
    assert rc == expect, rc
    return o


def twin_path(lib, sc, a, b, p):
    """One pair-particle of the twin: states [K + 1, 2, nx] (a, then b), the relative path [K + 1, 2], inside and first [K + 1] and came"""
    N, T, K = sc["x"].shape[1], len(sc["first"]) - 1, sc["K"]
    xp, Pp = eref.pack(sc["x"], sc["P"])
    Phi, Q = np.ascontiguousarray(sc["Phi"]), np.ascontiguousarray(sc["Q"])
    states, rel, flags = np.full((K + 1, 2, N), np.nan), np.full((K + 1, 2), np.nan), np.full(2 * (K + 1) + 1, -1, dtype=np.int32)
    rc = lib.mc_pair_path_host(N, 1 if sc["ct"] else 0, len(sc["x"]), T, K, sc["seed"], sc["dt"], sc["R"], Phi.ctypes.data, Q.ctypes.data, xp.ctypes.data,
                               Pp.ctypes.data, sc["first"].ctypes.data, sc["cdf"].ctypes.data, int(a), int(b), int(p), states.ctypes.data, rel.ctypes.data,
                               flags.ctypes.data)
    assert rc == 0, rc
    fl = flags[:-1].reshape(K + 1, 2)
    return dict(states=states, rel=rel, inside=fl[:, 0].astype(bool), first=fl[:, 1].astype(bool), came=bool(flags[-1]))


def dump(sc, pairs, path):
    """A scene and its pairs as the file tests/hostmath/mc_pair_host_main.cpp reads (the stand-alone program for a sanitizer build)"""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    N, T = sc["x"].shape[1], len(sc["first"]) - 1
    xp, Pp = eref.pack(sc["x"], sc["P"])
    with open(path, "wb") as fh:
        fh.write(np.array([N, 1 if sc["ct"] else 0, len(sc["x"]), T, len(pairs), sc["K"], sc["S"], 0], dtype=np.int32).tobytes())
        fh.write(np.array([sc["seed"]], dtype=np.uint64).tobytes())
        fh.write(np.array([sc["dt"], sc["R"]], dtype=np.float64).tobytes())
        for a in (sc["Phi"], sc["Q"], xp, Pp, sc["cdf"]):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(sc["first"], dtype=np.int32).tobytes())
        fh.write(pairs.tobytes())
