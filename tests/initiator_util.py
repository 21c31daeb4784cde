"""Streams, oracle runs and the raw-ABI driver of the initiator shape tests (test_initiator_shapes_cpu.py, test_initiator_shapes_gpu.py).

The device initiator (pymht_amd/csrc/mht_init_dev.h: initiator_body) changes path with the size of a scan: its ballot/prefix compactions
loop in passes of 1024, its new-track loop in blocks of 64 initiators, and each of its two assignment solves keeps its tables in LDS
(16-bit indices) while they fit INIT_GNN_LDS bytes and in global memory otherwise.  This module builds measurement streams that reach
those sizes, runs the live oracle (oracle/m_of_n_oracle.py) over them ONCE per case -- recording every assignment problem it solves --
and steps the device over the same stream through mht_initiator_step / mht_initiator_set_ais / mht_initiator_born, scan by scan.

Every assignment problem of every stream is checked on the CPU before anything goes to the device (`_check_problem`):
  * no connected component of the allowed graph has more than MAX_COMPONENT nodes (one device thread solves a component with Bellman-Ford
    in global memory: a giant component makes the kernel take seconds);
  * no two allowed costs of a component are equal (the optimum would be ambiguous).
A stream that breaks one of them needs another seed or density, not another assertion.
"""
import contextlib
import ctypes as C

import numpy as np

INIT_GNN_LDS = 7424          # csrc/mht_init_dev.h
INIT_ECAP = 1 << 15
NT = 1024                    # INIT_THREADS
MAX_COMPONENT = 64
T0 = 1000.0
V_MAX = 20.0
MERGE_THRESHOLD = 4 * 2.5 ** 2


def gnn_lds_bytes(n1, n2, E):
    """csrc/mht_init_dev.h::gnn_lds_bytes: e_cost 8E, bf_dist 8V, node_parent 4V, row_head + comp_head 8 n1, e_row/e_col/e_next 6E, bf_pred 2V,
    row_next + match_row 4 n1, match_col 2 n2, 64 spare."""
    V = n1 + n2
    return 14 * E + 14 * V + 12 * n1 + 2 * n2 + 64


# ---- streams -------------------------------------------------------------------------------------------------------------------------
def make_stream(seed, cohorts, cohort_size, n_scans, radius, clutter, p_d, period=2.5, track_after=4, pair_offset=None, dts=None):
    """Cohorts of straight-moving objects (position uniform in a square of half-side `radius`, velocity N(0, 7 m/s) per axis, detection
    noise 2.5 m, detection probability p_d), cohort c visible from scan c on, Poisson clutter.  Per scan (z float32 (M,2), used bool (M,),
    time), shuffled.  `used` marks what a tracker would have taken: the detections of objects that appeared at least `track_after` scans
    ago, and 10 % of the clutter.  pair_offset: object 1 moves with object 0 at that offset (their candidates are confirmed together and
    merged).  dts: the time steps (default: `period` throughout)."""
    rng = np.random.default_rng(seed)
    n_obj = cohorts * cohort_size
    pos = rng.uniform(-radius, radius, size=(n_obj, 2))
    vel = rng.normal(0.0, 7.0, size=(n_obj, 2))
    first = np.repeat(np.arange(cohorts), cohort_size)
    if pair_offset is not None:
        pos[1] = pos[0] + np.asarray(pair_offset, float)
        vel[1] = vel[0]
    scans, t = [], T0
    for k in range(n_scans):
        dt = period if dts is None else dts[k]
        t += dt
        pos = pos + dt * vel
        seen = (rng.uniform(size=n_obj) <= p_d) & (k >= first)
        det = pos[seen] + rng.normal(0.0, 2.5, size=(int(seen.sum()), 2))
        det_used = (k - first[seen]) >= track_after
        ncl = int(rng.poisson(clutter))
        cl = rng.uniform(-radius, radius, size=(ncl, 2))
        cl_used = rng.uniform(size=ncl) < 0.1
        z = np.concatenate([det, cl], axis=0)
        used = np.concatenate([det_used, cl_used])
        perm = rng.permutation(len(z))
        scans.append((np.ascontiguousarray(z[perm], dtype=np.float32).reshape(-1, 2), np.ascontiguousarray(used[perm], dtype=bool), t))
    return scans


def _pad_unused_to(scan, target, rng, radius=30000.0):
    """The scan with far-away clutter added until exactly `target` measurements are unused (the graphs stay sparse)."""
    z, used, t = scan
    n_un = int((~used).sum())
    assert n_un <= target, (n_un, target)
    far = rng.uniform(-radius, radius, size=(target - n_un, 2))
    far[np.abs(far).max(axis=1) < 2000.0] += 5000.0      # (keep it off the scene in the middle)
    z2 = np.concatenate([z.astype(np.float64), far], axis=0)
    u2 = np.concatenate([used, np.zeros(len(far), bool)])
    perm = rng.permutation(len(z2))
    z2, u2 = np.ascontiguousarray(z2[perm], dtype=np.float32).reshape(-1, 2), np.ascontiguousarray(u2[perm])
    assert int((~u2).sum()) == target
    return z2, u2, t


EDGES_DTS = [2.5, 2.5, 2.5, 1.0, 2.5, 2.5, 4.0, 2.5, 2.5, 1.0, 2.5, 4.0, 2.5]
EDGES_ROLES = {0: "empty", 3: 64, 4: 65, 5: "empty", 7: "all_used", 8: 1024, 9: 1025, 10: "one"}


def edges_stream(seed=1):
    """A hand-built stream on a dense-like scene: an empty first scan; unused counts of exactly 64, 65, 1024 and 1025 (padded with far-away
    clutter); an empty scan and a scan whose measurements are all used while preliminary tracks exist; a scan of one measurement; time
    steps of 1.0, 2.5 and 4.0 s; a pair of objects 8 m apart whose candidates merge."""
    base = make_stream(seed, 3, 6, len(EDGES_DTS), 400.0, 25, 0.95, track_after=5, pair_offset=(8.0, 0.0), dts=EDGES_DTS)
    rng = np.random.default_rng(seed + 1000)
    out = []
    for k, (z, used, t) in enumerate(base):
        role = EDGES_ROLES.get(k)
        if role == "empty":
            z, used = np.zeros((0, 2), np.float32), np.zeros(0, bool)
        elif role == "all_used":
            used = np.ones(len(z), bool)
        elif role == "one":
            j = int(np.flatnonzero(~used)[0])
            z, used = z[j:j + 1].copy(), np.zeros(1, bool)
        elif role is not None:
            z, used, t = _pad_unused_to((z, used, t), role, rng)
        out.append((z, used, t))
    return out


class AisMsg:
    __slots__ = ("time", "state", "mmsi", "used")

    def __init__(self, time, state, mmsi, used=False):
        self.time, self.state, self.mmsi, self.used = float(time), np.asarray(state, np.float64), int(mmsi), bool(used)


AIS_NO_RADAR_SCAN, AIS_NONE_SCANS, AIS_NULL_USED_SCANS = 5, (0, 6), (1, 5)


def ais_messages(scans, seed=7, period=2.5):
    """Per scan of the `dense` scene 0-40 AIS messages (list order = the order the initiator walks them):
      * `echo`: vessels that sit ON a clutter-free patch of their own and report every scan -- from the second report on their identity has a
        preliminary track (started by the first);
      * `twin`: two identities reporting nearly the same state in one scan -- the second is similar to the track the first just started;
      * `shadow`: a second identity reporting the state of an `echo` vessel one scan later -- similar to an EXISTING track;
      * strays: one-off reports anywhere on the scene;
      * about a third flagged used (a track took them) except on AIS_NULL_USED_SCANS, where the flags are passed as NULL;
      * none at all on AIS_NONE_SCANS."""
    rng = np.random.default_rng(seed)
    n_echo = 6
    e_pos, e_vel = rng.uniform(-350.0, 350.0, (n_echo, 2)), rng.normal(0.0, 4.0, (n_echo, 2))
    out, prev_echo = [], None
    for k, (_, _, t) in enumerate(scans):
        msgs = []
        if k not in AIS_NONE_SCANS:
            when = lambda: t - rng.uniform(0.2, period - 0.2)
            def at(p0, v, tm):
                return np.concatenate([p0 + v * (tm - T0), v])
            echo_now = []
            for i in range(n_echo):
                tm = when()
                s = at(e_pos[i], e_vel[i], tm) + np.concatenate([rng.normal(0.0, 0.3, 2), rng.normal(0.0, 0.05, 2)])
                msgs.append(AisMsg(tm, s, 257000100 + i))
                echo_now.append((tm, s))
            if prev_echo is not None:                       # shadows: another identity where an echo vessel's track already is
                for i in range(2):
                    tm = when()
                    s = at(e_pos[i], e_vel[i], tm) + np.concatenate([rng.normal(0.0, 0.3, 2), rng.normal(0.0, 0.05, 2)])
                    msgs.append(AisMsg(tm, s, 257000200 + 10 * k + i))
            prev_echo = echo_now
            for i in range(3):                              # twins
                tm = when()
                s = np.concatenate([rng.uniform(-380.0, 380.0, 2), rng.normal(0.0, 4.0, 2)])
                msgs.append(AisMsg(tm, s, 257001000 + 10 * k + i))
                msgs.append(AisMsg(tm + 0.05, s + np.concatenate([rng.normal(0.0, 0.5, 2), rng.normal(0.0, 0.05, 2)]), 257002000 + 10 * k + i))
            for i in range(int(rng.integers(0, 27))):       # strays
                msgs.append(AisMsg(when(), np.concatenate([rng.uniform(-400.0, 400.0, 2), rng.normal(0.0, 6.0, 2)]), 257003000 + 100 * k + i))
            order = rng.permutation(len(msgs))
            # (shuffled, but each first twin stays before its second)
            pos = {m.mmsi: j for j, m in enumerate(msgs)}
            for i in range(3):
                a, b = pos[257001000 + 10 * k + i], pos[257002000 + 10 * k + i]
                if a > b:
                    msgs[a], msgs[b] = msgs[b], msgs[a]
                    pos[msgs[a].mmsi], pos[msgs[b].mmsi] = a, b
            if k not in AIS_NULL_USED_SCANS:
                for m in msgs:
                    m.used = bool(rng.uniform() < 0.33) and not (257001000 <= m.mmsi < 257003000)
            assert len(msgs) <= 40
        out.append(msgs)
    return out


def ais_scene():
    """The radar scans of the `ais` case: the dense scene, one scan with every radar measurement used (messages only)."""
    scans = make_stream(**CASES["dense"]["stream"])
    z, used, t = scans[AIS_NO_RADAR_SCAN]
    scans[AIS_NO_RADAR_SCAN] = (z, np.ones(len(z), bool), t)
    return scans


CASES = {
    "wide": dict(stream=dict(seed=1, cohorts=5, cohort_size=450, n_scans=8, radius=20000.0, clutter=150, p_d=0.95, period=2.5, track_after=5),
                 M=3, N=5, max_meas=4096, max_prelim=4096, max_born=1024, large=True),
    "dense": dict(stream=dict(seed=2, cohorts=3, cohort_size=6, n_scans=8, radius=400.0, clutter=150, p_d=0.9, period=2.5, track_after=4),
                  M=2, N=3, max_meas=1024, max_prelim=2048, max_born=256, large=False),
    "seeds": dict(stream=dict(seed=3, cohorts=0, cohort_size=0, n_scans=4, radius=30000.0, clutter=1500, p_d=1.0, period=2.5, track_after=4),
                  M=2, N=3, max_meas=2048, max_prelim=2048, max_born=256, large=True),
    "edges": dict(M=2, N=3, max_meas=2048, max_prelim=2048, max_born=256, large=True),
    "ais": dict(M=2, N=3, max_meas=1024, max_prelim=2048, max_born=256, large=False),
}


def case_stream(name):
    """(scans, ais): the radar scans of the case and its AIS messages per scan (None: a radar-only case)."""
    if name == "edges":
        return edges_stream(), None
    if name == "ais":
        scans = ais_scene()
        return scans, ais_messages(scans)
    return make_stream(**CASES[name]["stream"]), None


# ---- the oracle's assignment, per connected component --------------------------------------------------------------------------------
def _allowed(delta, gate):
    cost = np.asarray(delta)
    return (cost <= gate) & (cost < np.inf)      # gnn_assign: cost[cost > gate] = inf; ok = cost < inf


def _components(ok):
    """Connected components of the bipartite allowed graph: (labels of the rows with an edge, labels of the columns with an edge, count)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n1, n2 = ok.shape
    r, c = np.nonzero(ok)
    g = coo_matrix((np.ones(len(r), np.int8), (r, n1 + c)), shape=(n1 + n2, n1 + n2))
    n, lab = connected_components(g, directed=False)
    return lab[:n1], lab[n1:], r, c


def gnn_assign_by_component(delta, gate=np.inf, whole=None):
    """oracle.gnn_assign (`whole`) on each connected component of the allowed graph: the padded cost of the whole matrix is (a constant) +
    the sum of the allowed costs taken + big_m per row or column left without a partner, so its optimum is a maximum matching of least
    cost in every component separately -- the same pairs wherever that optimum is unique.  Pairs in row order, as gnn_assign returns
    them (new preliminary tracks are tested against each other in that order)."""
    if whole is None:
        import m_of_n_oracle as orc
        whole = orc.gnn_assign
    delta = np.asarray(delta)
    ok = _allowed(delta, gate)
    if not ok.any():
        return []
    lr, lc, r, c = _components(ok)
    out = []
    for lab in np.unique(lr[r]):
        rows, cols = np.flatnonzero(lr == lab), np.flatnonzero(lc == lab)
        sub = np.array(delta[np.ix_(rows, cols)], copy=True)
        out.extend((rows[i], cols[j]) for i, j in whole(sub, gate))
    out.sort(key=lambda p: p[0])
    return out


def far_apart(track, other):
    """True only where PreliminaryTrack.similarity(track, other) = d' inv(P + 9 I) d is certainly above 1, from the positions alone:
    d' inv(S) d >= |d|^2 / lambda_max(S) >= |d_xy|^2 / trace(S) for the symmetric positive definite S, and the test asks for twice that
    (no rounding in either evaluation comes near a factor of 2).  On the `wide` stream 1.9 million of these tests, each with a 4 x 4
    np.linalg.inv, take 50 s; all but a few hundred are between tracks kilometres apart."""
    s, o, P = track.state, other.state, track.covariance
    dx, dy = float(s[0]) - float(o[0]), float(s[1]) - float(o[1])
    return dx * dx + dy * dy > 2.0 * (float(P[0, 0]) + float(P[1, 1]) + float(P[2, 2]) + float(P[3, 3]) + 36.0)


def _check_problem(delta, gate, where):
    """The record of one assignment problem, after the two conditions every stream must meet (module docstring)."""
    delta = np.asarray(delta)
    n1, n2 = delta.shape
    ok = _allowed(delta, gate)
    E = int(ok.sum())
    assert E <= INIT_ECAP, (where, E)
    biggest = 0
    if E:
        lr, lc, r, c = _components(ok)
        lab = lr[r]
        order = np.lexsort((delta[r, c], lab))
        sl, sc = lab[order], delta[r, c][order]
        same = (sl[1:] == sl[:-1]) & (sc[1:] == sc[:-1])
        assert not same.any(), "%s: two allowed costs of one component are equal (ambiguous optimum): change the seed or the density" % (where,)
        nodes = np.bincount(np.concatenate([lr[np.unique(r)], lc[np.unique(c)]]))      # (nodes with an edge, per component)
        biggest = int(nodes.max())
        assert biggest <= MAX_COMPONENT, "%s: a component of %d nodes (one device thread would walk it): change the seed or the density" % (where, biggest)
    lds = gnn_lds_bytes(n1, n2, E)
    return dict(where=where, n1=n1, n2=n2, V=n1 + n2, E=E, lds_bytes=lds, in_lds=bool(E > 0 and lds <= INIT_GNN_LDS), component=biggest,
                delta=None, gate=gate)


@contextlib.contextmanager
def recording_oracle(large, problems, keep_matrices=False, similar=None):
    """m_of_n_oracle with gnn_assign replaced by a form that checks and records every problem (`problems`).  large: the two shortcuts of
    the large streams -- assignment component by component (gnn_assign_by_component), the similarity test skipped between tracks that
    are far_apart; test_initiator_shapes_cpu.py holds both equal to the plain forms.  similar (a list): every similarity test that was
    evaluated, as (track, candidate's identity, <= 1)."""
    import m_of_n_oracle as orc
    whole = orc.gnn_assign
    sim = orc.PreliminaryTrack.similarity

    def gnn(delta, gate=np.inf):
        rec = _check_problem(delta, gate, (len(problems),))
        if keep_matrices:
            rec["delta"] = np.array(delta, copy=True)
        problems.append(rec)
        return gnn_assign_by_component(delta, gate, whole) if large else whole(delta, gate)

    def similarity(self, other):
        if large and far_apart(self, other):
            return np.inf
        v = sim(self, other)
        if similar is not None:
            similar.append((self, other.mmsi, bool(v <= 1.0)))
        return v
    orc.gnn_assign, orc.PreliminaryTrack.similarity = gnn, similarity
    try:
        yield orc
    finally:
        orc.gnn_assign, orc.PreliminaryTrack.similarity = whole, sim


# ---- one oracle run per case -----------------------------------------------------------------------------------------------------------
_RUNS = {}


def oracle_run(name, keep_matrices=False, large=None, n_scans=None):
    """The oracle over the stream of the case (its first n_scans scans), once per process: per scan what the device must return, the
    assignment problems, and the boundary figures the stream reached.  large: overrides the case's choice of form (recording_oracle)."""
    key = (name, keep_matrices, large, n_scans)
    if key in _RUNS:
        return _RUNS[key]
    from pymht_amd.models import pv
    from pymht_amd.utils.classDefinitions import MeasurementList
    cfg = CASES[name]
    scans, ais = case_stream(name)
    scans = scans[:n_scans]
    large = cfg["large"] if large is None else large
    problems, similar, want = [], [], []
    fig = dict(max_M=0, max_unused=0, max_prelim_in=0, max_prelim=0, max_seeds=0, max_born=0, max_V=0, n_merged=0, n_lds=0, n_global=0, n_E0=0,
               frozen_with_tracks=0, all_used=0, ais_known=0, ais_similar_old=0, ais_similar_new=0, ais_used=0, ais_only_scans=0, ais_started=0)
    with recording_oracle(large, problems, keep_matrices, similar) as orc:
        ini = orc.Initiator(cfg["M"], cfg["N"], V_MAX, pv.C_RADAR, pv.R_RADAR(), MERGE_THRESHOLD)
        for k, (z, used, t) in enumerate(scans):
            msgs = [] if ais is None else [m for m in ais[k] if not m.used]
            n_in, n_prob, n_sim = len(ini.preliminary_tracks), len(problems), len(similar)
            before = {id(p) for p in ini.preliminary_tracks}
            known = {p.mmsi for p in ini.preliminary_tracks if p.mmsi is not None}
            P_in = [np.array(p.covariance, copy=True) for p in ini.preliminary_tracks]
            n_unused = int((~used).sum())
            out = ini.processMeasurements(MeasurementList(t, z[~used]), msgs)
            x = np.array([np.asarray(b.x_0, dtype=np.float32) for b in out], dtype=np.float32).reshape(-1, 4)
            P = np.array([np.asarray(b.P_0, dtype=np.float32) for b in out], dtype=np.float32).reshape(-1, 4, 4)
            assert all(np.asarray(b.x_0).dtype == np.float32 for b in out)
            m = np.array([0 if b.measurementNumber is None else int(b.measurementNumber) for b in out], dtype=np.int32)      # (a merged birth: 0 on the device)
            want.append(dict(x=x, P=P, meas=m, n_prelim=len(ini.preliminary_tracks), n_seeds=len(ini.initiators), n_unused=n_unused))
            for p in problems[n_prob:]:
                p["where"] = (k,) + p["where"]
            fig["max_M"], fig["max_unused"] = max(fig["max_M"], len(z)), max(fig["max_unused"], n_unused)
            fig["max_prelim_in"], fig["max_prelim"] = max(fig["max_prelim_in"], n_in), max(fig["max_prelim"], len(ini.preliminary_tracks))
            fig["max_seeds"], fig["max_born"] = max(fig["max_seeds"], len(ini.initiators)), max(fig["max_born"], len(out))
            fig["n_merged"] += int((m == 0).sum())
            if n_unused == 0 and not msgs and n_in:      # frozen: the covariances move, the list and its counters do not
                assert len(ini.preliminary_tracks) == n_in and len(out) == 0
                assert all(not np.array_equal(a, p.covariance) for a, p in zip(P_in, ini.preliminary_tracks))
                fig["frozen_with_tracks"] += 1
                fig["all_used"] += int(len(z) > 0)
            if ais is not None:
                fig["ais_used"] += sum(1 for q in ais[k] if q.used)
                fig["ais_known"] += sum(1 for q in msgs if q.mmsi in known)
                fig["ais_only_scans"] += int(n_unused == 0 and len(msgs) > 0)
                hits = {}
                for trk, cand, hit in similar[n_sim:]:
                    if cand is not None and hit:
                        hits.setdefault(cand, id(trk) in before)
                fig["ais_similar_old"] += sum(1 for v in hits.values() if v)
                fig["ais_similar_new"] += sum(1 for v in hits.values() if not v)
                fig["ais_started"] += sum(1 for q in msgs if q.mmsi not in known and q.mmsi not in hits)
    for p in problems:
        fig["max_V"] = max(fig["max_V"], p["V"])
        fig["n_lds"] += int(p["in_lds"])
        fig["n_global"] += int(p["E"] > 0 and not p["in_lds"])
        fig["n_E0"] += int(p["n1"] > 0 and p["E"] == 0)
    fig["max_E"] = max([p["E"] for p in problems] or [0])
    fig["max_component"] = max([p["component"] for p in problems] or [0])
    fig["max_lds_bytes"] = max([p["lds_bytes"] for p in problems] or [0])
    run = dict(name=name, cfg=cfg, scans=scans, ais=ais, want=want, problems=problems, figures=fig)
    _RUNS[key] = run
    return run


def describe(run):
    f = run["figures"]
    keys = ["max_M", "max_unused", "max_prelim", "max_seeds", "max_born", "max_V", "max_E", "max_component", "max_lds_bytes", "n_lds", "n_global", "n_E0",
            "n_merged", "frozen_with_tracks", "all_used"]
    if run["ais"] is not None:
        keys += ["ais_started", "ais_known", "ais_similar_old", "ais_similar_new", "ais_used", "ais_only_scans"]
    return "%s: " % run["name"] + ", ".join("%s %d" % (k, f[k]) for k in keys)


# ---- the device, through the raw ABI -----------------------------------------------------------------------------------------------------
def used_words(used):
    """bool (M,) -> uint64 [ceil(M/64)], bit j of word j / 64 = measurement j is used (at least one word)."""
    b = np.packbits(np.asarray(used, bool), bitorder="little")
    w = np.zeros(max((len(used) + 63) // 64, 1) * 8, np.uint8)
    w[:len(b)] = b
    return w.view(np.uint64)


class DeviceInitiator:
    """One initiator behind mht_initiator_create, stepped scan by scan (the caller destroys it: close())."""

    def __init__(self, ctx, M_required, N_checks, max_meas=1024, max_prelim=2048, max_born=256):
        from test_initiator_gpu import make_initiator
        self.ctx, self.lib, self.max_born = ctx, ctx.lib, max_born
        self.h = make_initiator(ctx, M_required, N_checks, max_meas=max_meas, max_prelim=max_prelim, max_born=max_born)

    def close(self):
        from pymht_amd import _lib
        if self.h:
            _lib.check(self.lib.mht_initiator_destroy(self.h), self.lib)
            self.h = None

    def set_ais(self, msgs, t, null_used=False):
        from pymht_amd import _lib
        from pymht_amd.ais import initiator_messages
        arr = initiator_messages(msgs, t)
        flags = np.array([m.used for m in msgs], np.uint8)
        assert not (null_used and flags.any())
        fp = None if (null_used or not len(msgs)) else flags.ctypes.data_as(C.c_void_p)
        _lib.check(self.lib.mht_initiator_set_ais(self.h, C.byref(arr), len(msgs), fp), self.lib)

    def step(self, z, used, t):
        """-> return code of mht_initiator_step; used: bool (M,) handed over as the device bit mask, or None (NULL)."""
        import torch
        z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1, 2)
        zd = torch.from_numpy(z if len(z) else np.zeros((1, 2), np.float32)).cuda()
        ud = None if used is None else torch.from_numpy(used_words(used).view(np.int64)).cuda()
        rc = self.lib.mht_initiator_step(self.h, zd.data_ptr(), len(z), None if ud is None else ud.data_ptr(), float(t))
        self._keep = (zd, ud)      # (until mht_initiator_born has synchronised)
        return rc

    def born(self):
        """-> (return code, x float64 (n,4), P float32 (n,4,4), meas int32 (n,), n_born, n_prelim, n_seeds); canaries behind the rows."""
        cap = self.max_born
        x = np.full((cap + 1, 4), 777.0); P = np.full((cap + 1, 16), 777.0, np.float32); m = np.full(cap + 1, 777, np.int32)
        nb, npre, nseed = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        pp = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self.lib.mht_initiator_born(self.h, cap, pp(x), pp(P), pp(m), C.byref(nb), C.byref(npre), C.byref(nseed))
        n = min(nb.value, cap)
        assert np.all(x[n:] == 777.0) and np.all(P[n:] == 777.0) and np.all(m[n:] == 777), "mht_initiator_born wrote past the rows it reported"
        return rc, x[:n], P[:n].reshape(-1, 4, 4), m[:n], nb.value, npre.value, nseed.value


def compare_scan(got, want, where):
    """What test_initiator_gpu compares, exactly: births, measurement numbers, float32 states and covariances, list sizes."""
    from pymht_amd import _lib
    rc, x, P, m, nb, npre, nseed = got
    assert rc == _lib.MHT_OK, (where, rc)
    assert nb == len(want["meas"]), (where, nb, len(want["meas"]))
    assert np.array_equal(m, want["meas"]), where
    assert np.array_equal(x, want["x"].astype(np.float64)), where
    assert np.array_equal(P, want["P"]), where
    assert (npre, nseed) == (want["n_prelim"], want["n_seeds"]), (where, npre, nseed, want["n_prelim"], want["n_seeds"])


def run_device(ctx, run):
    """The device over the stream of an oracle run, compared scan by scan.  -> births in all."""
    from pymht_amd import _lib
    cfg = run["cfg"]
    dev = DeviceInitiator(ctx, cfg["M"], cfg["N"], cfg["max_meas"], cfg["max_prelim"], cfg["max_born"])
    total = 0
    try:
        for k, ((z, used, t), want) in enumerate(zip(run["scans"], run["want"])):
            if run["ais"] is not None:
                dev.set_ais(run["ais"][k], t, null_used=k in AIS_NULL_USED_SCANS)
            rc = dev.step(z, used, t)
            assert rc == _lib.MHT_OK, (run["name"], k, rc)
            got = dev.born()
            compare_scan(got, want, (run["name"], k))
            total += got[4]
    finally:
        dev.close()
    return total
