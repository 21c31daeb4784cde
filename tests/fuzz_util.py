"""Randomised parity scenarios (shared by tests/test_fuzz_gpu.py and tools/fuzz_parity.py): the drop-in Tracker (device forest, device
initiator) against the oracle (NumPy restatement of the reference, its own initiator restatement) on a random small scenario --
targets, area, clutter, N-scan window, detection probability, gate, radar period -- scan by scan."""
import os
import time

import numpy as np

# all-leaves state tolerance against the LIVE oracle (this host's BLAS): the north star's 1e-6; MHT_FUZZ_REL=0 demands bit equality
# (holds where the host's OpenBLAS picks the kernels the device arithmetic follows: Haswell / SkylakeX / Zen)
FUZZ_REL = float(os.environ.get("MHT_FUZZ_REL", "1e-6"))


def scenario_of(seed):
    from pymht_amd.utils.scenario import make_scenario
    rng = np.random.default_rng(seed)
    T = int(rng.integers(1, 70)); radius = float(rng.uniform(80, 900)); lam = float(rng.choice([0.0, 1e-6, 1e-5, 5e-5, 1.5e-4]))
    N = int(rng.integers(1, 8)); P_d = float(rng.uniform(0.5, 0.99)); eta2 = float(rng.choice([4.61, 5.99, 9.21])); period = float(rng.choice([1.0, 2.5, 4.0]))
    ns = int(rng.integers(4, 12))
    sc = make_scenario(T=T, radius=radius, lambda_phi=lam, n_scans=ns, P_d=P_d, period=period, seed=seed)
    desc = 'seed %d: T=%d r=%.0f lam=%.1e N=%d Pd=%.2f eta2=%.2f dt=%.1f scans=%d' % (seed, T, radius, lam, N, P_d, eta2, period, ns)
    return sc, N, eta2, desc


def run_case_streamed(seed, max_leaves=2000, budget_s=15.0):
    """The same scenarios with a host that streams the scans in and looks at the end: commit and admission of the initiator's births ride
    in the next scan's grow launch (fgrow_adm_kernel), reports are folded two scans late.  The oracle runs first (it decides where the
    scenario stops); per-scan statistics (from the tracker's log) and the final state are compared."""
    from test_tracker_gpu import make_tracker, tracker_selected, states_close, SCORE_ATOL
    from trace_util import make_oracle
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, N, eta2, desc = scenario_of(seed)
    g = dict(period=sc["period"], lambda_phi=sc["lambda_phi"], lambda_nu=1e-4, P_d=sc["P_d"], N=N, eta2=eta2, x0=sc["x0"], t0=sc["t0"], accepted=None)
    t0 = time.time()
    trk, acc = make_tracker(sc["period"], sc["lambda_phi"], 1e-4, sc["P_d"], N, eta2, sc["x0"], sc["t0"], logScanStats=True)
    try:
        g["accepted"] = acc
        o = make_oracle(g)
        infos = []
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            if time.time() - t0 > budget_s or (k > 0 and infos[-1]["L"] > max_leaves):
                break
            infos.append(dict(o.add_scan(float(t), z), n_ilp=o.n_ilp, n_targets=len(o.targets)))
        for z, t in zip(sc["scans"][:len(infos)], sc["times"][:len(infos)]):
            trk.addMeasurementList(MeasurementList(float(t), z))          # (nothing is looked at in between)
        os_, ts = o.selected(), tracker_selected(trk)
        lb, tb = o.leaf_batch(), trk.leafBatch()
        log = trk.scanStatsLog
        checks = [len(log) == len(infos) and all((s["L"], s["G"], s["ilp"], s["nTargets"]) == (i["L"], i["G"], i["n_ilp"], i["n_targets"]) and np.array_equal(s["unused"], i["unused"])
                                                   for s, i in zip(log, infos)),
                  [r.ID for r in o.targets] == [r.ID for r in trk.__targetList__],
                  np.array_equal(os_["ID"], ts["ID"]) and np.array_equal(os_["meas"], ts["meas"]),
                  states_close(os_["x"], ts["x"]) and np.allclose(os_["cnllr"], ts["cnllr"], rtol=0, atol=SCORE_ATOL),
                  np.array_equal(lb["ID"], tb["ID"]) and np.array_equal(lb["meas"], tb["meas"]) and states_close(lb["x"], tb["x"], rel=FUZZ_REL)]
        if not all(checks):
            return False, desc, 'MISMATCH (streamed): per-scan statistics %s targets %s selection %s states %s leaves %s' % tuple(checks)
        return True, desc, ' streamed %d scans, %d targets, %.1fs' % (len(infos), len(o.targets), time.time() - t0)
    finally:
        trk.close()


def run_case(seed, max_leaves=2000, budget_s=15.0, similar=False):
    """Returns (ok, description, message).  similar=True: similar-state pruning (addMeasurementList(pruneSimilar=True)) switched on
    and off at random from scan to scan, with a random pruneThreshold."""
    from test_tracker_gpu import make_tracker, tracker_selected, states_close, SCORE_ATOL
    from trace_util import make_oracle
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, N, eta2, desc = scenario_of(seed)
    g = dict(period=sc["period"], lambda_phi=sc["lambda_phi"], lambda_nu=1e-4, P_d=sc["P_d"], N=N, eta2=eta2, x0=sc["x0"], t0=sc["t0"], accepted=None)
    t0 = time.time()
    prng = np.random.default_rng(seed + 77)
    thr = float(prng.choice([4.0, 6.0, 12.0])) if similar else 4
    if similar:
        desc += ' similar thr=%.0f' % thr
    trk, acc = make_tracker(sc["period"], sc["lambda_phi"], 1e-4, sc["P_d"], N, eta2, sc["x0"], sc["t0"], pruneThreshold=thr)
    try:
        g["accepted"] = acc
        o = make_oracle(g)
        st, msg = {"L": 0}, ''
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            if time.time() - t0 > budget_s or (k > 0 and st["L"] > max_leaves):
                msg = 'stopped after scan %d (the oracle gets slow beyond this size)' % k
                break
            on = bool(similar and prng.uniform() < 0.75)
            info = o.add_scan(float(t), z, prune_similar=on, prune_threshold=thr)
            trk.addMeasurementList(MeasurementList(float(t), z), pruneSimilar=on)
            st = trk.lastScanStats
            os_, ts = o.selected(), tracker_selected(trk)
            lb, tb = o.leaf_batch(), trk.leafBatch()
            checks = [(st["L"], st["G"]) == (info["L"], info["G"]), np.array_equal(st["unused"], info["unused"]),
                      [r.ID for r in o.targets] == [r.ID for r in trk.__targetList__],
                      np.array_equal(os_["ID"], ts["ID"]) and np.array_equal(os_["meas"], ts["meas"]),
                      states_close(os_["x"], ts["x"]) and np.allclose(os_["cnllr"], ts["cnllr"], rtol=0, atol=SCORE_ATOL),
                      len(o.clusters) == len(trk.__clusterList__),
                      # (ALL leaves, not only the selected ones, at the north star's 1e-6 -- against a live oracle on this host's BLAS)
                      np.array_equal(lb["ID"], tb["ID"]) and np.array_equal(lb["meas"], tb["meas"]) and states_close(lb["x"], tb["x"], rel=FUZZ_REL),
                      o.n_ilp == trk.nOptimSolved]
            if not all(checks):
                return False, desc, 'MISMATCH at scan %d: gating %s unused %s targets %s selection %s states %s clusters %s leaves %s ilps %s' % ((k,) + tuple(checks))
        return True, desc, msg + ' L=%d ilp=%d %.1fs' % (st["L"], o.n_ilp, time.time() - t0)
    finally:
        trk.close()


# AIS-aided scenarios: the reference carries the covariances of a target that has met an AIS message in float64 (models/ais.py:4), and so
# does the forest (csrc/mht_vtab.h: float64 values; csrc/mht_la64.h: dgemm chains and dgesv in OpenBLAS' order): states and covariances of
# ALL leaves are compared bit for bit, in the reference's dtypes; only the cumulative scores have a tolerance (the NLLR constant's log).
AIS_SCORE_ATOL = 2e-5


def run_case_ais(seed, max_leaves=2500, budget_s=20.0):
    """AIS-aided variant (Tracker(aisAided=True), addMeasurementList(scan, aisList, aisInitialization=False); tracker.py:417-552): random
    scenario with N <= 7 and a finite radar range, random AIS traffic (share of equipped targets, report probability), similar-state
    pruning on some scans.  Decisions exact; states and covariances of the selected nodes and of all leaves bit for bit (np.array_equal,
    float64 where the reference carries float64); cumulative scores to AIS_SCORE_ATOL."""
    from trace_util import make_oracle_ais, oracle_rows
    from util import live_numpy_f64_is_pinned
    exact = live_numpy_f64_is_pinned()      # (float64 LAPACK order of THIS host's numpy = the one csrc/mht_la64.h restates)
    same = np.array_equal if exact else (lambda a, b: np.shape(a) == np.shape(b) and np.allclose(a, b, rtol=1e-12, atol=1e-12))
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import pv
    from pymht_amd.ais import AisMessage, AisMessageList
    from pymht_amd.utils.classDefinitions import MeasurementList
    from pymht_amd.utils.scenario import make_ais
    import mht_oracle as orc
    sc, N, eta2, desc = scenario_of(seed)
    N = min(N, 7)
    prng = np.random.default_rng(seed + 1234)
    equipped, p_report = float(prng.choice([0.3, 0.6, 1.0])), float(prng.choice([0.4, 0.8]))
    ais = make_ais(sc, seed=seed + 5, equipped=equipped, p_report=p_report)
    rr = 1.5 * sc["radius"]
    ais_init = bool(prng.uniform() < 0.6)          # the reference's default: messages no track took start tracks
    if ais_init and prng.uniform() < 0.5:
        sc["x0"] = sc["x0"][::2].copy()            # (half of the ships have no track at the start)
    desc += ' AIS equipped=%.1f p=%.1f N=%d init=%d' % (equipped, p_report, N, ais_init)
    g = dict(period=sc["period"], lambda_phi=sc["lambda_phi"], lambda_nu=1e-4, P_d=sc["P_d"], N=N, eta2=eta2, eta2_ais=9.45, x0=sc["x0"], t0=sc["t0"],
             radar_range=rr, position=np.asarray(sc["centre"], dtype=np.float64), with_initiator=True, accepted=None)
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=N, eta2=eta2, radarRange=rr, position=g["position"], aisAided=True,
                  maxTargets=512, maxNodes=1 << 19, maxMeasurements=512)
    t0 = time.time()
    try:
        acc = []
        for x in sc["x0"]:
            n0 = trk.nTargets
            trk.initiateTarget(Target(sc["t0"], None, x.copy(), pv.P0, status="preinitialized"))
            acc.append(trk.nTargets > n0)
        g["accepted"] = acc
        o = make_oracle_ais(g)
        st, msg, nf = {"L": 0}, '', 0
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            if time.time() - t0 > budget_s or (k > 0 and st["L"] > max_leaves):
                msg = 'stopped after scan %d' % k
                break
            on = bool(prng.uniform() < 0.3)
            msgs = ais[k] if prng.uniform() < 0.85 else []
            info = o.add_scan(float(t), z, prune_similar=on, ais=[orc.AisMessage(m[0], m[1].copy(), m[2], m[3]) for m in msgs], ais_initialization=ais_init)
            trk.addMeasurementList(MeasurementList(float(t), z), AisMessageList([AisMessage(*m) for m in msgs]), aisInitialization=ais_init, pruneSimilar=on)
            st = trk.lastScanStats
            nodes = list(trk.getTrackNodes())
            tb = trk.leafBatch()
            lb = oracle_rows([l for r in o.targets for l in r.leaves()])
            os_ = oracle_rows(o.track_nodes)
            t_mmsi = np.array([0 if n.mmsi is None else n.mmsi for n in nodes], dtype=np.int64)
            # (None without an identity: a merged new target, m_of_n.py:150 -- 0 in the oracle's table; None with one: no radar measurement)
            t_meas = np.array([(-1 if n.mmsi is not None else 0) if n.measurementNumber is None else n.measurementNumber for n in nodes], dtype=np.int64)
            o_meas = np.where((os_["meas"] == -1) & (os_["mmsi"] == 0), 0, os_["meas"])
            nf += info["n_fused"]
            t_x = np.array([np.asarray(n.x_0, dtype=np.float64) for n in nodes]).reshape(-1, 4)
            checks = [st["L"] == info["L"], np.array_equal(st["unused"], info["unused"]),
                      [r.ID for r in o.targets] == [r.ID for r in trk.__targetList__],
                      np.array_equal(os_["ID"], [n.ID for n in nodes]) and np.array_equal(o_meas, t_meas) and np.array_equal(os_["mmsi"], t_mmsi),
                      same(os_["x"], t_x) and np.allclose(os_["cnllr"], [float(n.cumulativeNLLR) for n in nodes], rtol=0, atol=AIS_SCORE_ATOL),
                      len(o.clusters) == len(trk.__clusterList__) and all(np.array_equal(a, np.asarray(b)) for a, b in zip(o.clusters, trk.__clusterList__)),
                      np.array_equal(lb["ID"], tb["ID"]) and np.array_equal(lb["meas"], tb["meas"]) and np.array_equal(lb["mmsi"], tb["mmsi"])
                      and same(lb["x"], tb["x"]) and np.array_equal(lb["Pf64"], tb["Pf64"]) and same(lb["P"], tb["P"])
                      and np.allclose(lb["cnllr"], tb["cnllr"], rtol=0, atol=AIS_SCORE_ATOL),
                      o.n_ilp == trk.nOptimSolved]
            if not all(checks):
                return False, desc, 'MISMATCH at scan %d: L %s unused %s targets %s selection %s states %s clusters %s leaves %s ilps %s' % ((k,) + tuple(checks))
        return True, desc, msg + ' L=%d fused=%d ilp=%d %.1fs' % (st["L"], nf, o.n_ilp, time.time() - t0)
    finally:
        trk.close()


def run_case_ct(seed, max_leaves=2500, budget_s=15.0, similar=False):
    """Constant-turn forests (pymht_amd/models/ct.py, six states; MHT_FOREST_CT): every hypothesis its own Phi(T, w), formed on the device
    from its f64 sin / cos.  Random scenario as above, every root with a RANDOM turn rate w (from exactly 0 and |w| below the model's
    straight-line threshold through gentle turns to 0.6 rad/s) and turn-rate derivative a, against the live oracle whose per-leaf arithmetic
    is the reference's kalman.predict_single + kalman.precalc restated (oracle.process_leaves_ct; kalman.py:67-70, :82-101).
    Decisions -- gating counts, unused measurements, target lists, clusters, selections, leaf sets, number of ILPs -- exact; states and
    covariances of all leaves 1e-6.  similar=True: similar-state pruning (tracker.py:230-231, :1233-1239; pyTarget.py:358-412) switched on and off at
    random from scan to scan with a random merge radius -- the merged node's mean covariance lives under the missed-detection child's key."""
    from test_tracker_gpu import tracker_selected, states_close, SCORE_ATOL
    from trace_util import make_oracle
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import ct
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, N, eta2, desc = scenario_of(seed)
    prng = np.random.default_rng(seed + 4242)
    T = len(sc["x0"])
    kind = prng.integers(0, 5, size=T)
    w = np.where(kind == 0, 0.0, np.where(kind == 1, prng.uniform(-1e-9, 1e-9, size=T), np.where(kind == 2, prng.normal(0.0, 0.02, size=T),
                 np.where(kind == 3, prng.uniform(-0.6, 0.6, size=T), prng.normal(0.0, 0.15, size=T)))))
    a = np.where(prng.uniform(size=T) < 0.5, 0.0, prng.normal(0.0, 1e-3, size=T))
    x0 = np.concatenate([sc["x0"], w[:, None], a[:, None]], axis=1)
    thr = float(prng.choice([4.0, 6.0, 12.0])) if similar else 4
    desc += ' CT |w|max=%.3f' % float(np.abs(w).max()) + (' similar thr=%.0f' % thr if similar else '')
    trk = Tracker(ct, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=N, eta2=eta2, useInitiator=False, maxTargets=256, maxNodes=1 << 18, maxMeasurements=512,
                  pruneThreshold=thr)
    t0 = time.time()
    try:
        acc = []
        for x in x0:
            n0 = trk.nTargets
            trk.initiateTarget(Target(sc["t0"], None, x.copy(), ct.P0, status="preinitialized"))
            acc.append(trk.nTargets > n0)
        g = dict(period=sc["period"], lambda_phi=sc["lambda_phi"], lambda_nu=1e-4, P_d=sc["P_d"], N=N, eta2=eta2, x0=x0, t0=sc["t0"], accepted=acc)
        o = make_oracle(g, with_initiator=False, model=ct)
        st, msg = {"L": 0}, ''
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            if time.time() - t0 > budget_s or (k > 0 and st["L"] > max_leaves):
                msg = 'stopped after scan %d' % k
                break
            on = bool(similar and prng.uniform() < 0.75)
            info = o.add_scan(float(t), z, prune_similar=on, prune_threshold=thr)
            trk.addMeasurementList(MeasurementList(float(t), z), pruneSimilar=on)
            st = trk.lastScanStats
            os_, ts = o.selected(), tracker_selected(trk, 6)
            lb, tb = o.leaf_batch(), trk.leafBatch()
            checks = [(st["L"], st["G"]) == (info["L"], info["G"]), np.array_equal(st["unused"], info["unused"]),
                      [r.ID for r in o.targets] == [r.ID for r in trk.__targetList__],
                      np.array_equal(os_["ID"], ts["ID"]) and np.array_equal(os_["meas"], ts["meas"]),
                      states_close(os_["x"], ts["x"]) and np.allclose(os_["cnllr"], ts["cnllr"], rtol=0, atol=SCORE_ATOL),
                      len(o.clusters) == len(trk.__clusterList__) and all(np.array_equal(a_, np.asarray(b_)) for a_, b_ in zip(o.clusters, trk.__clusterList__)),
                      np.array_equal(lb["ID"], tb["ID"]) and np.array_equal(lb["meas"], tb["meas"]) and states_close(lb["x"], tb["x"], rel=1e-6)
                      and states_close(lb["P"], np.asarray(tb["P"], dtype=np.float64), rel=1e-6),
                      o.n_ilp == trk.nOptimSolved]
            if not all(checks):
                return False, desc, 'MISMATCH at scan %d: gating %s unused %s targets %s selection %s states %s clusters %s leaves %s ilps %s' % ((k,) + tuple(checks))
        return True, desc, msg + ' L=%d ilp=%d %.1fs' % (st["L"], o.n_ilp, time.time() - t0)
    finally:
        trk.close()


# ---- linear six-state forests (Tracker(pymht_amd.models.ca, ...)): the four-state forest's kernels at NX = 6 ------------------------------
# The oracle runs FIRST and alone (oracle_run): it decides where a scene stops -- the leaf cap alone, no clock, so a scene is the same on
# every host -- keeps what every scan has to look like, and counts what the scene exercises (its census).  tests/test_six_state_fuzz_cpu.py
# asserts the census without a device; device_run steps a Tracker through the same scans against the record.
CA_SEED0 = int(os.environ.get("MHT_FUZZ_SEED", "20000"))
CA_PLAIN_SEEDS = [CA_SEED0 + 300000 + i for i in range(24)]
CA_SIMILAR_SEEDS = [CA_SEED0 + 350000 + i for i in range(24)]
CA_MAX_LEAVES = 1500
SHARDED_SEED = 320017      # a plain-slice scene whose largest cluster has 34 targets
VTAB_SCANS = 22        # the second switch of a 2 048-id table comes in front of scan 20; two more scans run on the third generation


def ca_tails(seed, T):
    """[ax, ay] per root from default_rng(seed + 4242): half of the targets exactly 0 (all G17 and cfg5 ever start from), the others N(0, 0.3) m/s^2."""
    prng = np.random.default_rng(seed + 4242)
    zero = prng.uniform(size=T) < 0.5
    return np.where(zero[:, None], 0.0, prng.normal(0.0, 0.3, size=(T, 2)))


def similar_draw(seed, similar, n_scans):
    """pruneThreshold and the per-scan switch of similar-state pruning, drawn as run_case draws them."""
    prng = np.random.default_rng(seed + 77)
    thr = float(prng.choice([4.0, 6.0, 12.0])) if similar else 4
    return thr, [bool(similar and prng.uniform() < 0.75) for _ in range(n_scans)]


def scene_of(sc, N, eta2, thr, on, desc, model="ca", tails=None, P0s=None, kinds=None, max_meas=512):
    """A scene: scenario, window, gate, merge radius, the per-scan pruning switches and the roots of the model ([x4, ax, ay] for ca,
    [x4, w, a] for ct).  P0s: one covariance per root (None: the model's P0 for every root); kinds: the turn-rate kinds of ct roots
    (ct_draw); max_meas: the forest's maxMeasurements."""
    x0 = sc["x0"] if model == "pv" else np.concatenate([sc["x0"], np.zeros((len(sc["x0"]), 2)) if tails is None else tails], axis=1)
    return dict(sc=sc, N=int(N), eta2=float(eta2), thr=thr, on=list(on), desc=desc, model=model, x0=x0, P0s=P0s, kinds=kinds, max_meas=int(max_meas))


def ca_scene(seed, similar=False):
    sc, N, eta2, desc = scenario_of(seed)
    thr, on = similar_draw(seed, similar, len(sc["scans"]))
    tails = ca_tails(seed, len(sc["x0"]))
    return scene_of(sc, N, eta2, thr, on, desc + ' CA |a|max=%.2f' % float(np.abs(tails).max()) + (' similar thr=%.0f' % thr if similar else ''), tails=tails)


# dense scenes that fuse large groups of hits (N, P_d, thr, lambda_phi, seed, T, radius): means over 3, 5, 6, 7 and more than 16 hits -- the
# path of mht_similar.hip::fuse_group that inserts a covariance value, takes a pseudo-parent key and writes a gains row
CRAFTED = {"A": (2, 0.95, 15.0, 1e-3, 23, 25, 250.0), "B": (3, 0.9, 25.0, 3e-3, 24, 12, 150.0), "C": (2, 0.9, 30.0, 4e-3, 25, 8, 120.0)}


def crafted_scene(name, model="ca"):
    """Zero acceleration tails, eta2 5.99, similar-state pruning on at EVERY scan (the runner's 0.75 draw would thin the large groups)."""
    from pymht_amd.utils.scenario import make_scenario
    N, P_d, thr, lam, seed, T, radius = CRAFTED[name]
    sc = make_scenario(T=T, radius=radius, lambda_phi=lam, n_scans=10, P_d=P_d, seed=seed)
    return scene_of(sc, N, 5.99, thr, [True] * 10, 'crafted %s (%s): T=%d r=%.0f lam=%.1e N=%d Pd=%.2f thr=%.0f' % (name, model, T, radius, lam, N, P_d, thr), model=model)


LONG_WINDOWS = {8: dict(T=15, P_d=0.8, seed=31), 9: dict(T=10, P_d=0.85, seed=32)}


def long_window_scene(N, model="ca"):
    """Windows of 8 and 9 scans: path records of 16 ints, targets of more than 128 leaves.  model="ct": ct_long_window_scene."""
    from pymht_amd.utils.scenario import make_scenario
    if model == "ct":
        return ct_long_window_scene(N)
    p = LONG_WINDOWS[N]
    sc = make_scenario(T=p["T"], radius=400.0, lambda_phi=1e-5, n_scans=12, P_d=p["P_d"], seed=p["seed"])
    return scene_of(sc, N, 5.99, 4, [False] * 12, 'long window N=%d: T=%d Pd=%.2f' % (N, p["T"], p["P_d"]), tails=ca_tails(p["seed"], p["T"]))


def vtab_scene(n_scans=VTAB_SCANS, T=12):
    """A stream with cfg2's clutter density, detection probability and window (1e-4 per m^2, 0.9, N = 3) and pruning on six scans of seven.
    It has 12 targets where cfg2 has 50: six-state covariances do not settle to a handful of float32 values as the four-state ones do (the
    oracle meets ~120 new values per scan here, ~350 with 50 targets), and a generation of a 2 048-id table has to last R + 2 scans."""
    from pymht_amd.utils.scenario import make_scenario
    sc = make_scenario(T=T, radius=500.0, lambda_phi=1e-4, n_scans=n_scans, P_d=0.9, seed=5446)
    return scene_of(sc, 3, 5.99, 4, [k % 7 != 5 for k in range(n_scans)], 'cfg2-like stream, %d targets, %d scans' % (T, n_scans), tails=ca_tails(5446, T))


def sector_scenes():
    """Two different scenes with one window (members of a group share the forest configuration): the first prunes on three scans of four."""
    from pymht_amd.utils.scenario import make_scenario
    a = make_scenario(T=40, radius=500.0, lambda_phi=6e-5, n_scans=10, P_d=0.85, seed=41)
    b = make_scenario(T=30, radius=400.0, lambda_phi=4e-5, n_scans=10, P_d=0.9, seed=42)
    return [scene_of(a, 3, 5.99, 7.5, [k % 4 != 1 for k in range(10)], 'sector 0', tails=ca_tails(41, 40)),
            scene_of(b, 3, 5.99, 4, [False] * 10, 'sector 1', tails=ca_tails(42, 30))]


# ---- constant-turn forests (Tracker(pymht_amd.models.ct, ...)) in the same deterministic runner ---------------------------------------------
# run_case_ct above stops on a clock; these scenes stop on the leaf cap alone, and oracle_run counts for them what fgrow_ct_kernel's own
# paths depend on (ct_grow_census).  tests/test_ct_fuzz_cpu.py asserts that census without a device.
# (twelve seeds each out of the ranges of test_fuzz_slice_constant_turn and test_constant_turn_forest_similar_state_pruning, picked with the
# census: windows of 1 .. 7 scans, candidate lists of more than 64 measurements (5, 12, 51), targets of more than 128 leaves, groups of three hits)
CT_PLAIN_SEEDS = [CA_SEED0 + 700000 + i for i in (0, 2, 5, 6, 8, 9, 12, 20, 26, 51, 59, 69)]
CT_SIMILAR_SEEDS = [880000 + i for i in (0, 6, 9, 10, 11, 13, 19, 22, 23, 24, 29, 30)]
CT_KINDS = 5      # turn-rate kinds of a root: 0 exactly zero, 1 |w| < 1e-9 (below the model's straight-line threshold), 2 N(0, 0.02), 3 U(-0.6, 0.6), 4 N(0, 0.15)
CT_CHUNK = 128    # leaves of a chunk of fgrow_ct_kernel (FG_CAP)


def ct_draw(seed, T):
    """(kind, [w, a]) per root from default_rng(seed + 4242), draw for draw as run_case_ct: the five kinds of turn rate (CT_KINDS), a exactly 0
    for half of the roots and N(0, 1e-3) for the others."""
    prng = np.random.default_rng(seed + 4242)
    kind = prng.integers(0, 5, size=T)
    w = np.where(kind == 0, 0.0, np.where(kind == 1, prng.uniform(-1e-9, 1e-9, size=T), np.where(kind == 2, prng.normal(0.0, 0.02, size=T),
                 np.where(kind == 3, prng.uniform(-0.6, 0.6, size=T), prng.normal(0.0, 0.15, size=T)))))
    a = np.where(prng.uniform(size=T) < 0.5, 0.0, prng.normal(0.0, 1e-3, size=T))
    return kind, np.stack([w, a], axis=1)


def ct_tails(seed, T):
    """[w, a] per root, exactly as run_case_ct draws them."""
    return ct_draw(seed, T)[1]


def ct_scene(seed, similar=False):
    sc, N, eta2, desc = scenario_of(seed)
    thr, on = similar_draw(seed, similar, len(sc["scans"]))
    kinds, tails = ct_draw(seed, len(sc["x0"]))
    return scene_of(sc, N, eta2, thr, on, desc + ' CT |w|max=%.3f' % float(np.abs(tails[:, 0]).max()) + (' similar thr=%.0f' % thr if similar else ''),
                    model="ct", tails=tails, kinds=kinds)


def ct_long_window_scene(N):
    """long_window_scene's streams under models.ct: turn rates N(0, 0.05) from default_rng(seed + 4242), turn-rate derivatives 0."""
    from pymht_amd.utils.scenario import make_scenario
    p = LONG_WINDOWS[N]
    sc = make_scenario(T=p["T"], radius=400.0, lambda_phi=1e-5, n_scans=12, P_d=p["P_d"], seed=p["seed"])
    w = np.random.default_rng(p["seed"] + 4242).normal(0.0, 0.05, size=p["T"])
    return scene_of(sc, N, 5.99, 4, [False] * 12, 'long window N=%d (ct): T=%d Pd=%.2f' % (N, p["T"], p["P_d"]), model="ct",
                    tails=np.stack([w, np.zeros(p["T"])], axis=1))


CT_LONG_CAP = {8: None, 9: 4000}      # leaf cap of the long-window scenes (N = 9 grows past what a test of a few seconds holds)

# two-scan streams of dense clutter in which root 0 starts with a position variance of sigma^2 (the others with ct.P0): its gate box holds
# hundreds of measurements -- the widths of fgrow_ct_kernel's hit masks over the candidate list (2 .. FG_HWC = 6 words per leaf in LDS) and,
# past 384 candidates, the full-width masks in global memory beside targets that stay in LDS.  (T, radius, lambda_phi, N, seed, sigma)
WIDE_GATE = {"a": (4, 150.0, 2e-2, 1, 61, 30.0), "b": (4, 200.0, 1e-2, 2, 62, 40.0), "c": (4, 150.0, 2e-2, 1, 64, 25.0), "d": (4, 200.0, 1e-2, 2, 64, 45.0),
             "e": (4, 200.0, 1e-2, 1, 63, 45.0)}


def wide_gate_scene(name):
    """Zero tails, eta2 5.99, P_d 0.9, no similar-state pruning, two scans; the forest takes 2 048 measurements per scan."""
    from pymht_amd.utils.scenario import make_scenario
    from pymht_amd.models import ct
    T, radius, lam, N, seed, sigma = WIDE_GATE[name]
    sc = make_scenario(T=T, radius=radius, lambda_phi=lam, n_scans=2, P_d=0.9, seed=seed)
    wide = np.array(ct.P0, copy=True)
    wide[0, 0] = wide[1, 1] = sigma * sigma
    return scene_of(sc, N, 5.99, 4, [False] * 2, 'wide gate %s: T=%d r=%.0f lam=%.1e N=%d sigma=%.0f' % (name, T, radius, lam, N, sigma), model="ct",
                    P0s=[wide] + [ct.P0] * (T - 1), max_meas=2048)


def ct_grow_census(r, C, eta2, z):
    """What one call of process_leaves_ct (one target, one scan) asks of fgrow_ct_kernel, from the oracle's own x_bar, S and gate indices in
    float64:
      cand      measurements inside the union over the target's leaves of z_hat +- sqrt(eta2 diag S), the bounding box of the leaf's exact
                gate.  A LOWER bound on the device's candidate list: the device takes the measurements inside one box around all of its
                leaves' boxes, and every leaf's box there is widened (conservative in float32) -- its list is never shorter;
      leaves    the leaf count;
      children  the sum over the leaves of 1 + hits;
      chunk     the largest such sum over CT_CHUNK consecutive leaves (the children of one chunk of the kernel)."""
    x_bar, S = np.asarray(r["x_bar"], dtype=np.float64), np.asarray(r["S"], dtype=np.float64)
    z_hat = x_bar.dot(np.asarray(C, dtype=np.float64).T)
    half = np.sqrt(float(eta2) * np.stack([S[:, 0, 0], S[:, 1, 1]], axis=1))
    zz = np.asarray(z, dtype=np.float64).reshape(-1, 2)
    inside = np.zeros(len(zz), dtype=bool)
    for i in range(len(z_hat)):
        inside |= np.all(np.abs(zz - z_hat[i]) <= half[i], axis=1)
    kids = 1 + np.array([len(i) for i in r["idx"]], dtype=np.int64)
    return dict(cand=int(inside.sum()), leaves=len(kids), children=int(kids.sum()),
                chunk=int(max(kids[c:c + CT_CHUNK].sum() for c in range(0, len(kids), CT_CHUNK))))


def ct_grow_rows(census):
    """The (scan, target, figures) rows of a constant-turn census."""
    return [(k, ti, g) for k, scan in enumerate(census["grow"]) for ti, g in enumerate(scan)]


def _model_of(scene):
    from pymht_amd.models import pv, ca, ct
    return {"pv": pv, "ca": ca, "ct": ct}[scene["model"]]


def _root_covariances(scene):
    """One covariance per root: scene["P0s"], or the model's P0 for every root."""
    P0 = _model_of(scene).P0
    return [P0] * len(scene["x0"]) if scene.get("P0s") is None else list(scene["P0s"])


def oracle_run(scene, max_leaves=None):
    """The oracle alone over a scene.  Returns dict(accepted, scans=[per-scan record], census): the census holds the number of ILPs, the
    largest cluster, the terminations, the largest L and the sizes of the fused groups (the number of hit children every call of
    Node.prune_similar removed: the call is wrapped here and computes what it always does)."""
    import mht_oracle as orc
    from trace_util import oracle_rows
    sc, model = scene["sc"], _model_of(scene)
    nx = scene["x0"].shape[1]
    o = orc.OracleTracker(sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=scene["N"], eta2=scene["eta2"], initiator=None,
                          model=None if scene["model"] == "pv" else model)
    acc = [o.initiate_target(sc["t0"], x.copy(), np.array(P0, copy=True), status="preinitialized") for x, P0 in zip(scene["x0"], _root_covariances(scene))]
    groups, merged, grown = [], [], []
    plain, plain_ct = orc.Node.prune_similar, orc.process_leaves_ct

    def counting(node, threshold):
        before = len(node.kids)
        plain(node, threshold)
        if len(node.kids) != before:
            groups.append(before - len(node.kids))
            merged.append(node.kids[0])

    def counting_ct(phi, T, Q, C, R, eta2, lambda_ex, x, P, P_d, z):
        r = plain_ct(phi, T, Q, C, R, eta2, lambda_ex, x, P, P_d, z)
        grown.append(ct_grow_census(r, C, eta2, z))
        return r

    census = dict(ilp=0, cluster=0, dead=0, L=0, groups=groups, scans=0, merged_leaves=0)
    if scene["model"] == "ct":
        census.update(grow=[], kinds=[] if scene.get("kinds") is None else sorted(set(int(q) for q in scene["kinds"])))
    recs = []
    orc.Node.prune_similar, orc.process_leaves_ct = counting, counting_ct
    try:
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            if max_leaves is not None and k > 0 and recs[-1]["L"] > max_leaves:
                break
            del merged[:]
            del grown[:]
            info = o.add_scan(float(t), z, prune_similar=scene["on"][k], prune_threshold=scene["thr"])
            if scene["model"] == "ct":
                census["grow"].append(list(grown))      # (one entry per target, in the order of the target list in front of the scan)
            leaves = [l for r in o.targets for l in r.leaves()]
            m_ids = set(id(n) for n in merged)
            lb, sel = oracle_rows(leaves, nx), oracle_rows(o.track_nodes, nx)
            recs.append(dict(L=info["L"], G=info["G"], unused=info["unused"].copy(), ids=[r.ID for r in o.targets], n_ilp=o.n_ilp,
                             clusters=[np.asarray(c).copy() for c in o.clusters], sel=sel, leaves=lb,
                             merged=np.array([id(l) in m_ids for l in leaves], dtype=bool)))
            census["ilp"] += o.n_ilp
            census["cluster"] = max([census["cluster"]] + [len(c) for c in o.clusters])
            census["dead"] += len(info["dead"])
            census["L"] = max(census["L"], info["L"])
            census["merged_leaves"] += int(recs[-1]["merged"].sum())
    finally:
        orc.Node.prune_similar, orc.process_leaves_ct = plain, plain_ct
    census["scans"] = len(recs)
    census["groups"] = list(groups)
    return dict(accepted=acc, scans=recs, census=census)


def group_histogram(groups):
    return {int(s): int(n) for s, n in zip(*np.unique(np.asarray(groups, dtype=np.int64), return_counts=True))}


def _rows_close(a, b, rel):
    """Every row within rel of its largest element (at least 1), as run_case_ct holds states and covariances; rel = 0: bit equality."""
    from test_tracker_gpu import states_close
    return states_close(a, np.asarray(b, dtype=np.float64), rel=rel)


def device_run(scene, rec, streamed=False, spill=False):
    """A Tracker over the scans the oracle ran, against its record.  Looked at after every scan: L, G, unused measurements, target ids,
    ILPs, selections, clusters member for member, leaf ids and measurement numbers exactly; states and covariances of ALL leaves (the
    merged ones once more on their own) at FUZZ_REL -- in a constant-turn scene at the 1e-6 run_case_ct holds them to, whatever FUZZ_REL
    says: the device's sin / cos may round an entry of Phi(T, w) one ulp away from NumPy's --, cumulative scores at SCORE_ATOL; no leaf
    carries flag 8.  streamed: nothing is looked at in between -- the per-scan numbers come from the tracker's log, the rest is compared
    at the end.  spill: MHT_CT_SPILL=1 while the Tracker is made (fgrow_ct_kernel then keeps every target's hit masks in the global
    block).  Returns (ok, message)."""
    from test_tracker_gpu import tracker_selected, SCORE_ATOL
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.utils.classDefinitions import MeasurementList
    sc, model = scene["sc"], _model_of(scene)
    nx = scene["x0"].shape[1]
    rel = 1e-6 if scene["model"] == "ct" else FUZZ_REL
    before = os.environ.get("MHT_CT_SPILL")
    if spill:
        os.environ["MHT_CT_SPILL"] = "1"
    try:
        trk = Tracker(model, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=scene["N"], eta2=scene["eta2"], useInitiator=False, maxTargets=256,
                      maxNodes=1 << 18, maxMeasurements=scene.get("max_meas", 512), pruneThreshold=scene["thr"], logScanStats=streamed)
    finally:
        if spill:
            if before is None:
                del os.environ["MHT_CT_SPILL"]
            else:
                os.environ["MHT_CT_SPILL"] = before
    t0 = time.time()

    def state_checks(r):
        os_, ts = r["sel"], tracker_selected(trk, nx)
        lb, tb = r["leaves"], trk.leafBatch()
        same_leaves = np.array_equal(lb["ID"], tb["ID"]) and np.array_equal(lb["meas"], tb["meas"])
        m = r["merged"]
        return [("targets", r["ids"] == [q.ID for q in trk.__targetList__]),
                ("selection", np.array_equal(os_["ID"], ts["ID"]) and np.array_equal(os_["meas"], ts["meas"])),
                ("selected states", _rows_close(os_["x"], ts["x"], 1e-6) and np.allclose(os_["cnllr"], ts["cnllr"], rtol=0, atol=SCORE_ATOL)),
                ("clusters", len(r["clusters"]) == len(trk.__clusterList__) and all(np.array_equal(a, np.asarray(b)) for a, b in zip(r["clusters"], trk.__clusterList__))),
                ("leaves", same_leaves),
                ("leaf states", same_leaves and _rows_close(lb["x"], tb["x"], rel)),
                ("leaf covariances", same_leaves and _rows_close(lb["P"], tb["P"], rel)),
                ("merged leaves' covariances", same_leaves and _rows_close(lb["P"][m], tb["P"][m], rel)),
                ("leaf scores", same_leaves and np.allclose(lb["cnllr"], tb["cnllr"], rtol=0, atol=SCORE_ATOL)),
                ("flag 8", not np.any(tb["flags"] & 8))]

    try:
        acc = []
        for x, P0 in zip(scene["x0"], _root_covariances(scene)):
            n0 = trk.nTargets
            trk.initiateTarget(Target(sc["t0"], None, x.copy(), P0, status="preinitialized"))
            acc.append(trk.nTargets > n0)
        if acc != rec["accepted"]:
            return False, 'MISMATCH: the roots the device admits'
        for k, r in enumerate(rec["scans"]):
            trk.addMeasurementList(MeasurementList(float(sc["times"][k]), sc["scans"][k]), pruneSimilar=scene["on"][k])
            if streamed:
                continue
            st = trk.lastScanStats
            checks = [("gating", (st["L"], st["G"]) == (r["L"], r["G"])), ("unused", np.array_equal(st["unused"], r["unused"])),
                      ("ilps", r["n_ilp"] == trk.nOptimSolved)] + state_checks(r)
            if not all(c for _, c in checks):
                return False, 'MISMATCH at scan %d: %s' % (k, ', '.join(n for n, c in checks if not c))
        if streamed and rec["scans"]:
            log = trk.scanStatsLog
            checks = [("number of scans", len(log) == len(rec["scans"]))]
            for k, (s, r) in enumerate(zip(log, rec["scans"])):
                checks.append(("scan %d statistics" % k, (s["L"], s["G"], s["ilp"], s["nTargets"]) == (r["L"], r["G"], r["n_ilp"], len(r["ids"]))
                               and np.array_equal(s["unused"], r["unused"])))
            checks += state_checks(rec["scans"][-1])
            if not all(c for _, c in checks):
                return False, 'MISMATCH (streamed): %s' % ', '.join(n for n, c in checks if not c)
        return True, '%s%s%d scans %.1fs' % ('streamed ' if streamed else '', 'spill ' if spill else '', len(rec["scans"]), time.time() - t0)
    finally:
        trk.close()


def run_case_ca(seed, max_leaves=1500, similar=False, streamed=False):
    """The linear six-state forest on scenario_of(seed) with random acceleration tails against the live oracle (oracle_run, device_run).
    Returns (ok, description, message, census)."""
    scene = ca_scene(seed, similar)
    rec = oracle_run(scene, max_leaves)
    ok, msg = device_run(scene, rec, streamed)
    c = rec["census"]
    return ok, scene["desc"], msg + ' L=%d ilp=%d cluster=%d dead=%d groups=%s' % (c["L"], c["ilp"], c["cluster"], c["dead"], group_histogram(c["groups"])), c


def add_census(total, c):
    """Census of a slice: sums of the ILPs and terminations, maxima of the cluster size and L, all group sizes."""
    total["ilp"] = total.get("ilp", 0) + c["ilp"]
    total["dead"] = total.get("dead", 0) + c["dead"]
    total["cluster"] = max(total.get("cluster", 0), c["cluster"])
    total["L"] = max(total.get("L", 0), c["L"])
    total.setdefault("groups", []).extend(c["groups"])
    if "grow" in c:      # (constant-turn scenes: every (target, scan) figure, the turn-rate kinds met)
        total.setdefault("grow", []).extend(g for _, _, g in ct_grow_rows(c))
        total["kinds"] = sorted(set(total.get("kinds", [])) | set(c["kinds"]))
    return total


def run_case_ct_scene(seed, max_leaves=CA_MAX_LEAVES, similar=False, streamed=False, spill=False):
    """The constant-turn forest on scenario_of(seed) with run_case_ct's random turn rates, the leaf cap alone deciding where it stops
    (oracle_run, device_run).  Returns (ok, description, message, census)."""
    scene = ct_scene(seed, similar)
    rec = oracle_run(scene, max_leaves)
    ok, msg = device_run(scene, rec, streamed, spill)
    c = rec["census"]
    return ok, scene["desc"], msg + ' L=%d ilp=%d cluster=%d dead=%d groups=%s' % (c["L"], c["ilp"], c["cluster"], c["dead"], group_histogram(c["groups"])), c
