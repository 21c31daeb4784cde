"""What the trial manoeuvres against every live hypothesis cost on the device in one call, next to the way the same numbers could be
reached before -- one mht_trial_manoeuvres call with the leaves as its tracks, the download of its [5][G][L] table and a NumPy segmented
fold on the host -- in ONE process (sibling of tools/trial_cost.py).

  python tools/trial_hyp_cost.py [--out FILE]      (default FILE: profiles/trial_hyp_cost.txt)
      for about 13 000 leaves over 500 targets (models/pv, 4-state build: the headline's shape) and about 100 000 leaves over 2 000
      targets (models/ca, 6-state build), G = 64 candidates, K = 24 steps of 2.5 s, R = 80 m, on one packed batch each:
        mht_trial_hypotheses with table = NULL: five launches, the figures [8][G][T] and the weights, no table anywhere
        mht_trial_hypotheses with the table
        mht_trial_manoeuvres (n = L), the table's download and the NumPy fold (vectorised: ufunc.reduceat over the segments)
      timed around the calls, 3 warm-up rounds, then 20 rounds that alternate between the three: medians, min, max, the ratio of the
      medians; the host fold's figures are held to the device's (extrema bit for bit, pcMean to 1e-12 relative)
      a Tracker over a scene of 500 targets: getHypothesisEncounters (the leaves as they are) next to getTrialManoeuvres (the
      best-hypothesis path with its walk over every history), 3 rounds each after one warm-up
      accuracy: the worst ratio to the bound of property 8 of tests/test_trial_hyp_gpu.py over its cases, both builds
      registers of the kernels, from the compiler's report (where hipcc is there)
      Without a device the file says NOT YET MEASURED and holds the register report alone."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

DT, STEPS, RADIUS, TURN_RATE, DELAY = 2.5, 24, 80.0, 0.05, 10.0
SIZES = {"pv": (13000, 500, 4, 8000.0), "ca": (100000, 2000, 6, 30000.0)}      # leaves, targets, states, half-width of the square [m]
WARM, REPS = 3, 20
OWN = np.array([0.0, 0.0, 6.0, 3.0])
OWN_COV = np.array([9.0, 2.0, 16.0])


def candidates():
    """16 course changes over +-60 degrees x 4 speed factors, all after DELAY seconds: [64, 3]"""
    return np.array([[a, f, DELAY] for a in np.linspace(-np.pi / 3, np.pi / 3, 16) for f in (1.0, 0.75, 0.5, 0.25)])


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def make_batch(model, L, T, spread, seed):
    """L leaves over T targets: a target's leaves are its state plus a scatter of 30 m and 1 m/s (the alternatives of a few scans), the
    segment sizes random (every target has a leaf), cnllr spread over 15 inside a target: (x, P, cnllr, seg, sel)"""
    import encounter_ref as eref
    rng = np.random.default_rng(seed)
    xt, Pt = eref.make_batch(model, max(T, 52), seed=seed, spread=spread)
    xt, Pt = xt[-T:], Pt[-T:]      # (without the special entries at the front)
    cuts = np.sort(rng.choice(np.arange(1, L), T - 1, replace=False))
    seg = np.concatenate([[0], cuts, [L]]).astype(np.int32)
    target = np.repeat(np.arange(T), np.diff(seg))
    x, P = xt[target].copy(), Pt[target].copy()
    x[:, :2] += rng.normal(0.0, 30.0, (L, 2))
    x[:, 2:4] += rng.normal(0.0, 1.0, (L, 2))
    cnllr = rng.uniform(0.0, 15.0, L) + rng.uniform(-40.0, 40.0, T)[target]
    sel = np.array([seg[t] + int(np.argmin(cnllr[seg[t]:seg[t + 1]])) for t in range(T)], dtype=np.int32)
    return x, P, cnllr, seg, sel


def host_fold(table, cnllr, seg, sel):
    """The NumPy segmented fold of a downloaded table [5, G, L] (every segment has a leaf): fig [8, G, T], vectorised over the segments"""
    tcpa, dcpa, pc = table[0], table[1], table[3]
    G, L = pc.shape
    start = seg[:-1].astype(np.intp)
    target = np.repeat(np.arange(len(start)), np.diff(seg))
    idx = np.arange(L)
    cmin = np.fmin.reduceat(cnllr, start)
    w = np.exp(-(cnllr - cmin[target]))
    fig = np.empty((8, G, len(start)))
    with np.errstate(invalid="ignore"):
        fig[0] = np.fmax.reduceat(pc, start, axis=1)
        fig[1] = np.minimum.reduceat(np.where(pc == fig[0][:, target], idx, L), start, axis=1)
        fig[2] = np.fmin.reduceat(dcpa, start, axis=1)
        fig[3] = np.minimum.reduceat(np.where(dcpa == fig[2][:, target], idx, L), start, axis=1)
        live = ~np.isnan(pc) & ~np.isnan(w)
        fig[4] = np.add.reduceat(np.where(live, w * pc, 0.0), start, axis=1) / np.add.reduceat(np.where(live, w, 0.0), start, axis=1)
    for f in (1, 3):
        fig[f][fig[f] == L] = -1
    fig[5], fig[6], fig[7] = pc[:, sel], dcpa[:, sel], tcpa[:, sel]
    return fig


def time_three(ctx, x, P, cnllr, seg, sel, Phi, Q, cand):
    """WARM + REPS rounds of: the new call without the table, the new call with it, and the old way (mht_trial_manoeuvres, download,
    host fold).  Returns the three lists of seconds, the device's fig [8, G, T] and the host fold's."""
    import torch
    import encounter_ref as eref
    from pymht_amd import _lib
    lib, dev = ctx.lib, ctx.device
    L, nx = x.shape
    G, T = len(cand), len(sel)
    xp, Pp = eref.pack(x, P)
    x_d, P_d, c_d = torch.from_numpy(xp).to(dev), torch.from_numpy(Pp).to(dev), torch.from_numpy(cnllr).to(dev)
    need_h, need_t = int(lib.mht_trial_hyp_work_bytes(L, T, G, STEPS)), int(lib.mht_trial_work_bytes(L, G, STEPS))
    work_h, work_t = torch.empty(need_h, dtype=torch.uint8, device=dev), torch.empty(need_t, dtype=torch.uint8, device=dev)
    table = torch.empty((5, G, L), dtype=torch.float64, device=dev)
    fig, weight = torch.empty((8, G, T), dtype=torch.float64, device=dev), torch.empty(L, dtype=torch.float64, device=dev)
    summary = torch.empty((4, G), dtype=torch.float64, device=dev)
    Phi, Q, cand = np.ascontiguousarray(Phi), np.ascontiguousarray(Q), np.ascontiguousarray(cand)
    torch.cuda.synchronize(dev)

    def hyp(tab):
        rc = lib.mht_trial_hypotheses(ctx.handle, nx, L, T, G, STEPS, DT, RADIUS, Phi.ctypes.data, Q.ctypes.data, x_d.data_ptr(), P_d.data_ptr(), c_d.data_ptr(),
                                      seg.ctypes.data, sel.ctypes.data, OWN.ctypes.data, OWN_COV.ctypes.data, TURN_RATE, cand.ctypes.data, tab, fig.data_ptr(),
                                      weight.data_ptr(), work_h.data_ptr(), need_h)      # (synchronises)
        _lib.check(rc, lib)
    t_bare, t_full, t_old = [], [], []
    for _ in range(WARM + REPS):
        t0 = time.perf_counter()
        hyp(None)
        got = fig.cpu().numpy()      # (the figures' download belongs to the call: [8][G][T])
        t_bare.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        hyp(table.data_ptr())
        t_full.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        rc = lib.mht_trial_manoeuvres(ctx.handle, nx, L, G, STEPS, DT, RADIUS, Phi.ctypes.data, Q.ctypes.data, x_d.data_ptr(), P_d.data_ptr(), OWN.ctypes.data,
                                      OWN_COV.ctypes.data, TURN_RATE, cand.ctypes.data, table.data_ptr(), summary.data_ptr(), work_t.data_ptr(), need_t)
        _lib.check(rc, lib)
        host = host_fold(table.cpu().numpy(), cnllr, seg, sel)
        t_old.append(time.perf_counter() - t0)
    return t_bare, t_full, t_old, got, host


def tracker_lines():
    """A Tracker over 500 targets and six scans with clutter: the two entry points on the same scene"""
    from pymht_amd.models import pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    from pymht_amd.utils.scenario import make_scenario
    sc = make_scenario(T=500, radius=1800.0, lambda_phi=3e-5, n_scans=6, P_d=0.85, seed=99)
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=3, eta2=5.99, useInitiator=False)
    try:
        for x0 in sc["x0"]:
            trk.initiateTarget(Target(sc["t0"], None, x0.copy(), pv.P0))
        for zk, tk in zip(sc["scans"], sc["times"]):
            trk.addMeasurementList(MeasurementList(float(tk), zk))
        n_leaves, n_targets = len(trk.leafBatch()["x"]), trk.nTargets
        dpsi, fs = np.linspace(-np.pi / 3, np.pi / 3, 16), (1.0, 0.75, 0.5, 0.25)
        calls = (("getHypothesisEncounters (the leaves as they are)", lambda: trk.getHypothesisEncounters(60.0, RADIUS, OWN, dpsi, TURN_RATE, speedFactors=fs, delay=DELAY)),
                 ("getTrialManoeuvres (re-filters every history)", lambda: trk.getTrialManoeuvres(60.0, RADIUS, OWN, dpsi, TURN_RATE, speedFactors=fs, delay=DELAY)))
        out = ["Tracker, models/pv, %d targets after %d scans with clutter, %d live leaves, G = 64, K = 24 (ms, host work included: median of 3 after a warm-up)"
               % (n_targets, len(sc["scans"]), n_leaves)]
        for label, call in calls:
            call()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            out.append("  %-52s %10.3f" % (label, float(np.median(ts)) * 1e3))
        return out + [""]
    finally:
        trk.close()


def accuracy_lines():
    import trial_ref
    from test_encounter_cpu import RADIUS as CASE_RADIUS
    from test_trial_hyp_cpu import CASES, DT as CASE_DT, check_figures, scene
    from test_trial_hyp_gpu import _raw
    from pymht_amd.device import Context
    out = ["Accuracy of pcMean and weight: the worst ratio of |device - truth| to (2 nLeaves + 64) eps truth + 2 eps, truth the np.longdouble fold of the",
           "device's own table and the input cnllr (property 8 of tests/test_trial_hyp_gpu.py, criterion <= 1), over that file's cases:"]
    for lib_nx in (4, 6):
        ctx = Context(0, nx=lib_nx)
        try:
            worst = [0.0, 0.0]
            for N, K, G, layout in CASES:
                x, P, cnllr, seg, sel, own, Sown, Phi, Q = scene(N, layout)
                rc, table, fig, weight, _ = _raw(ctx, x, P, cnllr, seg, sel, Phi, Q, K, CASE_DT, CASE_RADIUS, own, Sown, trial_ref.TURN_RATE, trial_ref.CANDIDATES[:G])
                assert rc == 0
                r = check_figures("N %d K %d G %d %s" % (N, K, G, layout), fig, weight, table, cnllr, seg, sel)
                worst = [max(a, b) for a, b in zip(worst, r)]
            out.append("  %d-state build: pcMean %.3g, weight %.3g" % (lib_nx, worst[0], worst[1]))
        finally:
            ctx.close()
    return out + [""]


def main(out_path):
    import encounter_ref as eref
    from pymht_amd.models import ca, pv
    cand = candidates()
    G = len(cand)
    lines = ["Trial manoeuvres against every live hypothesis (mht_trial_hypotheses: the weights, one target per lane; the L leaves propagated K steps once, one",
             "leaf per lane; the G candidates' paths, one per lane; one cell (candidate, leaf) per lane with a serial fold per piece of a target inside a tile of",
             "256 leaves; one lane per (candidate, target) over the pieces), K = %d steps of %.1f s, R = %.0f m, G = %d candidates (16 course changes over +-60" % (STEPS, DT, RADIUS, G),
             "degrees x 4 speed factors after %.0f s, w = %.2f rad/s), against the way the same figures could be reached before: mht_trial_manoeuvres with" % (DELAY, TURN_RATE),
             "the leaves as its tracks, the download of its [5][G][L] table, and a vectorised NumPy fold over the segments.  Times are around the calls (launches,",
             "the wait, and the download of what the caller reads), %d warm-up rounds, then %d rounds alternating between the three in one process." % (WARM, REPS), ""]
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        lines += ["NOT YET MEASURED on the device: no GPU was visible where this file was written; the register report below is the compiler's.", ""]
    else:
        from pymht_amd.device import Context
        for name, model in (("pv", pv), ("ca", ca)):
            L, T, nx, spread = SIZES[name]
            x, P, cnllr, seg, sel = make_batch(model, L, T, spread, seed=7)
            Phi, Q = eref.model_matrices(model, DT)
            ctx = Context(0, nx=nx)
            try:
                t_bare, t_full, t_old, got, host = time_three(ctx, x, P, cnllr, seg, sel, Phi, Q, cand)
            finally:
                ctx.close()
            exact = all(np.array_equal(got[f], host[f], equal_nan=True) for f in (0, 1, 2, 3, 5, 6, 7))
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = float(np.nanmax(np.abs(got[4] - host[4]) / np.maximum(np.abs(host[4]), 1e-300)))
            m_bare, m_full, m_old = stats(t_bare), stats(t_full), stats(t_old)
            lines.append("models/%s, %d leaves over %d targets (1 .. %d leaves a target) within +-%.0f m, %d-state build: %d cells, the table would be %.0f MB"
                         % (name, L, T, int(np.diff(seg).max()), spread, nx, G * L, 5 * G * L * 8 / 1e6))
            lines.append("  (ms: median  min  max)")
            lines.append("  %-58s %10.3f %10.3f %10.3f" % (("mht_trial_hypotheses, table = NULL, figures downloaded",) + m_bare))
            lines.append("  %-58s %10.3f %10.3f %10.3f" % (("mht_trial_hypotheses with the table (left on the device)",) + m_full))
            lines.append("  %-58s %10.3f %10.3f %10.3f" % (("mht_trial_manoeuvres (n = L) + download + NumPy fold",) + m_old))
            lines.append("  ratio of the medians, table plus host fold / the fused call: %.2f" % (m_old[0] / m_bare[0]))
            lines.append("  the host fold against the device's figures: extrema, leaves and Sel rows bit for bit: %s; pcMean largest relative difference %.3g"
                         % ("yes" if exact else "NO", rel))
            lines.append("")
        try:
            lines += tracker_lines()
        except Exception as exc:      # (the measurements above stand on their own)
            lines += ["Tracker scene: NOT MEASURED, it could not be run here (%s: %s)" % (type(exc).__name__, exc), ""]
        lines += accuracy_lines()
    lines += register_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


def register_lines():
    lines = []
    try:
        import pathlib
        import tempfile
        import test_filter_resources as res
        found = res.unit_report(pathlib.Path(tempfile.mkdtemp()), "mht_trial_hyp.hip", [])
        lines.append("Registers of the hypothesis kernels (compiler's report, gfx950, the library's flags):")
        for k, v in sorted(found.items()):
            lines.append("  %-80s VGPR %3d  AGPR %3d  scratch %d B  LDS %d B  VGPRs spilled %d" % (k, v["vgpr"], v["agpr"], v["scratch"], v["lds"], v["spill"]))
    except BaseException as exc:      # (no hipcc where the tool runs, or pytest's skip for the same reason)
        lines.append("Registers of the hypothesis kernels: the compiler's report could not be made here (%s)" % type(exc).__name__)
    return lines


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "trial_hyp_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
