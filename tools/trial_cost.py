"""What a grid of trial manoeuvres costs on the device in one call, next to what a caller had to do without it -- one mht_encounters
call per candidate -- and next to the NumPy reference, in ONE process (sibling of tools/encounter_cost.py).

  python tools/trial_cost.py [--out FILE]      (default FILE: profiles/trial_cost.txt)
      for 500 tracks (models/pv, 4-state build) and 2 000 tracks (models/ca, 6-state build), K = 24 steps of 2.5 s, R = 80 m, on one
      packed batch each:
        one mht_trial_manoeuvres call at G = 64 (16 course changes x 4 speed factors after 10 s, w = 0.05 rad/s): four launches, the
          tracks propagated once
        64 successive mht_encounters(first = 1) calls on the same tracks with the own ship as entry 0: 128 launches, the tracks
          propagated 64 times (a straight-line own state; a turn cannot be expressed that way, the cost is the same)
      timed around the library calls, 3 warm-up rounds, then 20 rounds that alternate between the two: medians, min, max, the ratio of
      the medians; the float64 NumPy reference (tests/trial_ref.py) on the first 4 candidates, scaled to 64
      accuracy ratios of the mpmath case of tests/test_trial_gpu.py
      registers of the kernels, from the compiler's report (where hipcc is there)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

DT, STEPS, RADIUS, TURN_RATE, DELAY = 2.5, 24, 80.0, 0.05, 10.0
SIZES = {"pv": (500, 4, 2000.0), "ca": (2000, 6, 8000.0)}      # tracks, states, half-width of the square they are spread over [m]
WARM, REPS = 3, 20
REF_CANDIDATES = 4      # candidates the NumPy reference is timed on
OWN = np.array([0.0, 0.0, 6.0, 3.0])
OWN_COV = np.array([9.0, 2.0, 16.0])


def candidates():
    """16 course changes over +-60 degrees x 4 speed factors, all after DELAY seconds: [64, 3]"""
    return np.array([[a, f, DELAY] for a in np.linspace(-np.pi / 3, np.pi / 3, 16) for f in (1.0, 0.75, 0.5, 0.25)])


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def time_both(ctx, x, P, Phi, Q, cand):
    """WARM + REPS rounds, each one mht_trial_manoeuvres call and then len(cand) mht_encounters(first = 1) calls on the same tracks:
    ([seconds per trial call], [seconds per run of encounter calls], out [5, G, n], summary [4, G])"""
    import torch
    import encounter_ref as eref
    from pymht_amd import _lib
    lib, dev = ctx.lib, ctx.device
    n, nx = x.shape
    G = len(cand)
    xp, Pp = eref.pack(x, P)
    x_d, P_d = torch.from_numpy(xp).to(dev), torch.from_numpy(Pp).to(dev)
    xo, Po = np.zeros(nx), np.zeros((nx, nx))
    xo[:4] = OWN
    Po[0, 0], Po[0, 1], Po[1, 0], Po[1, 1] = OWN_COV[0], OWN_COV[1], OWN_COV[1], OWN_COV[2]
    xe, Pe = eref.pack(np.vstack([xo, x]), np.concatenate([Po[None], P]))
    xe_d, Pe_d = torch.from_numpy(xe).to(dev), torch.from_numpy(Pe).to(dev)
    need_t, need_e = int(lib.mht_trial_work_bytes(n, G, STEPS)), int(lib.mht_encounter_work_bytes(n + 1, STEPS))
    work_t, work_e = torch.empty(need_t, dtype=torch.uint8, device=dev), torch.empty(need_e, dtype=torch.uint8, device=dev)
    out, summary = torch.empty((5, G, n), dtype=torch.float64, device=dev), torch.empty((4, G), dtype=torch.float64, device=dev)
    row = torch.empty((5, 1, n + 1), dtype=torch.float64, device=dev)
    Phi, Q, cand = np.ascontiguousarray(Phi), np.ascontiguousarray(Q), np.ascontiguousarray(cand)
    torch.cuda.synchronize(dev)
    t_trial, t_enc = [], []
    for _ in range(WARM + REPS):
        t0 = time.perf_counter()
        rc = lib.mht_trial_manoeuvres(ctx.handle, nx, n, G, STEPS, DT, RADIUS, Phi.ctypes.data, Q.ctypes.data, x_d.data_ptr(), P_d.data_ptr(), OWN.ctypes.data,
                                      OWN_COV.ctypes.data, TURN_RATE, cand.ctypes.data, out.data_ptr(), summary.data_ptr(), work_t.data_ptr(), need_t)      # (synchronises)
        t_trial.append(time.perf_counter() - t0)
        _lib.check(rc, lib)
        t0 = time.perf_counter()
        for _g in range(G):
            rc = lib.mht_encounters(ctx.handle, nx, n + 1, 1, STEPS, DT, RADIUS, Phi.ctypes.data, Q.ctypes.data, xe_d.data_ptr(), Pe_d.data_ptr(), row.data_ptr(),
                                    work_e.data_ptr(), need_e)      # (synchronises)
            if rc != 0:
                break
        t_enc.append(time.perf_counter() - t0)
        _lib.check(rc, lib)
    return t_trial, t_enc, out.cpu().numpy(), summary.cpu().numpy()


def main(out_path):
    import torch
    import encounter_ref as eref
    import trial_ref as ref
    from test_trial_cpu import DT as CASE_DT, mp_case
    from test_encounter_cpu import RADIUS as CASE_RADIUS
    from pymht_amd.device import Context
    from pymht_amd.models import ca, pv
    assert torch.cuda.is_available(), "no GPU"
    cand = candidates()
    G = len(cand)
    lines = ["Trial manoeuvres of the own ship (mht_trial_manoeuvres: the tracks propagated K steps once, one track per lane; the G candidates' paths in closed",
             "form, one per lane; one cell (candidate, track) per lane with mht_encounters' five figures and a fold per tile of 256 tracks; one wavefront per",
             "candidate over the tiles), K = %d steps of %.1f s, R = %.0f m, G = %d candidates (16 course changes over +-60 degrees x 4 speed factors after" % (STEPS, DT, RADIUS, G),
             "%.0f s, w = %.2f rad/s), against %d successive mht_encounters(first = 1) calls on the same tracks with the own ship as entry 0 -- what a caller" % (DELAY, TURN_RATE, G),
             "had to do before, and only for straight-line own states.  Times are the seams' own (launches and the wait), %d warm-up rounds, then %d rounds" % (WARM, REPS),
             "alternating between the two in one process.  The NumPy figure is the float64 reference (tests/trial_ref.py) on the first %d candidates, scaled" % REF_CANDIDATES,
             "to %d.  How many cells run the quadrature depends on the geometry -- the spread of the tracks is stated -- so the times are those of these" % G,
             "batches, not a rate.", ""]
    for name, model in (("pv", pv), ("ca", ca)):
        n, nx, spread = SIZES[name]
        x, P = eref.make_batch(model, n, seed=7, spread=spread)
        Phi, Q = eref.model_matrices(model, DT)
        ctx = Context(0, nx=nx)
        try:
            t_trial, t_enc, out, summary = time_both(ctx, x, P, Phi, Q, cand)
        finally:
            ctx.close()
        t0 = time.perf_counter()
        f64 = ref.manoeuvres(x, P, Phi, Q, STEPS, DT, RADIUS, OWN, OWN_COV, TURN_RATE, cand[:REF_CANDIDATES])
        t_np = time.perf_counter() - t0
        got = eref.seam_dict(out[:, :REF_CANDIDATES])
        same = all(np.array_equal(np.isnan(got[k]), np.isnan(f64[k])) for k in ref.NAMES)
        diff = max(float(np.nanmax(np.abs(got[k] - f64[k]) / (1 + np.abs(f64[k])))) for k in ref.NAMES if k != "tpc")
        want = ref.fold(out[3], out[1])
        folded = all(np.array_equal(summary[f], want[k].astype(np.float64), equal_nan=True) for f, k in enumerate(ref.SUMMARY))
        m_trial, m_enc = stats(t_trial), stats(t_enc)
        lines.append("models/%s, %d tracks over +-%.0f m, %d-state build: %d cells, %d of them with pc > 0 (ms: median  min  max)" % (name, n, spread, nx, G * n, int(np.sum(out[3] > 0))))
        lines.append("  %-44s %10.3f %10.3f %10.3f" % (("mht_trial_manoeuvres, G = %d, one call" % G,) + m_trial))
        lines.append("  %-44s %10.3f %10.3f %10.3f" % (("mht_encounters (first=1), %d calls" % G,) + m_enc))
        lines.append("  ratio of the medians, %d encounter calls / one trial call: %.2f" % (G, m_enc[0] / m_trial[0]))
        lines.append("  the summary is the NumPy fold of the device's table bit for bit: %s" % ("yes" if folded else "NO"))
        lines.append("  NumPy float64 reference: %.3f s for %d candidates, %.1f s scaled to %d; the device's rows against it: NaN cells %s, largest"
                     % (t_np, REF_CANDIDATES, t_np * G / REF_CANDIDATES, G, "the same" if same else "DIFFERENT"))
        lines.append("  |difference| / (1 + |reference|) over tcpa, dcpa, md2, pc %.3g" % diff)
        lines.append("")
    lines.append("Accuracy, ratios e_dev / max(e_np, eps64) against the truth (np.longdouble; pc: mpmath, 30 digits, the rule's 64 nodes), criterion <= 8,")
    lines.append("the mpmath case of tests/test_trial_gpu.py (52 tracks, 5 candidates, K = 3):")
    from test_trial_gpu import _raw
    for lib_nx in (4, 6):
        ctx = Context(0, nx=lib_nx)
        try:
            for N in (4, 6):
                x, P, own, Sown, Phi, Q, K, truth, f64, e_np = mp_case(N)
                rc, out, _ = _raw(ctx, x, P, Phi, Q, K, CASE_DT, CASE_RADIUS, own, Sown, ref.TURN_RATE, ref.CANDIDATES)
                assert rc == 0
                res = eref.ratios([eref.seam_dict(out)], [truth], [f64], [k for k in ref.NAMES if k != "tpc"])
                lines.append("  N %d, %d-state build: " % (N, lib_nx) + " | ".join("%s %.3g (e_np %.3g)" % (k, v[2], v[1]) for k, v in res.items()))
        finally:
            ctx.close()
    lines.append("")
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
        found = res.unit_report(pathlib.Path(tempfile.mkdtemp()), "mht_trial.hip", [])
        lines.append("Registers of the trial-manoeuvre kernels (compiler's report, gfx950, the library's flags):")
        for k, v in sorted(found.items()):
            lines.append("  %-80s VGPR %3d  AGPR %3d  scratch %d B  LDS %d B  VGPRs spilled %d" % (k, v["vgpr"], v["agpr"], v["scratch"], v["lds"], v["spill"]))
    except BaseException as exc:      # (no hipcc where the tool runs, or pytest's skip for the same reason)
        lines.append("Registers of the trial-manoeuvre kernels: the compiler's report could not be made here (%s)" % type(exc).__name__)
    return lines


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "trial_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
