"""What predicting the encounters of the live tracks costs on the device, next to the NumPy reference, in ONE process (sibling of
tools/nees_cost.py).

  python tools/encounter_cost.py [--out FILE]      (default FILE: profiles/encounter_cost.txt)
      for 500 entries (models/pv, 4-state build) and 2 000 entries (models/ca, 6-state build; BASELINE config 5's live tracks),
      K = 24 steps of 2.5 s, R = 80 m: the seam's own time of mht_encounters for all pairs (first = n) and for the own ship against
        everyone (first = 1) -- timed around the library call (the two launches and the wait), 3 warm-up rounds, then 10 rounds:
        median, min, max -- and the float64 NumPy reference (tests/encounter_ref.py) on a subsample of the rows, scaled to all pairs
      accuracy ratios of the cases of tests/test_encounter_gpu.py
      registers of the kernels, from the compiler's report (where hipcc is there)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

DT, STEPS, RADIUS = 2.5, 24, 80.0
SIZES = {"pv": (500, 4, 2000.0), "ca": (2000, 6, 8000.0)}      # entries, states, half-width of the square they are spread over [m]
WARM, REPS = 3, 10
REF_ROWS = 4      # rows of the table the NumPy reference is timed on


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def time_seam(ctx, x, P, Phi, Q, first):
    """mht_encounters on one batch on the device: ([seconds per call], out [5, first, n])"""
    import torch
    import encounter_ref as ref
    from pymht_amd import _lib
    lib, dev = ctx.lib, ctx.device
    n, nx = x.shape
    xp, Pp = ref.pack(x, P)
    x_d, P_d = torch.from_numpy(xp).to(dev), torch.from_numpy(Pp).to(dev)
    need = int(lib.mht_encounter_work_bytes(n, STEPS))
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty((5, first, n), dtype=torch.float64, device=dev)
    Phi, Q = np.ascontiguousarray(Phi), np.ascontiguousarray(Q)
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(WARM + REPS):
        t0 = time.perf_counter()
        rc = lib.mht_encounters(ctx.handle, nx, n, first, STEPS, DT, RADIUS, Phi.ctypes.data, Q.ctypes.data, x_d.data_ptr(), P_d.data_ptr(),
                                out.data_ptr(), work.data_ptr(), need)      # (synchronises)
        ts.append(time.perf_counter() - t0)
        _lib.check(rc, lib)
    return ts, out.cpu().numpy()


def main(out_path):
    import torch
    import encounter_ref as ref
    from test_encounter_cpu import N_ENTRIES, pc_case
    from pymht_amd.device import Context
    from pymht_amd.models import ca, pv
    assert torch.cuda.is_available(), "no GPU"
    lines = ["Encounters of the live tracks (mht_encounters: every entry propagated K steps with the model's Phi and Q, one entry per lane; then one",
             "cell (i, j) per lane: the closest point of approach, the smallest Mahalanobis distance and the largest probability of being within R,",
             "pc_k by the 64-node rule of csrc/mht_encounter.h wherever the 8-sigma clip does not make it 0), K = %d steps of %.1f s, R = %.0f m." % (STEPS, DT, RADIUS),
             "Times are the seam's own (two launches and the wait), %d warm-up rounds, then %d rounds.  The NumPy figure is the float64 reference" % (WARM, REPS),
             "(tests/encounter_ref.py) on the first %d rows of the table, scaled by the pairs.  How many cells run the quadrature depends on the" % REF_ROWS,
             "geometry -- the spread of the entries is stated -- so the times are those of these batches, not a rate.", ""]
    for name, model in (("pv", pv), ("ca", ca)):
        n, nx, spread = SIZES[name]
        x, P = ref.make_batch(model, n, seed=7, spread=spread)
        Phi, Q = ref.model_matrices(model, DT)
        ctx = Context(0, nx=nx)
        try:
            t_all, out = time_seam(ctx, x, P, Phi, Q, n)
            t_own, _ = time_seam(ctx, x, P, Phi, Q, 1)
        finally:
            ctx.close()
        t0 = time.perf_counter()
        f64 = ref.encounters(x, P, Phi, Q, STEPS, DT, RADIUS, first=REF_ROWS)
        t_np = time.perf_counter() - t0
        pairs, ref_pairs = n * (n - 1) // 2, sum(n - 1 - i for i in range(REF_ROWS))
        got = ref.seam_dict(out[:, :REF_ROWS])
        same = all(np.array_equal(np.isnan(got[k]), np.isnan(f64[k])) for k in ref.NAMES)
        diff = max(float(np.nanmax(np.abs(got[k] - f64[k]) / (1 + np.abs(f64[k])))) for k in ref.NAMES if k != "tpc")
        live = int(np.sum(out[3] > 0))
        lines.append("models/%s, %d entries over +-%.0f m, %d-state build: %d pairs, %d of them with pc > 0 (ms: median  min  max)" % (name, n, spread, nx, pairs, live))
        lines.append("  %-34s %10.3f %10.3f %10.3f" % (("mht_encounters, all pairs",) + stats(t_all)))
        lines.append("  %-34s %10.3f %10.3f %10.3f" % (("mht_encounters, own ship (first=1)",) + stats(t_own)))
        lines.append("  NumPy float64 reference: %.3f s for %d pairs, %.1f s scaled to all pairs; the device's rows against it: NaN cells %s, largest"
                     % (t_np, ref_pairs, t_np * pairs / ref_pairs, "the same" if same else "DIFFERENT"))
        lines.append("  |difference| / (1 + |reference|) over tcpa, dcpa, md2, pc %.3g" % diff)
        lines.append("")
    lines.append("Accuracy, ratios e_dev / max(e_np, eps64) against the truth (np.longdouble; pc: mpmath, 30 digits, the rule's 64 nodes), criterion <= 8,")
    lines.append("the mpmath case of tests/test_encounter_gpu.py (first = 4 of %d entries, K = 4):" % N_ENTRIES)
    from test_encounter_gpu import _raw
    for lib_nx in (4, 6):
        ctx = Context(0, nx=lib_nx)
        try:
            for N in (4, 6):
                x, P, Phi, Q, K, dt, truth, f64, e_np = pc_case(N)
                rc, out = _raw(ctx, x, P, Phi, Q, K, dt, RADIUS, first=4)
                assert rc == 0
                res = ref.ratios([ref.seam_dict(out)], [truth], [f64], [k for k in ref.NAMES if k != "tpc"])
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
        found = res.unit_report(pathlib.Path(tempfile.mkdtemp()), "mht_encounter.hip", [])
        lines.append("Registers of the encounter kernels (compiler's report, gfx950, the library's flags):")
        for k, v in sorted(found.items()):
            lines.append("  %-80s VGPR %3d  AGPR %3d  scratch %d B  LDS %d B  VGPRs spilled %d" % (k, v["vgpr"], v["agpr"], v["scratch"], v["lds"], v["spill"]))
    except BaseException as exc:      # (no hipcc on this machine, or pytest's skip for the same reason)
        lines.append("Registers of the encounter kernels: the compiler's report could not be made here (%s)" % type(exc).__name__)
    return lines


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "encounter_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
