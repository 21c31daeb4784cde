"""What a likelihood surface costs in one launch next to one score call per candidate, in ONE process (sibling of
tools/smooth_score_cost.py, same batches).

  python tools/smooth_score_grid_cost.py [--out FILE]      (default FILE: profiles/smooth_score_grid_cost.txt)
      for 500 tracks x 200 nodes (models/pv, 4-state build) and 2 000 x 400 (models/ca, 6-state build), 80 % detections, T = 2.5,
      packed and uploaded ONCE (smoothing._pack), the seams' own times, a host clock around library calls that end in a wait on the stream:
        one mht_score_tracks_grid call at G = 64 (an 8 x 8 grid of scalings)   against   64 successive mht_score_tracks calls
        one mht_score_tracks_grid call at G = 1                                against   one mht_score_tracks call
      3 warm-up rounds, then 20 rounds of the four, alternating: median, min, max and the ratios of the medians.  The 64 plain calls
      all carry the batch's own model: a call's time does not depend on the values of Q and R.  What the Python layer saves on top
      (one stand-in model, one packing and one upload a candidate) is not in these figures.
      Row 27 of the grid (both scales 1) is compared with the plain call's output, bit for bit, at the sizes timed."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

PERIOD = 2.5
SIZES = {"pv": (500, 200, 4), "ca": (2000, 400, 6)}
SCALES = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
G, WARM, REPS = 64, 3, 20


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def main(out_path):
    import torch
    import smooth_ref as sr
    from pymht_amd import _lib
    from pymht_amd.device import Context
    from pymht_amd.models import pv, ca
    from pymht_amd.smoothing import _model_x, _pack, noise_grid
    assert torch.cuda.is_available(), "no GPU"
    lines = ["Likelihood surface in one launch (mht_score_tracks_grid: one (track, candidate) per lane, ceil(n / 64) x G workgroups) next to one",
             "mht_score_tracks call per candidate (ceil(n / 64) workgroups each), on ONE packed batch, ONE process.  Times are the seams' own",
             "(copy of the lengths and, for the grid, of the table; the launch; the wait), host clock, %d warm-up rounds, then %d rounds," % (WARM, REPS),
             "alternating; ms: median  min  max.", ""]
    for name, model in (("pv", pv), ("ca", ca)):
        n, L, nx = SIZES[name]
        tracks = sr.make_batch(model, PERIOD, [L] * n, seed=7, p_detect=0.8)
        ctx = Context(0, nx=nx)
        try:
            lib, dev = ctx.lib, ctx.device
            lens, order, L_max, hp, (x_d, P_d, z_d, h_d) = _pack(ctx, tracks, nx)
            Q, R = noise_grid(model, PERIOD, SCALES, SCALES)
            Q, R = np.ascontiguousarray(Q), np.ascontiguousarray(R)
            one = SCALES.index(1.0) * len(SCALES) + SCALES.index(1.0)
            Q1, R1 = np.ascontiguousarray(Q[one:one + 1]), np.ascontiguousarray(R[one:one + 1])
            mx, keep = _model_x(model, PERIOD, nx, False)
            lens_sorted = np.ascontiguousarray(lens[order])
            ll_g, nis_g = (torch.empty((G, n), dtype=torch.float64, device=dev) for _ in range(2))
            ll_p, nis_p = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
            nobs_g, nobs_p = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
            need_g, need_p = int(lib.mht_score_grid_work_bytes(nx, n, L_max, G)), int(lib.mht_score_work_bytes(nx, n, L_max))
            work = torch.empty(max(need_g, need_p), dtype=torch.uint8, device=dev)
            head = (ctx.handle, C.byref(mx), n, L_max, lens_sorted.ctypes.data_as(C.c_void_p), x_d.data_ptr(), P_d.data_ptr(), z_d.data_ptr(), h_d.data_ptr())

            def grid(g, q, r):
                _lib.check(lib.mht_score_tracks_grid(*head, g, q.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), ll_g.data_ptr(),
                                                     nis_g.data_ptr(), nobs_g.data_ptr(), work.data_ptr(), need_g), lib)

            def plain(times):
                for _ in range(times):
                    _lib.check(lib.mht_score_tracks(*head, ll_p.data_ptr(), nis_p.data_ptr(), nobs_p.data_ptr(), work.data_ptr(), need_p), lib)
            runs = {"grid, G = 64": lambda: grid(G, Q, R), "64 plain calls": lambda: plain(G), "grid, G = 1": lambda: grid(1, Q1, R1),
                    "1 plain call": lambda: plain(1)}
            sinks = {k: [] for k in runs}
            torch.cuda.synchronize(dev)
            for _ in range(WARM + REPS):
                for k, run in runs.items():
                    t0 = time.perf_counter()
                    run()      # (every seam waits for its stream before it returns)
                    sinks[k].append(time.perf_counter() - t0)
            grid(G, Q, R)
            plain(1)
            torch.cuda.synchronize(dev)
            same = bool(torch.equal(ll_g[one], ll_p)) and bool(torch.equal(nis_g[one], nis_p)) and bool(torch.equal(nobs_g, nobs_p))
            st = {k: stats(t) for k, t in sinks.items()}
            lines.append("models/%s, %d tracks x %d nodes, %d-state build: %d workgroups a candidate, %d with G = 64" % (name, n, L, nx, (n + 63) // 64, (n + 63) // 64 * G))
            for k in runs:
                lines.append("  %-18s %9.3f %9.3f %9.3f" % ((k,) + st[k]))
            lines.append("  grid (G = 64) / 64 plain calls (medians)   %.4f   (%.1f x)" % (st["grid, G = 64"][0] / st["64 plain calls"][0], st["64 plain calls"][0] / st["grid, G = 64"][0]))
            lines.append("  grid (G = 64) / 1 plain call (medians)     %.3f   (what 63 further candidates cost on top of one)" % (st["grid, G = 64"][0] / st["1 plain call"][0]))
            lines.append("  grid (G = 1) / 1 plain call (medians)      %.3f" % (st["grid, G = 1"][0] / st["1 plain call"][0]))
            lines.append("  row of scale (1, 1) against the plain call, ll, nis and nObs bit for bit: %s" % ("equal" if same else "DIFFERENT"))
            lines.append("")
            assert same
        finally:
            ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "smooth_score_grid_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
