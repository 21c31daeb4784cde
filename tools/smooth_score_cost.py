"""What scoring track histories costs next to smoothing them, and what the EM trace adds to EM, in ONE process (sibling of
tools/smooth_cost.py and tools/smooth_em_cost.py, same batches).

  python tools/smooth_score_cost.py [--out FILE]      (default FILE: profiles/smooth_score_cost.txt)
      for 500 tracks x 200 nodes (models/pv, 4-state build) and 2 000 x 400 (models/ca, 6-state build), 80 % detections, T = 2.5:
        the seams' own times -- mht_score_tracks against mht_smooth_tracks with covariances, and mht_smooth_tracks_em_ll against
        mht_smooth_tracks_em at n_iter = 5 -- each timed around the library call (copy of the lengths, the launches, the wait),
        3 warm-up calls, then 20 calls of each, alternating: median, min, max, and the ratio of the medians
        accuracy ratios of the batches of tests/test_smooth_score_gpu.py
        registers of the score kernels, from the compiler's report (where hipcc is there)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

PERIOD = 2.5
SIZES = {"pv": (500, 200, 4), "ca": (2000, 400, 6)}
N_ITER, WARM, REPS = 5, 3, 20


def timed_seam(lib, name, sink):
    fn = getattr(lib, name)

    def call(*args):
        t0 = time.perf_counter()
        rc = fn(*args)      # (synchronises before it returns)
        sink.append(time.perf_counter() - t0)
        return rc
    setattr(lib, name, call)
    return fn


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def main(out_path):
    import torch
    import smooth_ais_ref as ar
    import smooth_ref as sr
    import smooth_score_ref as ref
    from pymht_amd.device import Context
    from pymht_amd.models import pv, ca, ct
    from pymht_amd.smoothing import score_tracks, score_tracks_ais, score_tracks_ct, smooth_tracks, smooth_tracks_em
    assert torch.cuda.is_available(), "no GPU"
    lines = ["Score of track histories (mht_score_tracks: forward pass only, nothing stored per node) next to the linear smoother",
             "(mht_smooth_tracks, with covariances), and the EM trace (mht_smooth_tracks_em_ll) next to EM (mht_smooth_tracks_em), n_iter = %d," % N_ITER,
             "ONE process.  Times are the seams' own (copy of the lengths, the launches, the wait), %d warm-up calls, then %d calls of each," % (WARM, REPS),
             "alternating.  Expectation from the code: a score well under one smoother call; the trace adds n_iter + 1 = %d score launches." % (N_ITER + 1), ""]
    for name, model in (("pv", pv), ("ca", ca)):
        n, L, nx = SIZES[name]
        tracks = sr.make_batch(model, PERIOD, [L] * n, seed=7, p_detect=0.8)
        ctx = Context(0, nx=nx)
        try:
            sinks = {s: [] for s in ("mht_score_tracks", "mht_smooth_tracks", "mht_smooth_tracks_em", "mht_smooth_tracks_em_ll")}
            saved = {s: timed_seam(ctx.lib, s, sink) for s, sink in sinks.items()}
            try:
                for _ in range(WARM + REPS):
                    score_tracks(model, PERIOD, tracks, ctx=ctx)
                    smooth_tracks(model, PERIOD, tracks, ctx=ctx)
                    smooth_tracks_em(model, PERIOD, tracks, n_iter=N_ITER, ctx=ctx)
                    smooth_tracks_em(model, PERIOD, tracks, n_iter=N_ITER, ctx=ctx, likelihoods=True)
            finally:
                for s, fn in saved.items():
                    setattr(ctx.lib, s, fn)
            st = {s: stats(t) for s, t in sinks.items()}
            lines.append("models/%s, %d tracks x %d nodes, %d-state build (ms: median  min  max)" % (name, n, L, nx))
            for s in sinks:
                lines.append("  %-26s %9.3f %9.3f %9.3f" % ((s,) + st[s]))
            lines.append("  score / smoother (medians)            %.3f" % (st["mht_score_tracks"][0] / st["mht_smooth_tracks"][0]))
            extra = st["mht_smooth_tracks_em_ll"][0] - st["mht_smooth_tracks_em"][0]
            lines.append("  EM with trace / EM (medians)          %.3f   (the trace adds %.3f ms = %.2f score calls' worth; %d launches)"
                         % (st["mht_smooth_tracks_em_ll"][0] / st["mht_smooth_tracks_em"][0], extra, extra / st["mht_score_tracks"][0], N_ITER + 1))
            lines.append("")
        finally:
            ctx.close()
    lines.append("Accuracy, ratios e_dev / max(e_np, eps64) against the np.longdouble reference (tests/smooth_score_ref.py), criterion <= 8:")
    for lib_nx in (4, 6):
        ctx = Context(0, nx=lib_nx)
        try:
            for kind, model, score, names in (("linear", pv, score_tracks, ("ll", "nis")), ("linear", ca, score_tracks, ("ll", "nis")),
                                              ("ct", ct, score_tracks_ct, ("ll", "nis")), ("ais", pv, score_tracks_ais, ("ll", "nis", "nis_ais"))):
                tracks, truth, f64 = ref.reference(kind, model, PERIOD)
                got = [dict(zip(("ll", "nis", "nobs", "nis_ais", "nais"), d)) for d in score(model, PERIOD, tracks, ctx=ctx)]
                res = ref.ratios(got, truth, f64, names)
                lines.append("  %-6s models/%-3s %d-state build: " % (kind, model.__name__.split(".")[-1], lib_nx)
                             + " | ".join("%s e_dev %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
            for name, model in (("pv", pv), ("ca", ca)):
                for start in ("model", "reference"):
                    tracks, truth, f64 = ref.trace_reference(model, PERIOD, start)
                    got = [t[4] for t in smooth_tracks_em(model, PERIOD, tracks, n_iter=N_ITER, start=start, ctx=ctx, likelihoods=True)]
                    rows = ref.trace_ratios(got, truth, f64)
                    lines.append("  trace  models/%-3s start=%-9s %d-state build, rows 0 .. %d ratio: " % (name, start, lib_nx, N_ITER)
                                 + " ".join("%.3g" % r[2] for r in rows) + "   (e_np %.3g .. %.3g)" % (min(r[1] for r in rows), max(r[1] for r in rows)))
        finally:
            ctx.close()
    lines.append("")
    try:
        import pathlib
        import tempfile
        import test_smooth_score_resources as res
        found = res.score_report(pathlib.Path(tempfile.mkdtemp()), [])
        lines.append("Registers of the score kernels (compiler's report, gfx950, the library's flags):")
        for k, v in sorted(found.items()):
            lines.append("  %-90s VGPR %3d  AGPR %3d  scratch %d B  LDS %d B  VGPRs spilled %d" % (k, v["vgpr"], v["agpr"], v["scratch"], v["lds"], v["spill"]))
    except BaseException as exc:      # (no hipcc on this machine, or pytest's skip for the same reason)
        lines.append("Registers of the score kernels: the compiler's report could not be made here (%s)" % type(exc).__name__)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "smooth_score_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
