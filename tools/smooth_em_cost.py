"""What learning Q and R by EM costs next to the plain linear smoother, in ONE process (sibling of tools/smooth_cost.py, same batches).

  python tools/smooth_em_cost.py [--out FILE]      (default FILE: profiles/smooth_em_cost.txt)
      for 500 tracks x 200 nodes (models/pv) and 2 000 x 400 (models/ca), 80 % detections, T = 2.5:
        the seams' own times -- mht_smooth_tracks with covariances and mht_smooth_tracks_em at n_iter = 5 on the same batch, each timed
        around the library call (copy of the lengths, the launches, the wait), 3 warm-up calls, then 20 calls alternating between the
        two: median, min, max, and the ratio of the medians; the expectation from the code is n_iter + 1 = 6 walks plus the sums
        accuracy ratios of the batch of tests/test_smooth_em_gpu.py (both models, both starts, both builds)
        registers of the four smooth_em_kernel instances, from the compiler's report (where hipcc is there)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

PERIOD = 2.5
SIZES = {"pv": (500, 200), "ca": (2000, 400)}
N_ITER, WARM, REPS = 5, 3, 20


# Read from the compiler's report (-Rpass-analysis=kernel-resource-usage, gfx950, the library's flags) while the kernel was written; the
# variants are not in the tree, so the figures are kept here and written out with every run.
VARIANT_NOT_TAKEN = """Why a launch is ONE walk (the variants not taken, six states, compiler's report):
  one kernel looping over n_iter + 1 walks, theta in registers, learning switched off:   VGPR 256  AGPR 220  (476; the single walk: 256 + 94)
  the same with the M-step sums (Q, R per lane in registers, sums in the workspace):      VGPR 256  AGPR 256  scratch 780 B  194 VGPRs spilled
  the same with A, C and Q read from memory per step instead of from the arguments:       VGPR 256  AGPR 256  scratch 1520 B  444 VGPRs spilled
  one walk per launch, Q and R in registers across the walk:                               VGPR 256  AGPR 256  scratch 236 B  58 VGPRs spilled
  ... with Q, R, the sums and the parked state in the workspace, no scheduling fence:      VGPR 256  AGPR 256  scratch 12 B  2 VGPRs spilled
  ... with the fence between the backward step and the term's loads (what is built):      the registers above, no scratch
What the n_iter + 1 launches and the workspace round trips cost is the n_iter = 0 line above (one launch of the EM kernel against one
of the linear kernel, same arithmetic) and the per-walk share of the n_iter = 5 line."""


def timed_seam(lib, name, sink):
    fn = getattr(lib, name)

    def call(*args):
        t0 = time.perf_counter()
        rc = fn(*args)      # (synchronises before it returns)
        sink.append(time.perf_counter() - t0)
        return rc
    setattr(lib, name, call)
    return fn


def main(out_path):
    import torch
    import smooth_em_ref as er
    import smooth_ref as sr
    from pymht_amd.device import Context
    from pymht_amd.models import pv, ca
    from pymht_amd.smoothing import smooth_tracks, smooth_tracks_em
    assert torch.cuda.is_available(), "no GPU"
    lines = ["EM smoother (mht_smooth_tracks_em, n_iter = %d) next to the linear smoother (mht_smooth_tracks, with covariances), ONE process." % N_ITER,
             "Times are the seams' own (copy of the lengths, the launches -- one for the linear smoother, n_iter + 1 for EM -- and the wait), %d warm-up calls," % WARM,
             "then %d calls of each, alternating.  Expectation from the code: n_iter + 1 = %d walks plus the sums." % (REPS, N_ITER + 1), ""]
    for name, model in (("pv", pv), ("ca", ca)):
        n, L = SIZES[name]
        nx = int(np.asarray(model.C_RADAR).shape[1])
        tracks = sr.make_batch(model, PERIOD, [L] * n, seed=99, p_detect=0.8)
        ctx = Context(0, nx=nx)
        t_lin, t_em, t_em0 = [], [], []
        keep = [(s, timed_seam(ctx.lib, s, sink)) for s, sink in (("mht_smooth_tracks", t_lin), ("mht_smooth_tracks_em", t_em))]
        for k in range(WARM + REPS):
            smooth_tracks(model, PERIOD, tracks, ctx=ctx)
            out = smooth_tracks_em(model, PERIOD, tracks, n_iter=N_ITER, ctx=ctx)
            smooth_tracks_em(model, PERIOD, tracks, n_iter=0, ctx=ctx)
            t_em0.append(t_em.pop())
        for s, fn in keep:
            setattr(ctx.lib, s, fn)
        ctx.close()
        finite = sum(bool(np.isfinite(o[0]).all()) for o in out)
        a, b, c = np.array(t_lin[WARM:]) * 1e3, np.array(t_em[WARM:]) * 1e3, np.array(t_em0[WARM:]) * 1e3
        lines += ["models/%s, %d tracks x %d nodes (%d-state build); %d of %d tracks finite after EM" % (name, n, L, nx, finite, n),
                  "  mht_smooth_tracks      median %8.3f ms   min %8.3f   max %8.3f   (n = %d)" % (np.median(a), a.min(), a.max(), len(a)),
                  "  mht_smooth_tracks_em   median %8.3f ms   min %8.3f   max %8.3f   (n = %d)" % (np.median(b), b.min(), b.max(), len(b)),
                  "  ... with n_iter = 0    median %8.3f ms   min %8.3f   max %8.3f   (one launch, the linear smoother's arithmetic: %.2f of it)" % (np.median(c), c.min(), c.max(), np.median(c) / np.median(a)),
                  "  ratio of the medians   %.2f   (per walk: %.2f of the linear smoother's)" % (np.median(b) / np.median(a), np.median(b) / np.median(a) / (N_ITER + 1)), ""]
        print("\n".join(lines[-6:]), flush=True)
    lines += ["Accuracy, the batch of tests/test_smooth_em_gpu.py, n_iter = 5: e_dev / max(e_np, eps64) against the np.longdouble evaluation of",
              "tests/smooth_em_ref.py (the test asks for <= 8):"]
    for lib_nx in (4, 6):
        ctx = Context(0, nx=lib_nx)
        for name, model in (("pv", pv), ("ca", ca)):
            for start in ("model", "reference"):
                tracks, truth, f64 = er.accuracy_reference(model, PERIOD, start)
                dev = smooth_tracks_em(model, PERIOD, tracks, n_iter=N_ITER, start=start, ctx=ctx)
                res = er.ratios([dict(xs=d[0], Ps=d[1], Q=d[2], R=d[3]) for d in dev], truth, f64)
                lines.append("  %d-state build, models/%s, start=%-9s  " % (lib_nx, name, start)
                             + "  ".join("%s %.2f (e_np %.1e)" % (k, v[2], v[1]) for k, v in res.items()))
        ctx.close()
    lines.append("")
    import pytest
    try:
        import pathlib
        import tempfile
        from test_smooth_em_resources import em_report
        with tempfile.TemporaryDirectory() as d:
            found = em_report(pathlib.Path(d), [])
        lines.append("Registers (compiler's report; LAST = 0: a learning walk, LAST = 1: the walk that writes the output):")
        for k, r in sorted(found.items()):
            if "smooth_em_kernel" in k:
                lines.append("  %-28s VGPR %3d  AGPR %3d  scratch %d B  spilled %d  LDS %d B" % (k[k.index("smooth_"):k.index("E", k.index("ELb")) + 4], r["vgpr"], r["agpr"], r["scratch"], r["spill"], r["lds"]))
    except (Exception, pytest.skip.Exception) as e:      # (the report skips where there is no compiler)
        lines.append("Registers: not read here (%s)" % type(e).__name__)
    lines += ["", VARIANT_NOT_TAKEN]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "smooth_em_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
