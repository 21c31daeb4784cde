"""What tracing track histories costs next to scoring them and next to smoothing them, in ONE process (sibling of
tools/smooth_score_cost.py, same batches).

  python tools/smooth_trace_cost.py [--out FILE]      (default FILE: profiles/smooth_trace_cost.txt)
      for 500 tracks x 200 nodes (models/pv, 4-state build) and 2 000 x 400 (models/ca, 6-state build), 80 % detections, T = 2.5:
        ONE packed batch on the device, and on it the seams' own times -- mht_trace_tracks against mht_score_tracks and against
        mht_smooth_tracks with covariances -- each timed around the library call (copy of the lengths, the launch, the wait),
        3 warm-up rounds, then 20 rounds, the three calls alternating within a round: median, min, max, and the ratios of the medians
        accuracy ratios of the batches of tests/test_smooth_trace_gpu.py
        registers of the trace kernels, from the compiler's report (where hipcc is there)"""
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
WARM, REPS = 3, 20
SEAMS = ("mht_trace_tracks", "mht_score_tracks", "mht_smooth_tracks")


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def time_batch(ctx, model, tracks, nx):
    """The three seams on one packed batch: {seam: [seconds per call]}"""
    import torch
    from pymht_amd import _lib
    from pymht_amd.smoothing import _model_x, _pack
    lib, dev = ctx.lib, ctx.device
    n, ns = len(tracks), nx * (nx + 1) // 2
    lens, order, L_max, hp, (x_d, P_d, z_d, h_d) = _pack(ctx, tracks, nx)
    lens_sorted = np.ascontiguousarray(lens[order])
    mx, keep = _model_x(model, PERIOD, nx, False)
    new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
    outs = {"mht_trace_tracks": [new(L_max, 7, n)],
            "mht_score_tracks": [new(n), new(n), new(n, dtype=torch.int32)],
            "mht_smooth_tracks": [new(L_max, nx, n), new(L_max, ns, n)]}
    need = {"mht_trace_tracks": int(lib.mht_trace_work_bytes(nx, n, L_max)), "mht_score_tracks": int(lib.mht_score_work_bytes(nx, n, L_max)),
            "mht_smooth_tracks": int(lib.mht_smooth_work_bytes(nx, n, L_max))}
    work = {s: new(b, dtype=torch.uint8) for s, b in need.items()}
    torch.cuda.synchronize(dev)
    times = {s: [] for s in SEAMS}
    for _ in range(WARM + REPS):
        for s in SEAMS:
            t0 = time.perf_counter()
            rc = getattr(lib, s)(ctx.handle, C.byref(mx), n, L_max, lens_sorted.ctypes.data_as(C.c_void_p), x_d.data_ptr(), P_d.data_ptr(),
                                 z_d.data_ptr(), h_d.data_ptr(), *(o.data_ptr() for o in outs[s]), work[s].data_ptr(), need[s])      # (synchronises)
            times[s].append(time.perf_counter() - t0)
            _lib.check(rc, lib)
    return times, L_max, need


def main(out_path):
    import torch
    import smooth_ref as sr
    import smooth_trace_ref as ref
    from pymht_amd.device import Context
    from pymht_amd.models import pv, ca, ct
    from pymht_amd.smoothing import trace_tracks, trace_tracks_ais, trace_tracks_ct
    assert torch.cuda.is_available(), "no GPU"
    lines = ["Trace of track histories (mht_trace_tracks: the score's forward pass with v, S, nis and ll of every node stored, 7 doubles per node",
             "and lane, coalesced) next to the score (mht_score_tracks: the same pass, nothing stored per node) and next to the linear smoother",
             "(mht_smooth_tracks, with covariances: forward and backward, N + NS doubles per node in the workspace and again in the output), ONE",
             "process, ONE packed batch.  Times are the seams' own (copy of the lengths, the launch, the wait), %d warm-up rounds, then %d rounds," % (WARM, REPS),
             "the three calls alternating.  Expectation from the code: above the score, below the smoother.", ""]
    for name, model in (("pv", pv), ("ca", ca)):
        n, L, nx = SIZES[name]
        tracks = sr.make_batch(model, PERIOD, [L] * n, seed=7, p_detect=0.8)
        ctx = Context(0, nx=nx)
        try:
            times, L_max, need = time_batch(ctx, model, tracks, nx)
        finally:
            ctx.close()
        st = {s: stats(t) for s, t in times.items()}
        lines.append("models/%s, %d tracks x %d nodes, %d-state build (ms: median  min  max)" % (name, n, L, nx))
        for s in SEAMS:
            lines.append("  %-20s %9.3f %9.3f %9.3f" % ((s,) + st[s]))
        r_score, r_smooth = st["mht_trace_tracks"][0] / st["mht_score_tracks"][0], st["mht_trace_tracks"][0] / st["mht_smooth_tracks"][0]
        lines.append("  trace / score (medians)       %.3f" % r_score)
        lines.append("  trace / smoother (medians)    %.3f" % r_smooth)
        lines.append("  the trace writes %.1f MB, the smoother's workspace and outputs are %.1f MB" % (L_max * 7 * n * 8 / 1e6,
                                                                                                  (need["mht_smooth_tracks"] + L_max * (nx + nx * (nx + 1) // 2) * n * 8) / 1e6))
        lines.append("  as expected: above the score, below the smoother" if r_score > 1.0 and r_smooth < 1.0 else
                     "  NOT as expected (above the score: %s, below the smoother: %s)" % (r_score > 1.0, r_smooth < 1.0))
        lines.append("")
    lines.append("Accuracy, ratios e_dev / max(e_np, eps64) against the np.longdouble reference (tests/smooth_trace_ref.py), criterion <= 8:")
    for lib_nx in (4, 6):
        ctx = Context(0, nx=lib_nx)
        try:
            for kind, model, trace, names in (("linear", pv, trace_tracks, ref.RADAR), ("linear", ca, trace_tracks, ref.RADAR),
                                              ("ct", ct, trace_tracks_ct, ref.RADAR), ("ais", pv, trace_tracks_ais, ref.RADAR + ref.AIS)):
                tracks, truth, f64 = ref.reference(kind, model, PERIOD)
                res = ref.ratios(trace(model, PERIOD, tracks, ctx=ctx), truth, f64, names)
                lines.append("  %-6s models/%-3s %d-state build: " % (kind, model.__name__.split(".")[-1], lib_nx)
                             + " | ".join("%s %.3g (e_np %.3g)" % (k, v[2], v[1]) for k, v in res.items()))
        finally:
            ctx.close()
    lines.append("")
    try:
        import pathlib
        import tempfile
        import test_smooth_trace_resources as res
        found = res.trace_report(pathlib.Path(tempfile.mkdtemp()), [])
        lines.append("Registers of the trace kernels (compiler's report, gfx950, the library's flags):")
        for k, v in sorted(found.items()):
            lines.append("  %-90s VGPR %3d  AGPR %3d  scratch %d B  LDS %d B  VGPRs spilled %d" % (k, v["vgpr"], v["agpr"], v["scratch"], v["lds"], v["spill"]))
    except BaseException as exc:      # (no hipcc on this machine, or pytest's skip for the same reason)
        lines.append("Registers of the trace kernels: the compiler's report could not be made here (%s)" % type(exc).__name__)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "smooth_trace_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
