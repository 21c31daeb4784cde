"""What handing out the filtered states of track histories costs next to scoring and next to smoothing them, and what the NEES launch
on top costs next to the bytes it moves, in ONE process (sibling of tools/smooth_trace_cost.py, same batches).

  python tools/nees_cost.py [--out FILE]      (default FILE: profiles/nees_cost.txt)
      for 500 tracks x 200 nodes (models/pv, 4-state build) and 2 000 x 400 (models/ca, 6-state build), 80 % detections, T = 2.5:
        ONE packed batch on the device, and on it the seams' own times -- mht_filter_tracks against mht_score_tracks and against
        mht_smooth_tracks with covariances, and mht_nees_nodes (D = nx, every cell present) on the filter's outputs where they lie --
        each timed around the library call (copy of the lengths, the launch, the wait), 3 warm-up rounds, then 20 rounds, the four
        calls alternating within a round: median, min, max, the ratios of the medians, and the NEES launch's bytes per second
        accuracy ratios of the batches of tests/test_filter_gpu.py and of the cells of tests/test_nees_gpu.py
        registers of the filter and NEES kernels, from the compiler's report (where hipcc is there)"""
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
SEAMS = ("mht_filter_tracks", "mht_score_tracks", "mht_smooth_tracks", "mht_nees_nodes")


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def nees_bytes(nx, cells):
    """What mht_nees_nodes moves at D = nx: x, truth, the packed P and the flag in, nx + 3 figures out"""
    return cells * ((2 * nx + nx * (nx + 1) // 2 + nx + 3) * 8 + 1)


def time_batch(ctx, model, tracks, nx):
    """The four seams on one packed batch: {seam: [seconds per call]}"""
    import torch
    from pymht_amd import _lib
    from pymht_amd.smoothing import _model_x, _pack
    lib, dev = ctx.lib, ctx.device
    n, ns = len(tracks), nx * (nx + 1) // 2
    lens, order, L_max, hp, (x_d, P_d, z_d, h_d) = _pack(ctx, tracks, nx)
    lens_sorted = np.ascontiguousarray(lens[order])
    mx, keep = _model_x(model, PERIOD, nx, False)
    new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
    outs = {"mht_filter_tracks": [new(L_max, nx, n), new(L_max, ns, n)],
            "mht_score_tracks": [new(n), new(n), new(n, dtype=torch.int32)],
            "mht_smooth_tracks": [new(L_max, nx, n), new(L_max, ns, n)]}
    need = {"mht_filter_tracks": int(lib.mht_filter_work_bytes(nx, n, L_max)), "mht_score_tracks": int(lib.mht_score_work_bytes(nx, n, L_max)),
            "mht_smooth_tracks": int(lib.mht_smooth_work_bytes(nx, n, L_max))}
    work = {s: new(b, dtype=torch.uint8) for s, b in need.items()}
    truth = torch.zeros((L_max, nx, n), dtype=torch.float64, device=dev)
    present = torch.ones((L_max, n), dtype=torch.uint8, device=dev)
    nees_out = new(L_max, nx + 3, n)
    torch.cuda.synchronize(dev)
    times = {s: [] for s in SEAMS}
    for _ in range(WARM + REPS):
        for s in SEAMS:
            t0 = time.perf_counter()
            if s == "mht_nees_nodes":      # (reads what the filter call of this round wrote)
                xf, Pf = outs["mht_filter_tracks"]
                rc = lib.mht_nees_nodes(ctx.handle, nx, n, L_max, nx, xf.data_ptr(), Pf.data_ptr(), truth.data_ptr(), present.data_ptr(), nees_out.data_ptr())
            else:
                rc = getattr(lib, s)(ctx.handle, C.byref(mx), n, L_max, lens_sorted.ctypes.data_as(C.c_void_p), x_d.data_ptr(), P_d.data_ptr(),
                                     z_d.data_ptr(), h_d.data_ptr(), *(o.data_ptr() for o in outs[s]), work[s].data_ptr(), need[s])      # (synchronises)
            times[s].append(time.perf_counter() - t0)
            _lib.check(rc, lib)
    assert bool(torch.isfinite(nees_out).all())
    return times, L_max, need


def main(out_path):
    import torch
    import filter_ref
    import nees_ref
    import smooth_ref as sr
    from pymht_amd import smoothing
    from pymht_amd.device import Context
    from pymht_amd.evaluation import _nees_launch
    from pymht_amd.models import pv, ca, ct
    assert torch.cuda.is_available(), "no GPU"
    lines = ["Filtered states of track histories (mht_filter_tracks: the score's forward pass with xf and the packed Pf of every node stored,",
             "N + NS doubles per node and lane, coalesced) next to the score (mht_score_tracks: the same pass, nothing stored per node) and next to",
             "the linear smoother (mht_smooth_tracks, with covariances: forward and backward, N + NS doubles per node in the workspace and again in",
             "the output), and the NEES of those states against truth (mht_nees_nodes, D = nx, every cell present: one cell per lane, 2 N + NS",
             "doubles and a flag read and N + 3 doubles written per cell), ONE process, ONE packed batch.  Times are the seams' own (copy of the",
             "lengths, the launch, the wait), %d warm-up rounds, then %d rounds, the four calls alternating.  Expectation from the code: the" % (WARM, REPS),
             "filter above the score and below the smoother; the NEES launch bound by the bytes it moves.", ""]
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
        r_score, r_smooth = st["mht_filter_tracks"][0] / st["mht_score_tracks"][0], st["mht_filter_tracks"][0] / st["mht_smooth_tracks"][0]
        lines.append("  filter / score (medians)      %.3f" % r_score)
        lines.append("  filter / smoother (medians)   %.3f" % r_smooth)
        lines.append("  the filter writes %.1f MB, the smoother's workspace and outputs are %.1f MB" % (L_max * (nx + nx * (nx + 1) // 2) * n * 8 / 1e6,
                                                                                                   (need["mht_smooth_tracks"] + L_max * (nx + nx * (nx + 1) // 2) * n * 8) / 1e6))
        lines.append("  as expected: above the score, below the smoother" if r_score > 1.0 and r_smooth < 1.0 else
                     "  NOT as expected (above the score: %s, below the smoother: %s)" % (r_score > 1.0, r_smooth < 1.0))
        moved = nees_bytes(nx, L_max * n)
        lines.append("  the NEES launch moves %.1f MB over %d cells: %.1f GB/s at the median, %.1f GB/s at the fastest call (launch and wait included)"
                     % (moved / 1e6, L_max * n, moved / st["mht_nees_nodes"][0] / 1e6, moved / st["mht_nees_nodes"][1] / 1e6))
        lines.append("")
    lines.append("Accuracy of the filter, ratios e_dev / max(e_np, eps64) against the np.longdouble reference (tests/filter_ref.py), criterion <= 8:")
    runs = {"linear": smoothing.filter_tracks, "ct": smoothing.filter_tracks_ct, "ais": smoothing.filter_tracks_ais, "ais-none": smoothing.filter_tracks_ais}
    for lib_nx in (4, 6):
        ctx = Context(0, nx=lib_nx)
        try:
            for kind, model in (("linear", pv), ("linear", ca), ("ct", ct), ("ais", pv), ("ais-none", pv)):
                tracks, truth, f64 = filter_ref.reference(kind, model, PERIOD, 130, 11)
                got = [dict(xf=a, Pf=b) for a, b in runs[kind](model, PERIOD, tracks, ctx=ctx)]
                res = filter_ref.ratios(got, truth, f64, filter_ref.NAMES)
                lines.append("  %-8s models/%-3s %d-state build: " % (kind, model.__name__.split(".")[-1], lib_nx)
                             + " | ".join("%s %.3g (e_np %.3g)" % (k, v[2], v[1]) for k, v in res.items()))
            lines.append("Accuracy of the NEES on the %d-state build, the cells of tests/test_nees_gpu.py (tests/nees_ref.py), criterion <= 8:" % lib_nx)
            for N in (4, 6):
                x, P, truth, present = nees_ref.cell_batch(N, 130, 60, seed=5)
                up = lambda a: torch.from_numpy(a).to(ctx.device)
                got = nees_ref.seam_dict(_nees_launch(ctx, N, 130, 60, N, up(x), up(P), truth, present), N)
                want, f64 = nees_ref.nees_batch(x, P, truth, present, N, np.longdouble), nees_ref.nees_batch(x, P, truth, present, N, np.float64)
                res = nees_ref.ratios([got], [want], [f64], nees_ref.NAMES)
                lines.append("  N %d D %d: " % (N, N) + " | ".join("%s %.3g (e_np %.3g)" % (k, v[2], v[1]) for k, v in res.items()))
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
        for unit, what in (("mht_smooth_filter.hip", "filter"), ("mht_nees.hip", "NEES")):
            found = res.unit_report(pathlib.Path(tempfile.mkdtemp()), unit, [])
            lines.append("Registers of the %s kernels (compiler's report, gfx950, the library's flags):" % what)
            for k, v in sorted(found.items()):
                lines.append("  %-90s VGPR %3d  AGPR %3d  scratch %d B  LDS %d B  VGPRs spilled %d" % (k, v["vgpr"], v["agpr"], v["scratch"], v["lds"], v["spill"]))
    except BaseException as exc:      # (no hipcc on this machine, or pytest's skip for the same reason)
        lines.append("Registers of the filter and NEES kernels: the compiler's report could not be made here (%s)" % type(exc).__name__)
    return lines


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "nees_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
