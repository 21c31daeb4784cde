"""What the fixed-interval IMM smoother over track histories costs next to what a user had before it -- the IMM filter for the mode
probabilities plus the plain smoother for a smoothed state -- in ONE process (sibling of tools/imm_cost.py, same batches).

  python tools/imm_smooth_cost.py [--out FILE]      (default FILE: profiles/imm_smooth_cost.txt)
      for 500 tracks x 200 nodes (models/pv, 4-state build) and 2 000 x 400 (models/ca, 6-state build), 80 % detections, T = 2.5:
        ONE packed batch on the device, and on it the seams' own times -- mht_imm_smooth_tracks at r = 2, 3, 4 against mht_imm_tracks at
        the same r and mht_smooth_tracks (neither changed by the smoother's arrival: mht_imm.hip compiles to the registers it had) --
        each timed around the library call (copy of the lengths and the modes, the launch, the wait), 3 warm-up rounds, then 20 rounds,
        the calls alternating within a round: median, min, max, and the ratio of the medians smoother / (filter + plain smoother)
        bytes moved per track and node, from the code
        accuracy ratios of the batches of tests/test_imm_smooth_gpu.py
        registers of the kernels, from the compiler's report (where hipcc is there)"""
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
MODES = (2, 3, 4)
Q_SCALES = (1.0, 16.0, 0.25, 4.0)      # the first r of them


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def time_batch(ctx, model, tracks, nx):
    """The plain smoother, and the IMM filter and the IMM smoother at r = 2, 3, 4, on one packed batch: {name: [seconds per call]}"""
    import torch
    from pymht_amd import _lib
    from pymht_amd.smoothing import _model_x, _pack, imm_modes
    lib, dev = ctx.lib, ctx.device
    n, ns = len(tracks), nx * (nx + 1) // 2
    lens, order, L_max, hp, (x_d, P_d, z_d, h_d) = _pack(ctx, tracks, nx)
    lens_sorted = np.ascontiguousarray(lens[order])
    mx, keep = _model_x(model, PERIOD, nx, False)
    new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
    xs, Ps = new(L_max, nx, n), new(L_max, ns, n)
    need_s = int(lib.mht_smooth_work_bytes(nx, n, L_max))
    work_s = new(need_s, dtype=torch.uint8)
    need_big = int(lib.mht_imm_smooth_work_bytes(nx, n, L_max, max(MODES)))
    work = new(need_big, dtype=torch.uint8)      # (one workspace for every IMM call: the largest)
    mu, muf, ll, nobs = new(L_max, max(MODES), n), new(L_max, max(MODES), n), new(n), new(n, dtype=torch.int32)
    modes = {r: [np.ascontiguousarray(m) for m in imm_modes(model, PERIOD, Q_SCALES[:r])] for r in MODES}
    torch.cuda.synchronize(dev)
    lp = lens_sorted.ctypes.data_as(C.c_void_p)
    batch = (x_d.data_ptr(), P_d.data_ptr(), z_d.data_ptr(), h_d.data_ptr())
    names = ["mht_smooth_tracks"] + [s % r for r in MODES for s in ("mht_imm_tracks r=%d", "mht_imm_smooth_tracks r=%d")]
    times = {s: [] for s in names}
    for _ in range(WARM + REPS):
        for s in names:
            t0 = time.perf_counter()
            if s == "mht_smooth_tracks":
                rc = lib.mht_smooth_tracks(ctx.handle, C.byref(mx), n, L_max, lp, *batch, xs.data_ptr(), Ps.data_ptr(), work_s.data_ptr(), need_s)
            else:
                r = int(s[-1])
                hostp = [m.ctypes.data_as(C.c_void_p) for m in modes[r]]
                if s.startswith("mht_imm_tracks"):
                    rc = lib.mht_imm_tracks(ctx.handle, C.byref(mx), n, L_max, lp, *batch, r, *hostp, mu.data_ptr(), xs.data_ptr(), Ps.data_ptr(),
                                            ll.data_ptr(), nobs.data_ptr(), work.data_ptr(), need_big)
                else:
                    rc = lib.mht_imm_smooth_tracks(ctx.handle, C.byref(mx), n, L_max, lp, *batch, r, *hostp, mu.data_ptr(), xs.data_ptr(), Ps.data_ptr(),
                                                   muf.data_ptr(), ll.data_ptr(), nobs.data_ptr(), work.data_ptr(), need_big)
            times[s].append(time.perf_counter() - t0)      # (every seam synchronises)
            _lib.check(rc, lib)
    assert bool(torch.isfinite(ll).all()) and bool(torch.isfinite(xs).all())
    return times


def all_times():
    """{model: {name: (median, min, max) ms}}"""
    import torch
    import smooth_ref as sr
    from pymht_amd.device import Context
    from pymht_amd.models import pv, ca
    assert torch.cuda.is_available(), "no GPU"
    out = {}
    for name, model in (("pv", pv), ("ca", ca)):
        n, L, nx = SIZES[name]
        tracks = sr.make_batch(model, PERIOD, [L] * n, seed=7, p_detect=0.8)
        ctx = Context(0, nx=nx)
        try:
            out[name] = {s: stats(t) for s, t in time_batch(ctx, model, tracks, nx).items()}
        finally:
            ctx.close()
    return out


def time_lines(res):
    lines = []
    for name in ("pv", "ca"):
        n, L, nx = SIZES[name]
        st = res[name]
        lines.append("models/%s, %d tracks x %d nodes, %d-state build (ms: median  min  max)" % (name, n, L, nx))
        for s, v in st.items():
            lines.append("  %-30s %9.3f %9.3f %9.3f" % ((s,) + tuple(v)))
        for r in MODES:
            both = st["mht_imm_tracks r=%d" % r][0] + st["mht_smooth_tracks"][0]
            lines.append("  r=%d: smoother / (filter + plain smoother) = %.3f / %.3f = %.2f;  smoother / filter = %.2f"
                         % (r, st["mht_imm_smooth_tracks r=%d" % r][0], both, st["mht_imm_smooth_tracks r=%d" % r][0] / both,
                            st["mht_imm_smooth_tracks r=%d" % r][0] / st["mht_imm_tracks r=%d" % r][0]))
    return lines


def byte_lines():
    lines = ["Bytes per track and node, from the code (N states, NS = N (N + 1) / 2, NV = N + NS, r modes; z and has_z: 17 read once):"]
    for nx in (4, 6):
        nv = nx + nx * (nx + 1) // 2
        for r in MODES:
            kept = r * (nv + 1) * 8
            back = r * ((r + 1) * nv + 1) * 8      # every mode loads its row once per term and once for the step, and its mu
            out = (2 * r + nv) * 8
            lines.append("  N = %d, r = %d: forward stores %4d, backward loads %5d (the row is loaded anew for each of the r terms and for the step: "
                         "from the cache behind the first), outputs %4d;  the workspace holds %4d" % (nx, r, kept, back, out, kept))
    return lines


def main(out_path):
    import imm_ref
    import imm_smooth_ref as ref
    from pymht_amd import smoothing
    from pymht_amd.device import Context
    from pymht_amd.models import pv, ca, ct
    lines = ["The fixed-interval IMM smoother over track histories (mht_imm_smooth_tracks: one (track, mode) per lane, ONE launch, the lane walks",
             "its track forward -- mht_imm_tracks' phases, every mode storing its row per node -- and backward: r predictions and Cholesky",
             "factors per mode and node for the terms, the back-mix, the smoother's own step) next to what there was before it for the same",
             "question: mht_imm_tracks for the mode probabilities plus mht_smooth_tracks for a smoothed state.  ONE process, ONE packed batch.",
             "Times are the seams' own (copy of the lengths and the modes, the launch, the wait), %d warm-up rounds, then %d rounds, the calls" % (WARM, REPS),
             "alternating.  Only the one-launch form was built: two launches were not tried.  No ratio was fixed in advance; this file",
             "records what was measured.", ""]
    lines += time_lines(all_times()) + [""]
    lines += byte_lines() + [""]
    lines.append("Accuracy, ratios e_dev / max(e_np, eps64) against the np.longdouble reference (tests/imm_smooth_ref.py), the batches of "
                 "tests/test_imm_smooth_gpu.py, criterion <= 8:")
    for lib_nx in (4, 6):
        ctx = Context(0, nx=lib_nx)
        try:
            for kind, model, key in (("linear", pv, 1), ("linear", pv, 2), ("linear", pv, 3), ("linear", pv, 4), ("linear", pv, "blocked"), ("linear", ca, 4), ("ct", ct, 2)):
                tracks, truth, f64 = ref.reference(kind, model, PERIOD, 35, 11, key)
                Q, R, Pi, mu0 = imm_ref.setup(model, PERIOD, key)
                run = smoothing.imm_smooth_tracks_ct if kind == "ct" else smoothing.imm_smooth_tracks
                got = [dict(mus=d["mu"], muf=d["muFiltered"], xs=d["x"], Ps=d["P"], ll=np.asarray(d["logLikelihood"]), nobs=d["nObs"])
                       for d in run(model, PERIOD, tracks, Q, R, Pi, mu0=mu0, ctx=ctx)]
                res = ref.ratios(got, truth, f64, ref.NAMES)
                lines.append("  %-6s models/%-3s modes %-7s %d-state build: " % (kind, model.__name__.split(".")[-1], key, lib_nx)
                             + " | ".join("%s %.3g (e_np %.3g)" % (k, v[2], v[1]) for k, v in res.items()))
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
        lines.append("Registers (compiler's report, gfx950, the library's flags):")
        for unit in ("mht_imm_smooth.hip", "mht_imm.hip"):
            found = res.unit_report(pathlib.Path(tempfile.mkdtemp()), unit, [])
            for k, v in sorted(found.items()):
                lines.append("  %-100s VGPR %3d  AGPR %3d  scratch %d B  LDS %d B  VGPRs spilled %d" % (k, v["vgpr"], v["agpr"], v["scratch"], v["lds"], v["spill"]))
    except BaseException as exc:      # (no hipcc on this machine, or pytest's skip for the same reason)
        lines.append("Registers: the compiler's report could not be made here (%s)" % type(exc).__name__)
    return lines


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "imm_smooth_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
