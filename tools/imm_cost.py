"""What an interacting-multiple-model filter over track histories costs next to filtering them under one model, in ONE process (sibling
of tools/nees_cost.py, same batches), and which of the two cross-lane reads the lanes of a quad should talk through.

  python tools/imm_cost.py [--out FILE]      (default FILE: profiles/imm_cost.txt)
      for 500 tracks x 200 nodes (models/pv, 4-state build) and 2 000 x 400 (models/ca, 6-state build), 80 % detections, T = 2.5:
        ONE packed batch on the device, and on it the seams' own times -- mht_imm_tracks at r = 2, 3, 4 against mht_filter_tracks --
        each timed around the library call (copy of the lengths and the modes, the launch, the wait), 3 warm-up rounds, then 20 rounds,
        the four calls alternating within a round: median, min, max, and the ratios of the medians
        the same with the library's other quad_read (csrc/mht_imm.hip: the DPP quad_perm broadcast is the default, __shfl at the quad's
        lane is -DMHT_IMM_QUAD_SHFL), where a build of it made by hand is there:
            MHT_LIB_VARIANT=.shfl MHT_EXTRA_HIPCC_FLAGS=-DMHT_IMM_QUAD_SHFL python -m pymht_amd.build
        timed in a child process of its own (a library is picked when it is loaded), the parent waiting
        accuracy ratios of the batches of tests/test_imm_gpu.py
        registers of the IMM kernels, from the compiler's report (where hipcc is there)
  python tools/imm_cost.py --times-only      the timing alone, as one JSON line (what the child process runs)"""
import ctypes as C
import json
import os
import subprocess
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
VARIANT = ".shfl"


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def time_batch(ctx, model, tracks, nx):
    """The filter seam and the IMM seam at r = 2, 3, 4 on one packed batch: {name: [seconds per call]}"""
    import torch
    from pymht_amd import _lib
    from pymht_amd.smoothing import _model_x, _pack, imm_modes
    lib, dev = ctx.lib, ctx.device
    n, ns = len(tracks), nx * (nx + 1) // 2
    lens, order, L_max, hp, (x_d, P_d, z_d, h_d) = _pack(ctx, tracks, nx)
    lens_sorted = np.ascontiguousarray(lens[order])
    mx, keep = _model_x(model, PERIOD, nx, False)
    new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
    xf, Pf = new(L_max, nx, n), new(L_max, ns, n)
    need_f = int(lib.mht_filter_work_bytes(nx, n, L_max))
    work_f = new(need_f, dtype=torch.uint8)
    imm = {}
    for r in MODES:
        modes = [np.ascontiguousarray(m) for m in imm_modes(model, PERIOD, Q_SCALES[:r])]
        need = int(lib.mht_imm_work_bytes(nx, n, L_max, r))
        imm[r] = (modes, [new(L_max, r, n), new(L_max, nx, n), new(L_max, ns, n), new(n), new(n, dtype=torch.int32)], new(need, dtype=torch.uint8), need)
    torch.cuda.synchronize(dev)
    lp = lens_sorted.ctypes.data_as(C.c_void_p)
    batch = (x_d.data_ptr(), P_d.data_ptr(), z_d.data_ptr(), h_d.data_ptr())
    names = ["mht_filter_tracks"] + ["mht_imm_tracks r=%d" % r for r in MODES]
    times = {s: [] for s in names}
    for _ in range(WARM + REPS):
        for s in names:
            t0 = time.perf_counter()
            if s == "mht_filter_tracks":
                rc = lib.mht_filter_tracks(ctx.handle, C.byref(mx), n, L_max, lp, *batch, xf.data_ptr(), Pf.data_ptr(), work_f.data_ptr(), need_f)
            else:
                modes, outs, work, need = imm[int(s[-1])]
                rc = lib.mht_imm_tracks(ctx.handle, C.byref(mx), n, L_max, lp, *batch, len(modes[0]), *(m.ctypes.data_as(C.c_void_p) for m in modes),
                                        *(o.data_ptr() for o in outs), work.data_ptr(), need)      # (synchronises)
            times[s].append(time.perf_counter() - t0)
            _lib.check(rc, lib)
    assert all(bool(torch.isfinite(imm[r][1][3]).all()) for r in MODES)
    return times


def all_times():
    """{model: {name: (median, min, max) ms}} on the library this process loads"""
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


def time_lines(title, res):
    lines = []
    for name in ("pv", "ca"):
        n, L, nx = SIZES[name]
        st = res[name]
        lines.append("%s: models/%s, %d tracks x %d nodes, %d-state build (ms: median  min  max;  median / the filter's)" % (title, name, n, L, nx))
        for s, v in st.items():
            lines.append("  %-22s %9.3f %9.3f %9.3f   %6.2f" % ((s,) + tuple(v) + (v[0] / st["mht_filter_tracks"][0],)))
    return lines


def other_variant():
    """The times of the hand-made build with the other quad_read, from a child process; None where there is no such build"""
    from pymht_amd import build
    if os.environ.get("MHT_LIB_VARIANT") or not all(os.path.exists(build.lib_path(nx) + VARIANT) for nx in (4, 6)):
        return None
    env = dict(os.environ, MHT_LIB_VARIANT=VARIANT)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--times-only"], env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError("the %s build failed: %s" % (VARIANT, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main(out_path):
    import imm_ref
    from pymht_amd import smoothing
    from pymht_amd.device import Context
    from pymht_amd.models import pv, ca, ct
    lines = ["An interacting-multiple-model filter over track histories (mht_imm_tracks: one (track, mode) per lane, the four lanes of a quad the",
             "modes of a track, sixteen tracks a wavefront; per node the mixing and the combination read the other modes' registers, 2 (r N + r (N + NS))",
             "doubles across lanes, and r + N + NS doubles are stored per track) next to the filter under one model (mht_filter_tracks: one track",
             "per lane, N + NS doubles stored per node), ONE process, ONE packed batch.  Times are the seams' own (copy of the lengths and the",
             "modes, the launch, the wait), %d warm-up rounds, then %d rounds, the four calls alternating.  Expectation from the code: a small" % (WARM, REPS),
             "multiple of the filter launch -- r times the lanes (four times the wavefronts whatever r is: a quad per track) at the same walk",
             "length, plus the mixing.  Nobody had measured it; this file records what it is.", ""]
    mine = all_times()
    lines += time_lines("quad_read by DPP quad_perm (the library)", mine) + [""]
    other = other_variant()
    if other is None:
        lines += ["quad_read by __shfl: no build of it here (see the head of tools/imm_cost.py)", ""]
    else:
        lines += time_lines("quad_read by __shfl (-DMHT_IMM_QUAD_SHFL, a build made by hand, a process of its own)", other) + [""]
        for name in ("pv", "ca"):
            lines.append("  models/%s, shuffle / DPP (medians): " % name +
                         "  ".join("r=%d %.3f" % (r, other[name]["mht_imm_tracks r=%d" % r][0] / mine[name]["mht_imm_tracks r=%d" % r][0]) for r in MODES))
        lines.append("")
    lines.append("Accuracy, ratios e_dev / max(e_np, eps64) against the np.longdouble reference (tests/imm_ref.py), the batches of tests/test_imm_gpu.py, criterion <= 8:")
    for lib_nx in (4, 6):
        ctx = Context(0, nx=lib_nx)
        try:
            for kind, model, key in (("linear", pv, 1), ("linear", pv, 2), ("linear", pv, 3), ("linear", pv, 4), ("linear", pv, "blocked"), ("linear", ca, 4), ("ct", ct, 2)):
                tracks, truth, f64 = imm_ref.reference(kind, model, PERIOD, 35, 11, key)
                Q, R, Pi, mu0 = imm_ref.setup(model, PERIOD, key)
                run = smoothing.imm_tracks_ct if kind == "ct" else smoothing.imm_tracks
                per, ll, nobs = run(model, PERIOD, tracks, Q, R, Pi, mu0=mu0, ctx=ctx)
                got = [dict(mu=m, x=x, P=P, ll=np.asarray(a), nobs=int(b)) for (m, x, P), a, b in zip(per, ll, nobs)]
                res = imm_ref.ratios(got, truth, f64, imm_ref.NAMES)
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
        found = res.unit_report(pathlib.Path(tempfile.mkdtemp()), "mht_imm.hip", [])
        lines.append("Registers of the IMM kernels (compiler's report, gfx950, the library's flags):")
        for k, v in sorted(found.items()):
            lines.append("  %-90s VGPR %3d  AGPR %3d  scratch %d B  LDS %d B  VGPRs spilled %d" % (k, v["vgpr"], v["agpr"], v["scratch"], v["lds"], v["spill"]))
    except BaseException as exc:      # (no hipcc on this machine, or pytest's skip for the same reason)
        lines.append("Registers of the IMM kernels: the compiler's report could not be made here (%s)" % type(exc).__name__)
    return lines


if __name__ == "__main__":
    if "--times-only" in sys.argv:
        print(json.dumps(all_times()))
    else:
        out = os.path.join(ROOT, "profiles", "imm_cost.txt")
        if "--out" in sys.argv:
            out = sys.argv[sys.argv.index("--out") + 1]
        main(out)
