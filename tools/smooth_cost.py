"""What the device smoother (pymht_amd/smoothing.py, `mht_smooth_tracks`) costs next to the float64 NumPy recursion (tests/smooth_ref.py).

  python tools/smooth_cost.py [--out FILE] [--reference-tracks N]
      for 500 tracks x 200 nodes (models/pv) and 2 000 x 400 (models/ca), 80 % detections:
        (a) smooth_tracks() end to end -- host packing, upload, kernel, copy back, unpacking -- with and without covariances (median of 5 behind a warm-up)
        (b) the float64 NumPy reference, a loop over tracks and nodes; it is linear in the tracks, so it is timed on the first N (default 50) and scaled
            (--reference-tracks 0: all of them, minutes)
        accuracy of the 40-track batch of tests/test_smooth_gpu.py: e_dev / e_np against the np.longdouble truth
        kernel time from ONE `rocprofv3 --kernel-trace --stats` run (a run of its own) next to the bytes the kernel has to move
      Every step that touches the GPU is a child process under its own timeout; the first that fails ends the run.
  python tools/smooth_cost.py --ct [--out FILE]
      the constant-turn smoother (smooth_tracks_ct, `mht_smooth_tracks_ct`; default FILE: smooth_ct_cost.txt): the accuracy ratios of the
      40-track batch of tests/test_smooth_ct_gpu.py on both library builds, then 2 000 tracks x 400 nodes of models/ct with and without
      covariances -- end to end and, from one profiler run, per kernel -- and IN THE SAME RUN the linear six-state smoother (models/ca) on
      a batch of the same shape: the thing to compare with.
  (children: `time NAME`, `accuracy`, `trace`, `time-ct`, `accuracy-ct`, `trace-ct`)"""
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

PERIOD = 2.5
SIZES = {"pv": (500, 200), "ca": (2000, 400)}
HBM_PEAK = 8.0e12      # bytes / s, MI355X (HBM3E)


def model_of(name):
    from pymht_amd.models import pv, ca
    return {"pv": pv, "ca": ca}[name]


def batch(name):
    import smooth_ref as sr
    n, L = SIZES[name]
    return sr.make_batch(model_of(name), PERIOD, [L] * n, seed=99, p_detect=0.8)


def kernel_bytes(nx, n, L, cov=True):
    """What one launch has to move: forward writes and backward reads the filtered state of every node but the last (nx + nx (nx + 1) / 2
    doubles each way), reads z (2 doubles) and has_z (1 byte) per node, writes xs (nx) and Ps (nx (nx + 1) / 2) per node."""
    ns = nx * (nx + 1) // 2
    per_node = 2 * (nx + ns) * 8 + 2 * 8 + 1 + nx * 8 + (ns * 8 if cov else 0)
    return n * L * per_node


def child_time(name):
    import torch
    from pymht_amd.device import Context
    from pymht_amd.smoothing import smooth_tracks
    model, tracks = model_of(name), batch(name)
    nx = int(np.asarray(model.C_RADAR).shape[1])
    ctx = Context(0, nx=nx)
    res = {}
    for cov in (True, False):
        smooth_tracks(model, PERIOD, tracks, ctx=ctx, covariances=cov)      # warm-up: code object load, allocator
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            smooth_tracks(model, PERIOD, tracks, ctx=ctx, covariances=cov)      # (ends in a device-to-host copy: synchronous)
            ts.append(time.perf_counter() - t0)
        res["cov" if cov else "means"] = ts
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def child_accuracy():
    import smooth_ref as sr
    from pymht_amd.smoothing import smooth_tracks
    assert np.finfo(np.longdouble).eps < 1e-18
    res = {}
    for name in ("pv", "ca"):
        model = model_of(name)
        rng = np.random.default_rng(20240)
        tracks = sr.make_batch(model, PERIOD, [int(v) for v in rng.integers(2, 401, 40)], seed=17, p_detect=0.8)      # (the batch of tests/test_smooth_gpu.py)
        dev = smooth_tracks(model, PERIOD, tracks)
        mats = sr.model_matrices(model, PERIOD)
        e = np.zeros(4)
        for (x0, P0, z), (xs, Ps) in zip(tracks, dev):
            t, f = sr.rts(*mats, x0, P0, z, dtype=np.longdouble), sr.rts(*mats, x0, P0, z, dtype=np.float64)
            e = np.maximum(e, [sr.err(xs, t["xs"]), sr.err(f["xs"], t["xs"]), sr.err(Ps, t["Ps"]), sr.err(f["Ps"], t["Ps"])])
        res[name] = e.tolist()
    print("RESULT " + json.dumps(res), flush=True)


def child_trace():
    from pymht_amd.smoothing import smooth_tracks
    for name in ("pv", "ca"):
        tracks = batch(name)
        for cov in (True, False):
            for _ in range(3):
                smooth_tracks(model_of(name), PERIOD, tracks, covariances=cov)


CT_SIZE = (2000, 400)


def ct_batches():
    """(models/ct, its batch), (models/ca, a batch of the same shape)."""
    import smooth_ct_ref as cr
    import smooth_ref as sr
    from pymht_amd.models import ca, ct
    n, L = CT_SIZE
    return (ct, cr.make_batch(ct, PERIOD, [L] * n, seed=99, p_detect=0.8)), (ca, sr.make_batch(ca, PERIOD, [L] * n, seed=99, p_detect=0.8))


def child_time_ct():
    import torch
    from pymht_amd.device import Context
    from pymht_amd.smoothing import smooth_tracks, smooth_tracks_ct
    (ct, ct_tracks), (ca, ca_tracks) = ct_batches()
    ctx = Context(0, nx=6)
    res = {}
    for key, fn, model, tracks in (("ct", smooth_tracks_ct, ct, ct_tracks), ("ca", smooth_tracks, ca, ca_tracks)):
        for cov in (True, False):
            fn(model, PERIOD, tracks, ctx=ctx, covariances=cov)      # warm-up: code object load, allocator
            ts = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(model, PERIOD, tracks, ctx=ctx, covariances=cov)      # (ends in a device-to-host copy: synchronous)
                ts.append(time.perf_counter() - t0)
            res[key + ("_cov" if cov else "_means")] = ts
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def child_accuracy_ct():
    import smooth_ct_ref as cr
    import smooth_ref as sr
    from pymht_amd.device import Context
    from pymht_amd.models import ct
    from pymht_amd.smoothing import smooth_tracks_ct
    assert np.finfo(np.longdouble).eps < 1e-18
    rng = np.random.default_rng(20240)
    tracks = cr.make_batch(ct, PERIOD, [int(v) for v in rng.integers(2, 401, 40)], seed=17, p_detect=0.8)      # (the batch of tests/test_smooth_ct_gpu.py)
    mats = cr.model_matrices(ct, PERIOD)
    refs = [(cr.rts_ct(*mats, x0, P0, z, dtype=np.longdouble), cr.rts_ct(*mats, x0, P0, z, dtype=np.float64)) for x0, P0, z in tracks]
    res = {}
    for nx in (4, 6):
        ctx = Context(0, nx=nx)
        dev = smooth_tracks_ct(ct, PERIOD, tracks, ctx=ctx)
        ctx.close()
        e = np.zeros(4)
        for (xs, Ps), (t, f) in zip(dev, refs):
            e = np.maximum(e, [sr.err(xs, t["xs"]), sr.err(f["xs"], t["xs"]), sr.err(Ps, t["Ps"]), sr.err(f["Ps"], t["Ps"])])
        res[str(nx)] = e.tolist()
    print("RESULT " + json.dumps(res), flush=True)


def child_trace_ct():
    from pymht_amd.smoothing import smooth_tracks, smooth_tracks_ct
    (ct, ct_tracks), (ca, ca_tracks) = ct_batches()
    for fn, model, tracks in ((smooth_tracks_ct, ct, ct_tracks), (smooth_tracks, ca, ca_tracks)):
        for cov in (True, False):
            for _ in range(3):
                fn(model, PERIOD, tracks, covariances=cov)


def main_ct(out_path):
    n, L = CT_SIZE
    lines = ["tools/smooth_cost.py --ct: the constant-turn Rauch-Tung-Striebel smoother (mht_smooth_tracks_ct: A_k = Phi(T, w) rebuilt per lane and per node from the",
             "filtered turn rate, float64 sin / cos recomputed in the backward pass) next to the linear six-state smoother (mht_smooth_tracks, models/ca) IN THE SAME RUN",
             "80 % detections, T = 2.5; end-to-end times are smooth_tracks_ct() / smooth_tracks() (host packing, upload, kernel, copy back, unpacking), median of 5", ""]
    emit = lambda s: (lines.append(s), print(s, flush=True))
    acc = run_child(["accuracy-ct"], 420)
    for nx in ("4", "6"):
        e = acc[nx]
        emit("accuracy models/ct, %s-state build (40 tracks of 2-400 nodes, turn rates 0 .. 0.6 rad/s, half with a coupled P_init; truth = np.longdouble): "
             "means e_dev %.3g e_np %.3g ratio %.2f | covariances e_dev %.3g e_np %.3g ratio %.2f  (required: <= 8)"
             % (nx, e[0], e[1], e[0] / e[1], e[2], e[3], e[2] / e[3]))
    emit("")
    res = run_child(["time-ct"], 900)
    for key, label in (("ct", "models/ct  constant turn   "), ("ca", "models/ca  linear six-state")):
        emit("%s %5d tracks x %3d nodes: with covariances %8.1f ms (%s), means only %8.1f ms (%s)"
             % (label, n, L, 1e3 * np.median(res[key + "_cov"]), " ".join("%.1f" % (1e3 * t) for t in res[key + "_cov"]),
                1e3 * np.median(res[key + "_means"]), " ".join("%.1f" % (1e3 * t) for t in res[key + "_means"])))
    emit("")
    prof_dir = os.path.join(os.path.dirname(os.path.abspath(out_path)), "smooth_ct_prof")
    run_child(["trace-ct"], 900, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "-o", "smooth_ct", "--"])
    times = kernel_times(prof_dir)
    if not times:
        emit("kernel times: no smoother kernel in the profiler's output under %s" % os.path.relpath(prof_dir, ROOT))
    med = {}
    for kname, v in sorted(times.items()):
        inst = re.search(r"smooth_rts_(ct_)?kernel(?:<(?:6, )?(true|false)>|(?:ILi6E)?I?Lb([01])E)", kname)      # demangled or mangled
        cov = inst.group(2) == "true" or inst.group(3) == "1"
        b = kernel_bytes(6, n, L, cov)
        t = float(np.median(v))
        med[(bool(inst.group(1)), cov)] = t
        emit("kernel %-24s %s %5d x %3d: %d launches, median %9.1f us (min %.1f, max %.1f); %.1f MB to move -> %.1f GB/s = %.2f %% of %.0f TB/s HBM peak"
             % ("smooth_rts_ct_kernel" if inst.group(1) else "smooth_rts_kernel<6>", "covariances" if cov else "means only ", n, L, len(v), t, min(v), max(v),
                b / 1e6, b / t / 1e3, 100 * b / (t * 1e-6) / HBM_PEAK, HBM_PEAK / 1e12))
    for cov in (True, False):
        if (True, cov) in med and (False, cov) in med:
            emit("constant turn / linear six-state, kernel time, %s: %.2f" % ("covariances" if cov else "means only", med[(True, cov)] / med[(False, cov)]))
    emit("(both kernels move the same bytes and walk the same chain; the difference is the transition: nine multiply-adds per six-vector and a sin / cos pair per step")
    emit(" in the forward AND in the backward pass against a dense 6 x 6 product with a wave-uniform matrix)")
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


AIS_SIZE = (2000, 100)      # --ais: tracks x nodes


def child_time_ais():
    """The seams themselves (length copy, kernel, wait), inputs packed and uploaded once: 3 warm-up calls, then 20 timed ones each of
    mht_smooth_tracks (nx = 4), mht_smooth_tracks_ais on the same radar-only batch and mht_smooth_tracks_ais with 30 % AIS nodes."""
    import ctypes as C
    import torch
    import smooth_ais_ref as sa
    from pymht_amd import _lib
    from pymht_amd.device import Context
    from pymht_amd.models import pv
    from pymht_amd.smoothing import _ais_inputs
    n, L = AIS_SIZE
    ctx = Context(0, nx=4)
    lib, dev = ctx.lib, ctx.device
    keep = [np.ascontiguousarray(np.asarray(m, dtype=np.float32).ravel()) for m in (pv.Phi(PERIOD), pv.Q(PERIOD), pv.C_RADAR, pv.R_RADAR())]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    mx = _lib.MhtModelX(4, fp(keep[0]), fp(keep[1]), fp(keep[2]), fp(keep[3]), 0.0, 0.0, 0, PERIOD)
    lens = np.full(n, L, dtype=np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xs = torch.empty((L, 4, n), dtype=torch.float64, device=dev)
    Ps = torch.empty((L, 10, n), dtype=torch.float64, device=dev)
    need = int(lib.mht_smooth_ais_work_bytes(n, L))
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    res = {}
    for key, p_ais in (("radar", 0.0), ("ais", 0.3)):
        tracks = sa.make_batch(pv, PERIOD, [L] * n, seed=41, p_detect=0.8, p_ais=p_ais)
        per_track, legs = _ais_inputs(pv, tracks)
        z = np.array([t[2] for t in tracks])
        has = ~np.isnan(z).any(axis=2)
        has[:, 0] = False
        kind = has.astype(np.uint8) + 2 * np.array([p[0] for p in per_track], dtype=np.uint8)
        d = dict(x=up(np.array([t[0] for t in tracks]).T), P=up(np.array([t[1].ravel() for t in tracks]).T),
                 z=up(np.where(has[:, :, None], z, 0.0).transpose(1, 2, 0)), h=up(has.astype(np.uint8).T), k=up(kind.T),
                 m=up(np.array([p[1] for p in per_track]).transpose(1, 2, 0)), r=up(np.array([p[2] for p in per_track]).T),
                 l=up(np.array([p[3] for p in per_track]).T), legs=up(legs if len(legs) else np.zeros((1, 52))))
        res[key + "_share"] = float((kind[:, 1:] >= 2).mean())
        res[key + "_legs"] = len(legs)
        torch.cuda.synchronize()
        lp = lens.ctypes.data_as(C.c_void_p)
        for cov in (True, False):
            Pp = Ps.data_ptr() if cov else None
            calls = {"ais": lambda: lib.mht_smooth_tracks_ais(ctx.handle, C.byref(mx), n, L, lp, d["x"].data_ptr(), d["P"].data_ptr(), d["z"].data_ptr(),
                                                               d["h"].data_ptr(), d["k"].data_ptr(), d["m"].data_ptr(), d["r"].data_ptr(), d["l"].data_ptr(),
                                                               d["legs"].data_ptr(), max(len(legs), 1), xs.data_ptr(), Pp, work.data_ptr(), need)}
            if key == "radar":
                calls["linear"] = lambda: lib.mht_smooth_tracks(ctx.handle, C.byref(mx), n, L, lp, d["x"].data_ptr(), d["P"].data_ptr(), d["z"].data_ptr(),
                                                                d["h"].data_ptr(), xs.data_ptr(), Pp, work.data_ptr(), need)
            for name, fn in calls.items():
                ts = []
                for i in range(23):
                    t0 = time.perf_counter()
                    _lib.check(fn(), lib)
                    ts.append(time.perf_counter() - t0)
                res["%s_%s_%s" % (name, key, "cov" if cov else "means")] = ts[3:]
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def main_ais(out_path):
    n, L = AIS_SIZE
    lines = ["tools/smooth_cost.py --ais: the AIS-aware Rauch-Tung-Striebel smoother (mht_smooth_tracks_ais, four states) next to the linear four-state smoother",
             "(mht_smooth_tracks) IN THE SAME RUN.  %d tracks x %d nodes, 80 %% detections, T = 2.5, models/pv.  Times are the seams' (copy of the lengths, one kernel," % (n, L),
             "the wait), inputs packed and uploaded once: 3 warm-up calls, then the median of 20", ""]
    emit = lambda s: (lines.append(s), print(s, flush=True))
    res = run_child(["time-ais"], 600)
    med = lambda k: 1e6 * float(np.median(res[k]))
    span = lambda k: "min %.0f, max %.0f" % (1e6 * min(res[k]), 1e6 * max(res[k]))
    for cov, label in (("cov", "with covariances"), ("means", "means only      ")):
        a, b, c = med("linear_radar_" + cov), med("ais_radar_" + cov), med("ais_ais_" + cov)
        emit("%s  mht_smooth_tracks                       radar-only batch: %8.0f us (%s)" % (label, a, span("linear_radar_" + cov)))
        emit("%s  mht_smooth_tracks_ais                   radar-only batch: %8.0f us (%s)   / linear: %.2f" % (label, b, span("ais_radar_" + cov), b / a))
        emit("%s  mht_smooth_tracks_ais  %4.1f %% AIS nodes, %d leg entries: %8.0f us (%s)   / linear: %.2f   / itself radar-only: %.2f"
             % (label, 100 * res["ais_share"], res["ais_legs"], c, span("ais_ais_" + cov), c / a, c / b))
        emit("")
    emit("(the radar-only batch runs the linear kernel's arithmetic through the new kernel: what it pays on top is one byte load of `kind` per node and pass and the")
    emit(" second filtered slot's stride in the workspace; the leg gather and the two extra steps are paid by AIS nodes only -- but by the whole wavefront, whose lanes")
    emit(" without a message wait while the others walk their legs: with 30 % AIS nodes nearly every wavefront step has one)")
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def run_child(args, timeout, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + list(args)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-3000:] + out.stderr[-3000:])
        raise SystemExit("step %s failed with exit status %d: stopping" % (" ".join(args), out.returncode))
    for line in out.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    return None


def kernel_times(prof_dir):
    """Durations (us) per smoother kernel instance from the profiler's output: the kernel-trace CSV, or the rocpd database."""
    times = {}
    for path in glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True):
        import csv
        for row in csv.DictReader(open(path)):
            if "smooth_rts_" in row["Kernel_Name"]:
                times.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if times:
        return times
    for path in glob.glob(os.path.join(prof_dir, "**", "*.db"), recursive=True):
        import sqlite3
        c = sqlite3.connect(path)
        tabs = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
        disp = next(t for t in tabs if t.startswith("rocpd_kernel_dispatch"))
        sym = next(t for t in tabs if t.startswith("rocpd_info_kernel_symbol"))
        names = {r[0]: r[1] for r in c.execute('select id, kernel_name from "%s"' % sym)}
        for kid, s, e in c.execute('select kernel_id, start, end from "%s" order by start' % disp):
            if "smooth_rts_" in names[kid]:
                times.setdefault(names[kid], []).append((e - s) / 1e3)
    return times


def main():
    import smooth_ref as sr
    out_path, n_ref, ct_mode, ais_mode = None, 50, False, False
    argv = sys.argv[1:]
    while argv:
        a = argv.pop(0)
        if a == "--out":
            out_path = argv.pop(0)
        elif a == "--reference-tracks":
            n_ref = int(argv.pop(0))
        elif a == "--ct":
            ct_mode = True
        elif a == "--ais":
            ais_mode = True
    if out_path is None:
        out_path = os.path.join(os.environ.get("OUT_DIR", os.path.join(ROOT, "out")), "smooth_ais_cost.txt" if ais_mode else "smooth_ct_cost.txt" if ct_mode else "smooth_cost.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    if ais_mode:
        return main_ais(out_path)
    if ct_mode:
        return main_ct(out_path)
    lines = ["tools/smooth_cost.py: the device Rauch-Tung-Striebel smoother (mht_smooth_tracks, one track per lane) against the float64 NumPy recursion",
             "80 % detections, T = 2.5; device times are smooth_tracks() end to end (host packing, upload, kernel, copy back, unpacking), median of 5", ""]
    emit = lambda s: (lines.append(s), print(s, flush=True))
    acc = run_child(["accuracy"], 300)
    for name in ("pv", "ca"):
        e = acc[name]
        emit("accuracy models/%s (40 tracks of 2-400 nodes, truth = np.longdouble): means e_dev %.3g e_np %.3g ratio %.2f | covariances e_dev %.3g e_np %.3g ratio %.2f  (required: <= 8)"
             % (name, e[0], e[1], e[0] / e[1], e[2], e[3], e[2] / e[3]))
    emit("")
    dev_cov = {}
    for name in ("pv", "ca"):
        n, L = SIZES[name]
        res = run_child(["time", name], 420)
        tracks = batch(name)
        mats = sr.model_matrices(model_of(name), PERIOD)
        k = n if n_ref <= 0 else min(n_ref, n)
        t0 = time.perf_counter()
        for x0, P0, z in tracks[:k]:
            sr.rts(*mats, x0, P0, z, dtype=np.float64)
        t_np = (time.perf_counter() - t0) * n / k
        dev_cov[name] = float(np.median(res["cov"]))
        emit("%s  %5d tracks x %3d nodes: device with covariances %8.1f ms (%s), means only %8.1f ms | NumPy float64 %9.1f ms (%d tracks timed%s) | NumPy / device %.0f x"
             % (name, n, L, 1e3 * np.median(res["cov"]), " ".join("%.1f" % (1e3 * t) for t in res["cov"]), 1e3 * np.median(res["means"]), 1e3 * t_np, k,
                "" if k == n else ", scaled by %d / %d" % (n, k), t_np / np.median(res["cov"])))
        if not np.median(res["cov"]) < t_np:
            emit("  !! the device path is NOT faster than the NumPy loop at this size")
    emit("")
    prof_dir = os.path.join(os.path.dirname(os.path.abspath(out_path)), "smooth_prof")
    run_child(["trace"], 600, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "-o", "smooth", "--"])
    times = kernel_times(prof_dir)
    if not times:
        emit("kernel times: no smooth_rts_kernel in the profiler's output under %s" % os.path.relpath(prof_dir, ROOT))
    for kname, v in sorted(times.items()):
        inst = re.search(r"smooth_rts_kernel(?:<(\d), (true|false)>|ILi(\d)ELb([01])E)", kname)      # demangled or mangled
        nx = int(inst.group(1) or inst.group(3))
        cov = inst.group(2) == "true" or inst.group(4) == "1"
        n, L = SIZES["pv" if nx == 4 else "ca"]
        b = kernel_bytes(nx, n, L, cov)
        t = float(np.median(v))
        emit("kernel smooth_rts_kernel<%d, %s> %5d x %3d: %d launches, median %9.1f us (min %.1f, max %.1f); %.1f MB to move -> %.1f GB/s = %.2f %% of %.0f TB/s HBM peak"
             % (nx, "covariances" if cov else "means only", n, L, len(v), t, min(v), max(v), b / 1e6, b / t / 1e3, 100 * b / (t * 1e-6) / HBM_PEAK, HBM_PEAK / 1e12))
    emit("(a batch is n / 64 wavefronts of one serial chain per lane -- 8 wavefronts at 500 tracks, 32 at 2 000, on a device with 1 024 SIMDs: the kernel is bound by the")
    emit(" latency of the chain, not by bandwidth; the rest of the end-to-end time is host packing, the copies and the unpacking)")
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "time":
        child_time(sys.argv[2])
    elif len(sys.argv) > 1 and sys.argv[1] == "accuracy":
        child_accuracy()
    elif len(sys.argv) > 1 and sys.argv[1] == "trace":
        child_trace()
    elif len(sys.argv) > 1 and sys.argv[1] == "time-ct":
        child_time_ct()
    elif len(sys.argv) > 1 and sys.argv[1] == "accuracy-ct":
        child_accuracy_ct()
    elif len(sys.argv) > 1 and sys.argv[1] == "time-ais":
        child_time_ais()
    elif len(sys.argv) > 1 and sys.argv[1] == "trace-ct":
        child_trace_ct()
    else:
        main()
