"""What OSPA(2) over windows costs on the device next to the reference's computation on the host, in ONE process.

  python tools/ospa2_cost.py [--out FILE]      (default FILE: profiles/ospa2_cost.txt)
      two batches of tests/ospa2_ref.py's tracker-like scene (c = 20, p = 2):
          500 targets over 100 steps, windows of 10 steps ending at every step      (100 windows)
        2 000 targets over  50 steps, windows of 10 steps ending at every 5th step   (10 windows; cfg5's size)
      on each: the seam's own time (mht_ospa2_windows on a run that is already on the device: copy of the windows, three launches, the
      wait), the base-distance launch and the assignment launch separately by events (mht_ospa2_set_timing), against the reference's
      computation on the host (a vectorised NumPy base distance plus scipy.optimize.linear_sum_assignment per window, float64 sums),
      3 warm-up rounds, then 20 rounds of the seam: median, min, max and the ratio of the medians.  One round of the host loop takes
      seconds (3 - 9 s on the first batch and 5 - 18 s on the second, by the host), so it alternates with the seam in the first 1 + 5 and 1 + 3 rounds only
      (warm-up + timed) and the file says so.  The tracks are the scene's first 500 and 2 000 (the scene makes more tracks than targets:
      fragments and false tracks).  Beside them the column sweeps the search makes, counted by the host twin
      (tests/hostmath/ospa2_host.cpp), and the device's figures held to the criterion of the tests (every window of the first batch; the first, a middle and the last window of the second, whose
      reference in np.longdouble takes 5 s a window).
      Without a device the file says NOT YET MEASURED and holds the sweep counts alone."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

WARM, REPS = 3, 20
CUT, P, W = 20.0, 2, 10


def stats(ts, warm=WARM):
    ts = np.array(ts[warm:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def host_twin():
    so = os.path.join(tempfile.mkdtemp(), "libospa2_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "ospa2_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.ospa2_window_host.argtypes = ([C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_double, C.c_int32] + [C.c_void_p] * 4)
    return lib


def count_sweeps(lib, run, lo, hi):
    n = run[1].shape[1]
    win, count, match, sweeps = np.zeros(2), np.zeros(3, dtype=np.int32), np.zeros(n + 1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    assert lib.ospa2_window_host(len(run[1]), n, run[0].ctypes.data, run[1].ctypes.data, run[3].shape[1], run[2].ctypes.data, run[3].ctypes.data,
                                 lo, hi, CUT, P, win.ctypes.data, count.ctypes.data, match.ctypes.data, sweeps.ctypes.data) == 0
    return int(sweeps[0]), int(min(count[1], count[2]))


def host_batch(run, wins):
    """The reference's work per window in float64: base distances (vectorised), assignment on D^p, pairs that are no edges dropped, sums"""
    from scipy.optimize import linear_sum_assignment
    import ospa2_ref as ref
    on = (run[1] != 0, run[3] != 0)
    out = []
    for lo, hi in wins:
        ti, tj, D, nNear = ref.base_distances(run[0], on[0], run[2], on[1], lo, hi, CUT)
        rows, cols = linear_sum_assignment(D ** P)
        keep = (nNear[rows, cols] > 0) & (D[rows, cols] < CUT)
        loc = float((D[rows, cols][keep] ** P).sum())
        k = int(keep.sum())
        out.append((loc + CUT ** P * (max(len(ti), len(tj)) - k), loc, k))
    return out


class DeviceRun:
    """A run on the device once; call() is the seam alone"""

    def __init__(self, ctx, run, wins):
        import torch
        self.ctx, dev = ctx, ctx.device
        self.K, self.n, self.m, self.k = len(run[1]), run[1].shape[1], run[3].shape[1], len(wins)
        self.lo = np.ascontiguousarray([w[0] for w in wins], dtype=np.int32)
        self.hi = np.ascontiguousarray([w[1] for w in wins], dtype=np.int32)
        self.dev = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in run]
        self.win = torch.empty((self.k, 2), dtype=torch.float64, device=dev)
        self.count = torch.empty((self.k, 3), dtype=torch.int32, device=dev)
        self.match = torch.empty((self.k, self.n), dtype=torch.int32, device=dev)
        self.need = int(ctx.lib.mht_ospa2_work_bytes(self.n, self.m, self.K, self.k))
        self.work = torch.empty(self.need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

    def call(self):
        from pymht_amd import _lib
        d = self.dev
        _lib.check(self.ctx.lib.mht_ospa2_windows(self.ctx.handle, self.K, self.n, d[0].data_ptr(), d[1].data_ptr(), self.m, d[2].data_ptr(), d[3].data_ptr(),
                                                  self.k, self.lo.ctypes.data, self.hi.ctypes.data, CUT, P, self.win.data_ptr(), self.count.data_ptr(),
                                                  self.match.data_ptr(), self.work.data_ptr(), self.need), self.ctx.lib)      # (synchronises)
        ms = (C.c_float * 3)()
        self.ctx.lib.mht_ospa2_stage_times(C.byref(ms))
        return tuple(ms)

    def windows(self):
        win, count, match = self.win.cpu().numpy(), self.count.cpu().numpy(), self.match.cpu().numpy()
        return [(win[w, 0], win[w, 1], count[w, 0], count[w, 1], count[w, 2], match[w]) for w in range(self.k)]


def main(out_path):
    import ospa2_ref as ref
    twin = host_twin()
    def scene(T, K):      # (the first T tracks: T x T)
        run = ref.tracker_scene(T, seed=T, K=K)
        return np.ascontiguousarray(run[0][:, :T]), np.ascontiguousarray(run[1][:, :T]), run[2], run[3]
    # label, run, every, host rounds (warm-up, timed), windows held to the reference (None: all)
    batches = [("tracker-like scene of 500 targets over 100 steps, windows of %d steps ending at every step" % W, scene(500, 100), 1, (1, 5), None),
               ("tracker-like scene of 2 000 targets over 50 steps (cfg5's size), windows of %d steps ending at every 5th step" % W,
                scene(2000, 50), 5, (1, 3), (0, 4, 9))]
    lines = ["OSPA(2) over windows on the device (mht_ospa2_windows: membership, the base distances of every (track, truth) pair of every window,",
             "one wavefront per window for the assignment search with its tables in LDS) next to the reference's computation on the host (NumPy",
             "base distances, scipy.optimize.linear_sum_assignment per window); c = %g, p = %d.  Times are the seam's own (the run is on the device" % (CUT, P),
             "already: copy of the windows, three launches, the wait), its launches by events, and the host loop's; ONE process, %d warm-up rounds," % WARM,
             "then %d rounds of the seam; the host loop alternates with it in the first rounds only (how many: below).  Sweeps: column sweeps" % REPS,
             "of the search, counted by the host twin of the kernel's code; the expectation from the algorithm is about one sweep per row on",
             "tracker-like scenes.", ""]
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    ctx = None
    if have_gpu:
        from pymht_amd.device import Context
        ctx = Context(0)
        ctx.lib.mht_ospa2_set_timing(1)
    else:
        lines += ["NOT YET MEASURED on the device: no GPU was visible where this file was written; the sweep counts below are the host twin's.", ""]
    try:
        for label, run, every, (h_warm, h_reps), held in batches:
            K, n, m = len(run[1]), run[1].shape[1], run[3].shape[1]
            wins = ref.sliding(K, W, every)
            counted = [count_sweeps(twin, run, lo, hi) for lo, hi in wins]
            sweeps, rows = [s for s, _ in counted], [max(r, 1) for _, r in counted]
            lines.append(label)
            lines.append("  %d tracks x %d truths x %d steps, %d windows; rows per window (the smaller side) %d .. %d; sweeps per window: median %d, min %d, max %d;"
                         " sweeps / rows: median %.2f" % (n, m, K, len(wins), min(rows), max(rows), np.median(sweeps), min(sweeps), max(sweeps),
                                                          np.median(np.array(sweeps) / np.array(rows))))
            if ctx is None:
                lines.append("")
                continue
            dev = DeviceRun(ctx, run, wins)
            lines.append("  workspace %.1f MB" % (dev.need / 1e6))
            t_dev, t_host, t_stage = [], [], []
            for _ in range(WARM + REPS):
                t0 = time.perf_counter()
                ms = dev.call()
                t_dev.append(time.perf_counter() - t0)
                t_stage.append(ms)
                if len(t_host) < h_warm + h_reps:
                    t0 = time.perf_counter()
                    host_batch(run, wins)
                    t_host.append(time.perf_counter() - t0)
            for w, (got, (lo, hi)) in enumerate(zip(dev.windows(), wins)):
                if held is None or w in held:
                    ref.hold(got, ref.reference(*run, lo, hi, CUT, P), hi - lo + 1)
            sd, sh = stats(t_dev), stats(t_host, h_warm)
            st = [stats([s[k] * 1e-3 for s in t_stage]) for k in range(3)]
            lines.append("  (ms: median  min  max)")
            lines.append("  mht_ospa2_windows, whole batch      %10.3f %10.3f %10.3f" % sd)
            lines.append("    membership launch (events)        %10.3f %10.3f %10.3f" % st[0])
            lines.append("    base-distance launch (events)     %10.3f %10.3f %10.3f" % st[1])
            lines.append("    assignment launch (events)        %10.3f %10.3f %10.3f" % st[2])
            lines.append("  NumPy + SciPy on the host, batch    %10.3f %10.3f %10.3f      (%d warm-up + %d rounds)" % (sh + (h_warm, h_reps)))
            lines.append("  host / device (medians)             %10.1f" % (sh[0] / sd[0]))
            pairs = sum((hi - lo + 1) for lo, hi in wins) * n * m
            lines.append("  base-distance launch: %.2f G pair-steps/s over the full n x m x W of every window (members only are computed)"
                         % (pairs / (st[1][0] * 1e-3) / 1e9))
            lines.append("  %s meet%s the tests' criterion against the reference (counts and matches exact)"
                         % (("every window", "s") if held is None else ("windows %s" % ", ".join(str(w) for w in held), "")))
            lines.append("")
    finally:
        if ctx is not None:
            ctx.lib.mht_ospa2_set_timing(0)
            ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "ospa2_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
