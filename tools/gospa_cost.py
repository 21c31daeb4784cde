"""What GOSPA on the device costs next to the SciPy reference on the host, in ONE process.

  python tools/gospa_cost.py [--out FILE]      (default FILE: profiles/gospa_cost.txt)
      three batches (tests/gospa_ref.py's scenes, c = 20, p = 2, every step drawn with its own seed):
        100 steps of the sparse tracker-like scene of 500 targets (10 % undetected, 10 % false estimates, sigma 2.5)
         20 steps of the dense scene, 137 estimates x 130 truths inside one cut-off
          5 steps of the sparse scene of 2 000 targets (cfg5's size: the search tables take more than the 48 KB of LDS a kernel has by default)
      on each: the seam's own time (mht_gospa_steps on a batch that is already on the device: copy of the offsets, ONE launch, the
      wait) against scipy.optimize.linear_sum_assignment on min(d, c)^p step by step on the host (distances, assignment, cut-off
      pairs dropped, float64 sums), 3 warm-up rounds, then 20 rounds, the calls alternating within a round: median, min, max and the
      ratio of the medians; beside them the column sweeps the search makes, counted by the host twin (tests/hostmath/gospa_host.cpp),
      and the device's figures held to the criterion of the tests.
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
CUT, P = 20.0, 2


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def host_twin():
    so = os.path.join(tempfile.mkdtemp(), "libgospa_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "gospa_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.gospa_step_host.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_int32] + [C.c_void_p] * 4
    return lib


def count_sweeps(lib, X, Y):
    X, Y = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(Y, dtype=np.float64)
    step, count, match, sweeps = np.zeros(2), np.zeros(3, dtype=np.int32), np.zeros(len(X) + 1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    assert lib.gospa_step_host(len(X), X.ctypes.data, len(Y), Y.ctypes.data, CUT, P, step.ctypes.data, count.ctypes.data, match.ctypes.data,
                               sweeps.ctypes.data) == 0
    return int(sweeps[0])


def scipy_batch(X, Y):
    """The reference's work per step in float64: distances, assignment on min(d, c)^p, cut-off pairs dropped, the sums"""
    from scipy.optimize import linear_sum_assignment
    import gospa_ref as ref
    out = []
    for x, y in zip(X, Y):
        d = ref.distances(x, y)
        rows, cols = linear_sum_assignment(np.minimum(d, CUT) ** P)
        keep = d[rows, cols] < CUT
        loc = float((d[rows, cols][keep] ** P).sum())
        k = int(keep.sum())
        out.append((loc + CUT ** P / 2 * (len(x) + len(y) - 2 * k), loc, k))
    return out


class DeviceBatch:
    """A batch packed on the device once; call() is the seam alone"""

    def __init__(self, ctx, X, Y):
        import torch
        self.ctx, self.torch, dev = ctx, torch, ctx.device
        self.est_off = np.concatenate([[0], np.cumsum([len(x) for x in X])]).astype(np.int32)
        self.tru_off = np.concatenate([[0], np.cumsum([len(y) for y in Y])]).astype(np.int32)
        self.n = len(X)
        self.est = torch.from_numpy(np.concatenate(X)).to(dev)
        self.tru = torch.from_numpy(np.concatenate(Y)).to(dev)
        self.step = torch.empty((self.n, 2), dtype=torch.float64, device=dev)
        self.count = torch.empty((self.n, 3), dtype=torch.int32, device=dev)
        self.match = torch.empty(int(self.est_off[-1]), dtype=torch.int32, device=dev)
        self.need = int(ctx.lib.mht_gospa_work_bytes(self.n, int(self.est_off[-1]), int(self.tru_off[-1])))
        self.work = torch.empty(self.need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

    def call(self):
        from pymht_amd import _lib
        _lib.check(self.ctx.lib.mht_gospa_steps(self.ctx.handle, self.n, self.est_off.ctypes.data, self.est.data_ptr(), self.tru_off.ctypes.data,
                                                self.tru.data_ptr(), CUT, P, self.step.data_ptr(), self.count.data_ptr(), self.match.data_ptr(),
                                                self.work.data_ptr(), self.need), self.ctx.lib)      # (synchronises)

    def steps(self):
        step, count, match = self.step.cpu().numpy(), self.count.cpu().numpy(), self.match.cpu().numpy()
        return [(step[s, 0], step[s, 1], count[s, 0], count[s, 1], count[s, 2], match[self.est_off[s]:self.est_off[s + 1]]) for s in range(self.n)]


def main(out_path):
    import gospa_ref as ref
    twin = host_twin()
    batches = [("sparse tracker-like scene of 500 targets, 100 steps", [ref.sparse_scene(500, seed=1000 + s) for s in range(100)]),
               ("dense scene, 137 estimates x 130 truths inside one cut-off, 20 steps", [ref.dense_scene(seed=2000 + s) for s in range(20)]),
               ("sparse tracker-like scene of 2 000 targets (cfg5's size, 55 KB of LDS), 5 steps", [ref.sparse_scene(2000, seed=3000 + s) for s in range(5)])]
    lines = ["GOSPA of a batch of steps on the device (mht_gospa_steps: one launch, one step per workgroup of one wavefront, the search tables in",
             "LDS) next to scipy.optimize.linear_sum_assignment on min(d, c)^p step by step on the host; c = %g, p = %d.  Times are the seam's own" % (CUT, P),
             "(the batch is on the device already: copy of the offsets, the launch, the wait) and the host loop's (distances, assignment, sums),",
             "ONE process, %d warm-up rounds, then %d rounds, the calls alternating within a round.  Sweeps: column sweeps of the search, counted" % (WARM, REPS),
             "by the host twin of the kernel's code; the expectation from the algorithm is about one sweep per row on tracker-like scenes.", ""]
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    ctx = None
    if have_gpu:
        from pymht_amd.device import Context
        ctx = Context(0)
    else:
        lines += ["NOT YET MEASURED on the device: no GPU was visible where this file was written; the sweep counts below are the host twin's.", ""]
    try:
        for label, scenes in batches:
            X, Y = [s[0] for s in scenes], [s[1] for s in scenes]
            sweeps = [count_sweeps(twin, x, y) for x, y in zip(X, Y)]
            rows = [min(len(x), len(y)) for x, y in zip(X, Y)]
            lines.append(label)
            lines.append("  rows per step (the smaller side) %d .. %d; sweeps per step: median %d, min %d, max %d; sweeps / rows: median %.2f"
                         % (min(rows), max(rows), np.median(sweeps), min(sweeps), max(sweeps), np.median(np.array(sweeps) / np.array(rows))))
            if ctx is None:
                lines.append("")
                continue
            dev = DeviceBatch(ctx, X, Y)
            t_dev, t_host = [], []
            for _ in range(WARM + REPS):
                t0 = time.perf_counter()
                dev.call()
                t_dev.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                host = scipy_batch(X, Y)
                t_host.append(time.perf_counter() - t0)
            for got, x, y in zip(dev.steps(), X, Y):
                ref.hold(got, ref.reference(x, y, CUT, P))
            sd, sh = stats(t_dev), stats(t_host)
            lines.append("  (ms: median  min  max)")
            lines.append("  mht_gospa_steps, whole batch      %10.3f %10.3f %10.3f" % sd)
            lines.append("  SciPy on the host, whole batch    %10.3f %10.3f %10.3f" % sh)
            lines.append("  host / device (medians)           %10.1f" % (sh[0] / sd[0]))
            lines.append("  batch time over its steps %.1f us, batch time per sweep of the batch's longest step %.2f us (its %d sweeps bound the launch: one wavefront per step)"
                         % (sd[0] * 1e3 / len(X), sd[0] * 1e3 / max(sweeps), max(sweeps)))
            lines.append("  every step meets the tests' criterion against the reference (counts and matches exact)")
            lines.append("")
    finally:
        if ctx is not None:
            ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "gospa_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
