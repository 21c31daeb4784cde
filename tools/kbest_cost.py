"""What listing the k best global hypotheses per cluster costs on the device, in ONE process (sibling of tools/trial_hyp_cost.py).

  python tools/kbest_cost.py [--out FILE]      (default FILE: profiles/kbest_cost.txt)
      a headline-size leaf set -- about 13 000 leaves over 500 targets, window keys of 4 levels, the targets in groups of 1 .. 6 that
      share plots -- prepared once on the host (evaluation.k_best_prep), then mht_kbest_hypotheses on its clusters for k = 1, 8 and 64:
        the launch's time around the call and mht_synchronize (the two fills and the one kernel; inputs resident), 3 warm-up rounds and
        20 rounds alternating between the three k: median, min, max
        node counts (sibling tests): total, largest cluster; the statuses
        the Python reference (tests/kbest_ref.branch_and_bound) on the same clusters, k = 8, once, and that its lists are the device's
      accuracy: the worst ratio of prob and the marginals to the bound (2 K + 64) eps over the cases of tests/test_kbest_gpu.py, both builds
      registers of the kernel, from the compiler's report (where hipcc is there)
      Without a device the file says NOT YET MEASURED and holds the register report alone."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

L_TOTAL, T_TOTAL, LEVELS = 13000, 500, 4
WARM, REPS = 3, 20
KS = (1, 8, 64)


def make_leaves(seed=7):
    """(cost [L], target [L], rows [L, LEVELS]): the targets in groups of 1 .. 6, a group's leaves draw their plot of every level from
    the group's pool of 2 plots per member (or none, 3 times in 10); cnllr-like costs spread over 15 inside a target"""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, L_TOTAL), T_TOTAL - 1, replace=False))
    seg = np.concatenate([[0], cuts, [L_TOTAL]])
    target = np.repeat(np.arange(T_TOTAL), np.diff(seg)).astype(np.int32)
    group, base, size = np.zeros(T_TOTAL, dtype=np.int64), np.zeros(T_TOTAL, dtype=np.int64), np.zeros(T_TOTAL, dtype=np.int64)
    t, g, b = 0, 0, 1
    while t < T_TOTAL:
        n = min(int(rng.integers(1, 7)), T_TOTAL - t)
        group[t:t + n], base[t:t + n], size[t:t + n] = g, b, 2 * n
        t, g, b = t + n, g + 1, b + 2 * n
    plot = base[target][:, None] + (rng.random((L_TOTAL, LEVELS)) * size[target][:, None]).astype(np.int64)
    rows = np.where(rng.random((L_TOTAL, LEVELS)) < 0.3, -1, (np.arange(LEVELS)[None, :] << 24) | plot).astype(np.int64)
    cost = rng.uniform(0.0, 15.0, L_TOTAL) + rng.uniform(-40.0, 40.0, T_TOTAL)[target]
    return cost, target, rows


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def measure(lines):
    import torch
    import kbest_ref as ref
    from pymht_amd import _lib, evaluation
    from pymht_amd.device import Context
    cost, target, rows = make_leaves()
    t0 = time.perf_counter()
    gp, cp, ct, local = evaluation.k_best_prep(target, rows)
    t_prep = time.perf_counter() - t0
    L, T, nC, D = len(cost), len(gp) - 1, len(cp) - 1, rows.shape[1]
    sizes = np.diff(cp)
    cols = np.array([int(sum(gp[t + 1] - gp[t] for t in ct[cp[c]:cp[c + 1]])) for c in range(nC)])
    lines += ["%d leaves over %d targets, keys of %d levels: %d clusters (host preparation %.1f ms), 1 .. %d targets and up to %d leaves a cluster, %d clusters of"
              % (L, T, D, nC, t_prep * 1e3, int(sizes.max()), int(cols.max()), int((sizes > 1).sum())), "more than one target.", ""]
    ctx = Context(0)
    try:
        lib, dev = ctx.lib, ctx.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        gp_d, cp_d, ct_d, rw_d, c_d = up(gp), up(cp), up(ct), up(local), up(cost)
        outs = {}
        for k in KS:
            outs[k] = (torch.empty((3, nC), dtype=torch.int32, device=dev), torch.empty((2, k, nC), dtype=torch.float64, device=dev),
                       torch.empty((k, T), dtype=torch.int32, device=dev), torch.empty(L, dtype=torch.float64, device=dev),
                       torch.empty(int(lib.mht_kbest_work_bytes(L, T, nC, D, k)), dtype=torch.uint8, device=dev))
        torch.cuda.synchronize(dev)

        def call(k):
            ints, hyp, sel, mar, work = outs[k]
            _lib.check(lib.mht_kbest_hypotheses(ctx.handle, L, T, nC, D, k, 1 << 20, gp_d.data_ptr(), rw_d.data_ptr(), c_d.data_ptr(), cp_d.data_ptr(), ct_d.data_ptr(),
                                                ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), hyp[0].data_ptr(), hyp[1].data_ptr(), sel.data_ptr(),
                                                mar.data_ptr(), work.data_ptr(), work.numel()), lib)
            _lib.check(lib.mht_synchronize(ctx.handle), lib)
        ts = {k: [] for k in KS}
        for _ in range(WARM + REPS):
            for k in KS:
                t0 = time.perf_counter()
                call(k)
                ts[k].append(time.perf_counter() - t0)
        lines.append("mht_kbest_hypotheses, inputs resident, around the call and the wait (ms: median  min  max), node counts, statuses:")
        for k in KS:
            ints = outs[k][0].cpu().numpy()
            lines.append("  k = %2d  %10.3f %10.3f %10.3f   nodes: %d in all, %d in the largest search; status 0 / 1 / 2 / 3: %s"
                         % ((k,) + stats(ts[k]) + (int(ints[2].sum()), int(ints[2].max()), np.bincount(ints[1], minlength=4).tolist())))
        ints, hyp, sel = outs[8][0].cpu().numpy(), outs[8][1].cpu().numpy(), outs[8][2].cpu().numpy()
        t0 = time.perf_counter()
        same = True
        for c in range(nC):
            tg = ct[cp[c]:cp[c + 1]]
            idx = np.concatenate([np.arange(gp[t], gp[t + 1]) for t in tg])
            want, _ = ref.branch_and_bound([int(gp[t + 1] - gp[t]) for t in tg], cost[idx], [[int(r) for r in rows[i] if r >= 0] for i in idx], 8)
            got = [(float(hyp[0, r, c]), tuple(int(sel[r, t] - gp[t]) for t in tg)) for r in range(int(ints[0, c]))]
            same = same and got == want
        lines += ["  the Python reference (recursive branch and bound, k = 8) over the same clusters, once: %.1f ms; its lists are the device's bit for bit: %s"
                  % ((time.perf_counter() - t0) * 1e3, "yes" if same else "NO"), ""]
    finally:
        ctx.close()


def accuracy_lines():
    import kbest_ref as ref
    import tempfile
    from test_kbest_gpu import call_seam
    from pymht_amd.device import Context
    out = ["Accuracy of prob and the marginals: the worst ratio of |device - truth| to (2 K + 64) eps truth, truth the np.longdouble fold of the device's own",
           "costs (criterion <= 1), over the cases of tests/kbest_ref.py:"]
    for lib_nx in (4, 6):
        ctx = Context(0, nx=lib_nx)
        try:
            worst = max(ref.hold_probabilities(c["label"], c["packed"], call_seam(ctx, c["packed"], c["K"]), c["K"]) for c in ref.cases())
            out.append("  %d-state build: %.3g" % (lib_nx, worst))
        finally:
            ctx.close()
    return out + [""]


def register_lines():
    lines = []
    try:
        import pathlib
        import tempfile
        import test_kbest_resources as res
        found = res.kbest_report(pathlib.Path(tempfile.mkdtemp()), [])
        lines.append("Registers of the kernel (compiler's report, gfx950, the library's flags); its LDS is dynamic, %d B at the limits:" % res.LDS_AT_THE_LIMITS)
        for k, v in sorted(found.items()):
            lines.append("  %-60s VGPR %3d  AGPR %3d  scratch %d B  static LDS %d B  spilled: %d vector, %d scalar"
                         % (k, v["vgpr"], v["agpr"], v["scratch"], v["lds"], v["spill"], v["sgpr_spill"]))
    except BaseException as exc:      # (no hipcc where the tool runs, or pytest's skip for the same reason)
        lines.append("Registers of the kernel: the compiler's report could not be made here (%s)" % type(exc).__name__)
    return lines


def main(out_path):
    lines = ["The k best global hypotheses per cluster (mht_kbest_hypotheses: one wavefront per cluster walks a depth-first branch and bound, 64 sibling",
             "columns tested per step against the used-row table in LDS; csrc/mht_kbest.h).  No speed figure is promised: this file is where it is recorded.", ""]
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        lines += ["NOT YET MEASURED on the device: no GPU was visible where this file was written; the register report below is the compiler's.", ""]
    else:
        measure(lines)
        lines += accuracy_lines()
    lines += register_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "kbest_cost.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
