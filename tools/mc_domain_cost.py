"""What the Monte-Carlo SHIP-DOMAIN engine costs (evaluation.mc_domain_encounters -> mht_mc_domain_encounters), written to
profiles/mc_domain_cost.txt.

  python tools/mc_domain_cost.py [--out FILE] [--quick]

Shape: tools/mc_cost.py's headline forest (13 000 leaves in 500 targets, models/pv, four states; the traffic lies in a square of
+-4 km and travels 900 m at most), K = 24 steps of 2.5 s, S = 4 096 particles; the own ship of tools/mc_cost.py (at the origin, 8 m/s
due east) with that tool's candidate paths, so that FEW TARGETS ARE NEAR THE OWN SHIP, as at sea.  Cases:
  1 x 16    one domain of 8 vertices (410 m long, 180 m wide) on 16 paths, next to evaluation.mc_encounters with the same 16 paths
  2 x 16    that domain and an outer one of 8 vertices (1 020 m long)
  1 x 64    the first domain on 64 paths, next to evaluation.mc_encounters with the same 64 paths
  64 vertices   a 64-gon of the first domain's size on 16 paths: the 8-vertex figure is case 1 x 16
  the skip  the same 64-gon blown up until its box holds all the traffic on every path: the same vertices to stage, the same edges,
            and no wavefront can skip a cell.  The difference is what the skip saves
  config 5  100 000 constant-turn leaves in 2 000 targets (models/ct, six states), 1 x 16
One process, one context per model; a time is the whole call as a caller sees it -- upload, three launches, download, the host's
figures -- after two warm-up calls, as median (min .. max) over the repeats; where two calls stand next to each other they were timed
ALTERNATELY in the same run.  Then the NumPy reference (tests/mc_domain_ref.py) for the smallest case, 1 x 16 at S = 1 024, its
counts compared with the device's.  No threshold is set: the file records what was found, and says which figures were NOT measured.
The kernels' register and LDS figures are the compiler's (tests/test_mc_domain_resources.py reads them from the compiled object)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mc_cost      # noqa: E402  (the forest, the matrices and the own ship of the own-ship tool)

K, DT, RADIUS, OWN, TURN = mc_cost.K, mc_cost.DT, mc_cost.RADIUS, mc_cost.OWN, mc_cost.TURN

# bow-up: (to starboard, ahead)
INNER = np.array([(-60, -80), (90, -80), (110, 60), (100, 180), (20, 330), (-40, 240), (-70, 120), (-70, 0)], dtype=np.float64)
OUTER = np.array([(-220, -200), (330, -200), (380, 100), (360, 400), (60, 820), (-120, 620), (-260, 300), (-260, 0)], dtype=np.float64)


def gon(n, r, centre, rot=0.1):
    a = rot + 2.0 * np.pi * np.arange(n) / n
    return np.asarray(centre, dtype=np.float64) + r * np.stack([np.cos(a), np.sin(a)], axis=1)


def candidates(G):
    """tools/mc_cost.paths' candidates"""
    return [(0.0, 1.0, 0.0)] + [((g - G / 2) * 0.1, 1.0, 5.0) for g in range(1, G)]


def timed_both(first, second=None):
    """(the results, the times in ms of n calls each after two warm-up calls each); two calls are timed alternately"""
    calls = [first] + ([second] if second is not None else [])
    outs, once = [], 0.0
    for call in calls:
        t0 = time.perf_counter()
        outs.append(call())
        once = max(once, time.perf_counter() - t0)
        call()
    n = 20 if once < 0.05 else (7 if once < 0.5 else 3)
    ts = [[] for _ in calls]
    for _ in range(n):
        for i, call in enumerate(calls):
            t0 = time.perf_counter()
            call()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return outs, ts


def fmt(ts):
    return "%9.2f (%9.2f .. %9.2f)  n %2d" % (np.median(ts), min(ts), max(ts), len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_domain_cost.txt"))
    ap.add_argument("--quick", action="store_true", help="a small forest: a check of the tool itself")
    a = ap.parse_args()
    import torch
    from pymht_amd import evaluation
    from pymht_amd.models import ct, pv
    import mc_domain_ref
    import test_mc_domain_resources as res
    have_gpu = torch.cuda.is_available()
    leaves, targets, S = (260, 10, 1024) if a.quick else (13000, 500, 4096)
    leaves5, targets5 = (520, 20) if a.quick else (100000, 2000)
    x, P, tg, w = mc_cost.batch(pv, leaves, targets, 7)
    Phi, Q, _ = mc_cost.matrices(pv)
    poses = {G: evaluation.mc_own_poses(OWN, candidates(G), TURN, K, DT) for G in (16, 64)}
    round64, wide64 = gon(64, 200.0, (10.0, 120.0)), gon(64, 14000.0, (0.0, 0.0))
    lines = ["Monte-Carlo ship domains (tools/mc_domain_cost.py) on %s; %d leaves in %d targets, models/pv, K = %d steps of %.1f s, S = %d particles"
             % (torch.cuda.get_device_name(0) if have_gpu else "NO DEVICE", leaves, targets, K, DT, S),
             "time of evaluation.mc_domain_encounters, whole call, ms: median (min .. max) over n calls after 2 warm-up calls;",
             "`own ship` is evaluation.mc_encounters (a disc of %.0f m) on the same paths and leaves at the same S, timed alternately with the domain call" % RADIUS, ""]
    small = None
    if have_gpu:
        from pymht_amd.device import Context
        ctx = Context(0, nx=4)
        try:
            kw = dict(particles=S, seed=1, transition="linear", ctx=ctx)
            dom = lambda doms, G: (lambda: evaluation.mc_domain_encounters(x, P, tg, w, Phi, Q, K, DT, doms, poses[G], **kw))
            disc = lambda G: (lambda: evaluation.mc_encounters(x, P, tg, w, Phi, Q, K, DT, RADIUS, np.ascontiguousarray(poses[G][:, :, :2]), **kw))
            med = {}
            for label, doms, G, beside in (("1 x 16,  8 vertices", [INNER], 16, True), ("2 x 16, 16 vertices", [INNER, OUTER], 16, False),
                                           ("1 x 64,  8 vertices", [INNER], 64, True), ("1 x 16, 64 vertices", [round64], 16, False),
                                           ("1 x 16, 64 vertices, ALL TRAFFIC IN THE BOX", [wide64], 16, False)):
                outs, ts = timed_both(dom(doms, G), disc(G) if beside else None)
                med[label] = float(np.median(ts[0]))
                ever = outs[0]["ever"]
                rate = float(targets) * S * K / np.median(ts[0]) / 1e6
                line = "  %-44s %s   %.2f G particle-steps/s, %.2f G cell-particle-steps/s   pEver > 0 in %d of %d (cell, target)s" % (
                    label, fmt(ts[0]), rate, rate * len(doms) * G, int((ever > 0).sum()), ever.size)
                if beside:
                    line += "\n  %-44s %s   domain / own ship %.2f" % ("    own ship, G %d" % G, fmt(ts[1]), np.median(ts[0]) / np.median(ts[1]))
                lines.append(line)
            far, near = med["1 x 16, 64 vertices"], med["1 x 16, 64 vertices, ALL TRAFFIC IN THE BOX"]
            lines += ["", "the skip of a far cell: the 64-gon about the own ship takes %.2f ms, the same 64-gon with all the traffic in its box %.2f ms: the skip saves "
                      "%.0f %% of that call" % (far, near, 100.0 * (near - far) / near)]
            small = evaluation.mc_domain_encounters(x, P, tg, w, Phi, Q, K, DT, [INNER], poses[16], particles=1024, seed=1, transition="linear", ctx=ctx)
        finally:
            ctx.close()
        x5, P5, tg5, w5 = mc_cost.batch(ct, leaves5, targets5, 7)
        Phi5, Q5, _ = mc_cost.matrices(ct)
        ctx = Context(0, nx=6)
        try:
            kw = dict(particles=S, seed=1, transition="ct", ctx=ctx)
            outs, ts = timed_both(lambda: evaluation.mc_domain_encounters(x5, P5, tg5, w5, Phi5, Q5, K, DT, [INNER], poses[16], **kw),
                                  lambda: evaluation.mc_encounters(x5, P5, tg5, w5, Phi5, Q5, K, DT, RADIUS, np.ascontiguousarray(poses[16][:, :, :2]), **kw))
            rate = float(targets5) * S * K / np.median(ts[0]) / 1e6
            lines += ["", "config 5: %d leaves in %d targets, models/ct (constant turn, six states), S = %d" % (leaves5, targets5, S),
                      "  %-44s %s   %.2f G particle-steps/s" % ("1 x 16,  8 vertices", fmt(ts[0]), rate),
                      "  %-44s %s   domain / own ship %.2f" % ("    own ship, G 16", fmt(ts[1]), np.median(ts[0]) / np.median(ts[1]))]
        finally:
            ctx.close()
    else:
        lines += ["NOT MEASURED on the device: no GPU was visible where this file was written -- no time, no rate and no share of the skip; the NumPy",
                  "reference's time below stands alone.", ""]
    lines += ["", "the kernels (csrc/mht_mc_domain.hip), as the compiler reports them for gfx950 (tests/test_mc_domain_resources.py; read when written):"]
    lines += ["  %-34s %3d vector registers, no scratch, no spill, no accumulator registers" % (k + "E", v[0]) for k, v in res.KERNELS.items()]
    lines += ["  static LDS %d bytes at four states and %d at six, of which the counts at the limits' size are %d" % (res.LDS_READ[4], res.LDS_READ[6], res.COUNTS_BYTES)]
    first, cdf, order = (small["first"], small["cdf"], small["order"]) if small is not None else (None, None, None)
    if small is None:      # (the grouping evaluation.mc_domain_encounters would use: its host half needs no device)
        order = np.argsort(tg, kind="stable")
        first = np.append(np.unique(tg[order], return_index=True)[1], len(tg)).astype(np.int32)
        cdf = np.zeros(len(tg))
        for t in range(len(first) - 1):
            ww = w[order[first[t]:first[t + 1]]]
            cdf[first[t]:first[t + 1]] = np.cumsum(ww / ww.sum())
            cdf[first[t + 1] - 1] = 1.0
    sc = dict(x=x[order], P=P[order], first=first, cdf=cdf, Phi=Phi, Q=Q, own=None, ct=False, K=K, dt=DT, R=RADIUS, S=1024, seed=1)
    t0 = time.perf_counter()
    want = mc_domain_ref.encounters(sc, [INNER], poses[16])
    t_ref = time.perf_counter() - t0
    verdict = "no device to compare with"
    if small is not None:
        same = all(np.array_equal(want[k], small[k]) for k in mc_domain_ref.COUNTS)
        verdict = "its counts %s the device's" % ("equal" if same else "DIFFER from")
    lines += ["", "NumPy reference (tests/mc_domain_ref.py), 1 x 16, 8 vertices, S 1024: %.1f s; %s (%d borderline particles)" % (t_ref, verdict, want["border"])]
    lines += ["", "NOT measured here: the walk kernel's time on its own (no profiler run: the figures above are whole calls with their uploads, the read-back of the poses",
              "and domains for the seam's checks, and the downloads), its memory traffic, and any shape beyond those listed.",
              "How to read the ratios: against a disc the walk pays, per (path, step), two transforms where the disc has two subtractions, per cell two ballots where the",
              "disc has one, and the edge loops of the (cell, target)s whose wavefronts are near the domain's box; a domain whose box is near more of the traffic, or that",
              "has more vertices, costs in proportion to both."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
