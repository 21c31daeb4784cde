"""What the Monte-Carlo ZONE engine costs (evaluation.mc_zone_encounters -> mht_mc_zone_encounters), written to
profiles/mc_zone_cost.txt.

  python tools/mc_zone_cost.py [--out FILE] [--quick]

Shape: tools/mc_cost.py's headline forest (13 000 leaves in 500 targets, models/pv, four states; the traffic lies in a square of
+-4 km and travels 900 m at most), K = 24 steps of 2.5 s, S = 4 096 particles, at three zone sets:
  Z = 1    a square of 4 vertices in the middle of the traffic
  Z = 16   64-gons of 250 m radius on a 4 x 4 grid of 2 km pitch, 64 vertices each: few zones near any target (FAR) -- and the same
           16 64-gons blown up about the origin until each one's box holds all the traffic (ON THE TRAFFIC): the same vertices to
           stage and the same edges per zone, and no wavefront can skip a zone.  The difference is what the skip saves
  Z = 32   32-gons, 1 024 vertices in all, every box over all the traffic
One process, one context; a time is the whole call as a caller sees it -- upload, three launches, download, the host's figures --
after warm-up calls, as median (min .. max) over the repeats.  Next to every figure stands the own-ship engine's call
(evaluation.mc_encounters, unchanged here) with G = Z own paths on the same leaves at the same S, measured in the same run.  Then the
NumPy reference (tests/mc_zone_ref.py) at Z = 1 and S = 1 024, its counts compared with the device's.  No ratio is fixed in advance: the
file records what was found.  Without a device the file says NOT YET MEASURED and holds the reference's time alone."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mc_cost      # noqa: E402  (the forest, the matrices and the own paths of the own-ship tool)
from mc_pair_cost import timed      # noqa: E402

K, DT, RADIUS = mc_cost.K, mc_cost.DT, mc_cost.RADIUS


def gon(n, r, centre, rot=0.1):
    a = rot + 2.0 * np.pi * np.arange(n) / n
    return np.asarray(centre, dtype=np.float64) + r * np.stack([np.cos(a), np.sin(a)], axis=1)


def zone_sets():
    grid = [(-3000.0 + 2000.0 * i, -3000.0 + 2000.0 * j) for i in range(4) for j in range(4)]
    return [("Z  1,    4 vertices, in the traffic", [np.array([(-1000.0, -1000.0), (1000.0, -1000.0), (1000.0, 1000.0), (-1000.0, 1000.0)])]),
            ("Z 16, 1024 vertices, FAR (4 x 4 grid)", [gon(64, 250.0, c) for c in grid]),
            ("Z 16, 1024 vertices, ON THE TRAFFIC", [gon(64, 7000.0 + 10.0 * z, (0.0, 0.0)) for z in range(16)]),
            ("Z 32, 1024 vertices, ON THE TRAFFIC", [gon(32, 7000.0 + 10.0 * z, (0.0, 0.0)) for z in range(32)])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_zone_cost.txt"))
    ap.add_argument("--quick", action="store_true", help="a small forest: a check of the tool itself")
    a = ap.parse_args()
    import torch
    from pymht_amd import evaluation
    from pymht_amd.models import pv
    import mc_zone_ref
    have_gpu = torch.cuda.is_available()
    leaves, targets, S = (260, 10, 1024) if a.quick else (13000, 500, 4096)
    x, P, tg, w = mc_cost.batch(pv, leaves, targets, 7)
    Phi, Q, _ = mc_cost.matrices(pv)
    sets = zone_sets()
    lines = ["Monte-Carlo guard zones (tools/mc_zone_cost.py) on %s; %d leaves in %d targets, models/pv, K = %d steps of %.1f s, S = %d particles"
             % (torch.cuda.get_device_name(0) if have_gpu else "NO DEVICE", leaves, targets, K, DT, S),
             "time of evaluation.mc_zone_encounters, whole call, ms: median (min .. max) over n calls after 2 warm-up calls;",
             "`own ship` is evaluation.mc_encounters with G = Z own paths on the same leaves at the same S, in this run", ""]
    small = None
    if have_gpu:
        from pymht_amd.device import Context
        ctx = Context(0, nx=4)
        try:
            kw = dict(particles=S, seed=1, transition="linear", ctx=ctx)
            med = {}
            for label, zones in sets:
                Z = len(zones)
                out, ts = timed(lambda: evaluation.mc_zone_encounters(x, P, tg, w, Phi, Q, K, DT, zones, **kw))
                own = mc_cost.paths(Z)
                _, to = timed(lambda: evaluation.mc_encounters(x, P, tg, w, Phi, Q, K, DT, RADIUS, own, **kw))
                med[label] = float(np.median(ts))
                rate = float(targets) * S * K / np.median(ts) / 1e6
                lines.append("  %-38s %9.2f (%9.2f .. %9.2f)  n %2d   %.2f G particle-steps/s, %.2f G zone-particle-steps/s   own ship, G %2d: %9.2f (%9.2f .. %9.2f)  n %2d   "
                             "zones / own ship %.2f   pEver > 0 in %d of %d cells"
                             % (label, np.median(ts), min(ts), max(ts), len(ts), rate, rate * Z, Z, np.median(to), min(to), max(to), len(to),
                                np.median(ts) / np.median(to), int((out["ever"] > 0).sum()), out["ever"].size))
            far, near = med[sets[1][0]], med[sets[2][0]]
            lines += ["", "the skip of a far zone: the 16 64-gons FAR take %.2f ms, the same 16 64-gons ON THE TRAFFIC %.2f ms: the skip saves %.0f %% of the call"
                      % (far, near, 100.0 * (near - far) / near)]
            small = evaluation.mc_zone_encounters(x, P, tg, w, Phi, Q, K, DT, sets[0][1], particles=1024, seed=1, transition="linear", ctx=ctx)
        finally:
            ctx.close()
    else:
        lines += ["NOT YET MEASURED on the device: no GPU was visible where this file was written; the NumPy reference's time below stands alone.", ""]
    first, cdf, order = (small["first"], small["cdf"], small["order"]) if small is not None else (None, None, None)
    if small is None:      # (the grouping evaluation.mc_zone_encounters would use: its host half needs no device)
        order = np.argsort(tg, kind="stable")
        first = np.append(np.unique(tg[order], return_index=True)[1], len(tg)).astype(np.int32)
        cdf = np.zeros(len(tg))
        for t in range(len(first) - 1):
            ww = w[order[first[t]:first[t + 1]]]
            cdf[first[t]:first[t + 1]] = np.cumsum(ww / ww.sum())
            cdf[first[t + 1] - 1] = 1.0
    sc = dict(x=x[order], P=P[order], first=first, cdf=cdf, Phi=Phi, Q=Q, own=None, ct=False, K=K, dt=DT, R=RADIUS, S=1024, seed=1)
    t0 = time.perf_counter()
    want = mc_zone_ref.encounters(sc, sets[0][1])
    t_ref = time.perf_counter() - t0
    verdict = "no device to compare with"
    if small is not None:
        same = all(np.array_equal(want[k], small[k]) for k in mc_zone_ref.COUNTS)
        verdict = "its counts %s the device's" % ("equal" if same else "DIFFER from")
    lines += ["", "NumPy reference (tests/mc_zone_ref.py), Z 1, S 1024: %.1f s; %s (%d borderline particles)" % (t_ref, verdict, want["border"])]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
