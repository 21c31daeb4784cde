"""What the Monte-Carlo PAIR engine costs (evaluation.mc_pair_encounters -> mht_mc_pair_encounters), written to
profiles/mc_pair_cost.txt.

  python tools/mc_pair_cost.py [--out FILE] [--quick]

Shapes: tools/mc_cost.py's forests -- the headline's (13 000 leaves in 500 targets, models/pv, four states) and config 5's (100 000
leaves in 2 000 targets, models/ct, six states, the constant-turn walk) --, K = 24 steps of 2.5 s, S of 1 024 and 4 096 particles, R = 200 m;
the pairs of a 2 km screen (evaluation.mc_pair_screen over the horizon) and, for the headline, all 124 750 pairs.  One process, one
context per model; a time is the whole call as a caller sees it -- upload, three launches, download, the host's figures -- after
warm-up calls, as median (min .. max) over the repeats.  The rate is PAIR-particle-steps per second; one pair-particle-step is two
particle-steps, and next to every figure stands the own-ship engine's G = 1 call (tools/mc_cost.py's) at the same S, re-measured in
the same run.  Then the NumPy reference (tests/mc_pair_ref.py) at the smallest case, its counts compared with the device's."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mc_cost      # noqa: E402  (the forests, the matrices and the own paths of the own-ship tool)

K, DT, RADIUS, SCREEN = mc_cost.K, mc_cost.DT, mc_cost.RADIUS, 2000.0


def timed(call):
    """(the first call's result, the times in ms of n calls after two warm-up calls)"""
    t0 = time.perf_counter()
    out = call()
    once = time.perf_counter() - t0
    call()
    n = 20 if once < 0.05 else (7 if once < 0.5 else 3)
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_pair_cost.txt"))
    ap.add_argument("--quick", action="store_true", help="small shapes: a check of the tool itself")
    a = ap.parse_args()
    import torch
    from pymht_amd import evaluation
    from pymht_amd.device import Context
    from pymht_amd.models import ct, pv
    import mc_pair_ref
    lines = ["Monte-Carlo encounters between pairs of targets (tools/mc_pair_cost.py) on %s; K = %d steps of %.1f s, R = %.0f m"
             % (torch.cuda.get_device_name(0), K, DT, RADIUS),
             "time of evaluation.mc_pair_encounters, whole call, ms: median (min .. max) over n calls after 2 warm-up calls;",
             "a pair-particle-step is two particle-steps; `own ship` is evaluation.mc_encounters with G = 1 at the same S, in this run", ""]
    shapes = [("headline: 13 000 leaves in 500 targets, models/pv", pv, 13000, 500, True), ("config 5: 100 000 leaves in 2 000 targets, models/ct", ct, 100000, 2000, False)]
    if a.quick:
        shapes = [("quick pv", pv, 260, 10, True), ("quick ct", ct, 500, 10, False)]
    first = None
    for label, model, leaves, targets, every in shapes:
        x, P, tg, w = mc_cost.batch(model, leaves, targets, 7)
        Phi, Q, turning = mc_cost.matrices(model)
        transition = "ct" if turning else "linear"
        t0 = time.perf_counter()
        near = evaluation.mc_pair_screen(x, tg, w, K * DT, SCREEN)
        t_screen = (time.perf_counter() - t0) * 1e3
        cases = [("screen %.0f m" % SCREEN, near)]
        if every:
            i, j = np.triu_indices(targets, 1)
            cases.append(("all pairs", np.stack([i, j], axis=1)))
        ctx = Context(0, nx=x.shape[1])
        try:
            lines.append("%s; mc_pair_screen keeps %d of %d pairs in %.1f ms on the host" % (label, len(near), targets * (targets - 1) // 2, t_screen))
            own = mc_cost.paths(1)
            for S in (1024, 4096):
                _, ts = timed(lambda: evaluation.mc_encounters(x, P, tg, w, Phi, Q, K, DT, RADIUS, own, particles=S, seed=1, transition=transition, ctx=ctx))
                own_rate = float(targets) * S * K / np.median(ts) / 1e6
                lines.append("  S %5d  own ship, G 1        %9.2f (%9.2f .. %9.2f)  n %2d   %.2f G particle-steps/s" % (S, np.median(ts), min(ts), max(ts), len(ts), own_rate))
                for what, pairs in cases:
                    out, ts = timed(lambda: evaluation.mc_pair_encounters(x, P, tg, w, Phi, Q, K, DT, RADIUS, pairs, particles=S, seed=1, transition=transition, ctx=ctx))
                    rate = float(len(pairs)) * S * K / np.median(ts) / 1e6
                    lines.append("  S %5d  %-14s %7d pairs  %9.2f (%9.2f .. %9.2f)  n %2d   %.2f G pair-particle-steps/s = %.2f G particle-steps/s (%.2f x own ship)   pEver > 0 in %d pairs"
                                 % (S, what, len(pairs), np.median(ts), min(ts), max(ts), len(ts), rate, 2 * rate, 2 * rate / own_rate, int((out["ever"] > 0).sum())))
                    if first is None:
                        first = (label, x, P, Phi, Q, turning, S, pairs, out)
            lines.append("")
        finally:
            ctx.close()
    label, x, P, Phi, Q, turning, S, pairs, out = first
    order = out["order"]
    sc = dict(x=x[order], P=P[order], first=out["first"], cdf=out["cdf"], Phi=Phi, Q=Q, own=None, ct=turning, K=K, dt=DT, R=RADIUS, S=S, seed=1)
    t0 = time.perf_counter()
    want = mc_pair_ref.encounters(sc, np.searchsorted(out["targets"], pairs))
    t_ref = time.perf_counter() - t0
    same = all(np.array_equal(want[k], out[k]) for k in ("within", "firstAt", "ever", "valid", "status"))
    lines.append("NumPy reference (tests/mc_pair_ref.py), %s, %d pairs, S %d: %.1f s; its counts %s the device's (%d borderline pair-particle-steps)"
                 % (label.split(":")[0], len(pairs), S, t_ref, "equal" if same else "DIFFER from", want["border"]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
