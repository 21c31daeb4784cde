"""What the Monte-Carlo encounter engine costs (evaluation.mc_encounters -> mht_mc_encounters), written to profiles/mc_cost.txt.

  python tools/mc_cost.py [--out FILE] [--quick]

Shapes: the headline's (13 000 leaves in 500 targets, models/pv, four states) and config 5's (100 000 leaves in 2 000 targets, models/ct,
six states, the constant-turn walk), K = 24 steps of 2.5 s, S of 1 024, 4 096 and 65 536 particles per target, G of 1 and 16 own paths.
One process, one context per model; a time is the whole call as a caller sees it -- upload, three launches, download, the host's
figures -- after warm-up calls, as median / min / max over the repeats (fewer repeats where a call takes long; the count is written
next to the figures).  Then the NumPy reference (tests/mc_ref.py) on the same machine at the smallest shape, and, for models/pv, the
largest |pcMax - trial_manoeuvres' pc| / sePcMax over one-component targets at S = 65 536 -- the sampler against the Gaussian rule
where that rule applies.  pcMax is the LARGEST of K + 1 noisy shares, so it is biased upward, most where pc is a few particles' worth
and se sits at its floor of one particle; the per-step comparison without that bias is tests/test_mc_cpu.py's (within 4 se)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, DT, RADIUS, OWN, TURN = 24, 2.5, 200.0, np.array([0.0, 0.0, 8.0, 0.0]), 0.05


def batch(model, leaves, targets, seed):
    rng = np.random.default_rng(seed)
    nx = np.asarray(model.P0).shape[0]
    centre = np.zeros((targets, nx))
    centre[:, :2] = rng.uniform(-4000.0, 4000.0, (targets, 2))
    speed, head = rng.uniform(0, 15, targets), rng.uniform(0, 2 * np.pi, targets)
    centre[:, 2], centre[:, 3] = speed * np.cos(head), speed * np.sin(head)
    if getattr(model, "transition", None) == "ct":
        centre[:, 4] = rng.uniform(-0.02, 0.02, targets)
    tg = np.sort(np.concatenate([np.arange(targets), rng.integers(0, targets, leaves - targets)])).astype(np.int32)
    x = centre[tg]
    x[:, :2] += rng.normal(0.0, 30.0, (leaves, 2))
    x[:, 2:4] += rng.normal(0.0, 0.5, (leaves, 2))
    P = np.tile(np.asarray(model.P0, dtype=np.float64), (leaves, 1, 1))
    return x, P, tg, np.exp(-rng.uniform(0.0, 6.0, leaves))


def matrices(model):
    nx = np.asarray(model.P0).shape[0]
    widen = lambda m: np.asarray(m, dtype=np.float32).astype(np.float64).reshape(nx, nx)
    ct = getattr(model, "transition", None) == "ct"
    return (widen(model.Phi(DT, 0.0)) if ct else widen(model.Phi(DT))), widen(model.Q(DT)), ct


def paths(G):
    from pymht_amd import evaluation
    cand = [(0.0, 1.0, 0.0)] + [((g - G / 2) * 0.1, 1.0, 5.0) for g in range(1, G)]
    return evaluation.mc_own_paths(OWN, cand, TURN, K, DT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_cost.txt"))
    ap.add_argument("--quick", action="store_true", help="small shapes: a check of the tool itself")
    a = ap.parse_args()
    import torch
    from pymht_amd import evaluation
    from pymht_amd.device import Context
    from pymht_amd.models import ct, pv
    import mc_ref
    lines = ["Monte-Carlo encounters (tools/mc_cost.py) on %s; K = %d steps of %.1f s, R = %.0f m" % (torch.cuda.get_device_name(0), K, DT, RADIUS),
             "time of evaluation.mc_encounters, whole call, ms: median (min .. max) over n calls after 2 warm-up calls", ""]
    shapes = [("headline: 13 000 leaves in 500 targets, models/pv", pv, 13000, 500), ("config 5: 100 000 leaves in 2 000 targets, models/ct", ct, 100000, 2000)]
    if a.quick:
        shapes = [("quick pv", pv, 260, 10), ("quick ct", ct, 500, 10)]
    first = None
    for label, model, leaves, targets in shapes:
        x, P, tg, w = batch(model, leaves, targets, 7)
        Phi, Q, turning = matrices(model)
        ctx = Context(0, nx=x.shape[1])
        try:
            lines.append(label)
            for S in (1024, 4096, 65536):
                for G in (1, 16):
                    own = paths(G)
                    call = lambda: evaluation.mc_encounters(x, P, tg, w, Phi, Q, K, DT, RADIUS, own, particles=S, seed=1, transition="ct" if turning else "linear", ctx=ctx)
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
                    steps = float(targets) * S * K
                    lines.append("  S %6d  G %2d   %9.2f (%9.2f .. %9.2f)  n %2d   %.2f G particle-steps/s   pEver > 0 in %d of %d cells"
                                 % (S, G, np.median(ts), min(ts), max(ts), n, steps / np.median(ts) / 1e6, int((out["ever"] > 0).sum()), out["ever"].size))
                    if first is None:
                        first = (label, x, P, tg, w, Phi, Q, own, out)
            if model is pv:      # the sampler against the Gaussian rule, one-component targets
                lead = np.searchsorted(tg, np.arange(targets))
                own = paths(1)
                mc = evaluation.mc_encounters(x[lead], P[lead], np.arange(targets), np.ones(targets), Phi, Q, K, DT, RADIUS, own, particles=65536, seed=1, ctx=ctx)
                rule = evaluation.trial_manoeuvres(x[lead], P[lead], Phi, Q, K, DT, RADIUS, OWN, [(0.0, 1.0, 0.0)], TURN, ctx=ctx)
                ratio = np.abs(mc["pcMax"][0] - rule["pc"][0]) / mc["sePcMax"][0]
                lines.append("  against the Gaussian rule (trial_manoeuvres' pc), %d one-component targets, S 65536: largest |pcMax - pc| / se %.2f, %d targets with 1e-3 < pc < 0.999"
                             % (targets, float(np.nanmax(ratio)), int(((rule["pc"][0] > 1e-3) & (rule["pc"][0] < 0.999)).sum())))
            lines.append("")
        finally:
            ctx.close()
    label, x, P, tg, w, Phi, Q, own, out = first
    order = np.argsort(tg, kind="stable")
    t0 = time.perf_counter()
    want = mc_ref.encounters(x[order], P[order], out["first"], out["cdf"], Phi, Q, own, K, DT, RADIUS, 1024, 1)
    t_ref = time.perf_counter() - t0
    same = np.array_equal(want["within"], out["within"]) and np.array_equal(want["ever"], out["ever"])
    lines.append("NumPy reference (tests/mc_ref.py), %s, S 1024, G 1: %.1f s; its counts %s the device's (%d borderline pairs)"
                 % (label.split(":")[0], t_ref, "equal" if same else "DIFFER from", int(want["borderWithin"].sum())))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
