"""Development: what step 7 (the lifted 4-state M-of-N initiator, Tracker(..., useInitiator=True, liftBirths=True)) costs a constant-turn forest.

  ab [timed scans per run, default 100] [rounds, default 4]
      BASELINE config 5 as the bench streams it (2 000 preinitialised CT targets, ~2 000 measurements per scan, N = 6): (a) initiator off
      against (b) lifted initiator on, alternated run by run, each run timed over its scans behind N + 2 warm-up scans (streamed, nothing looked at)
  trace [timed scans, default 60]
      (b) only, for `rocprofv3 --kernel-trace --stats` (a run of its own): where step 7 lands
  stagger [targets, default 600] [per scan, default 150]
      (c) an empty CT tracker and targets that enter over several scans, at most `per scan` at a time: how many it brings up, scan by scan"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from pymht_amd.tracker import Tracker
from pymht_amd.pyTarget import Target
from pymht_amd.models import ct
from pymht_amd.utils.classDefinitions import MeasurementList
from pymht_amd.utils.scenario import make_config

LAMBDA_NU, ETA2 = 1e-4, 5.99      # bench.py's


def cfg5_run(sc, lifted, n_warm):
    kw = dict(useInitiator=True, liftBirths=True) if lifted else dict(useInitiator=False)
    trk = Tracker(ct, sc["period"], sc["lambda_phi"], LAMBDA_NU, P_d=sc["P_d"], N=sc["N"], eta2=ETA2, maxTargets=2304, maxNodes=1 << 20,
                  maxMeasurements=2048, **kw)
    x6 = np.concatenate([sc["x0"], np.zeros((len(sc["x0"]), 2))], axis=1)
    trk._add_targets([Target(sc["t0"], None, x.copy(), ct.P0, status="preinitialized") for x in x6])
    lists = [MeasurementList(float(t), z) for z, t in zip(sc["scans"], sc["times"])]
    try:
        for m in lists[:n_warm]:
            trk.addMeasurementList(m)
        trk.synchronize()
        t0 = time.perf_counter()
        for m in lists[n_warm:]:
            trk.addMeasurementList(m)
        trk.synchronize()
        dt = time.perf_counter() - t0
        return (len(lists) - n_warm) / dt, trk.nTargets
    finally:
        trk.close()


def ab(n_timed, rounds):
    res = {False: [], True: []}
    for r in range(rounds):
        sc = make_config("cfg5", seed=1234 + r, n_scans=8 + n_timed, confine=True)
        for lifted in ((False, True) if r % 2 == 0 else (True, False)):
            rate, nT = cfg5_run(sc, lifted, 8)
            res[lifted].append(rate)
            print("round %d %-22s %8.1f scans/s  (%d timed scans, %d targets at the end)" % (r, "(b) lifted initiator" if lifted else "(a) no initiator", rate, n_timed, nT), flush=True)
    a, b = np.array(res[False]), np.array(res[True])
    print("(a) no initiator      median %8.1f scans/s  (%s)" % (np.median(a), " ".join("%.0f" % v for v in a)))
    print("(b) lifted initiator  median %8.1f scans/s  (%s)" % (np.median(b), " ".join("%.0f" % v for v in b)))
    print("step 7 costs %.1f us per scan (median rates; %d x %d timed scans per mode)" % (1e6 * (1 / np.median(b) - 1 / np.median(a)), rounds, n_timed))


def stagger(n_tgt, per_scan, period=2.5, seed=7):
    rng = np.random.default_rng(seed)
    radius = 8000.0
    n_scans = -(-n_tgt // per_scan) + 8
    start = np.repeat(np.arange(n_tgt // per_scan + 1), per_scan)[:n_tgt]
    r = radius * 0.8 * np.sqrt(rng.uniform(size=n_tgt))
    th = rng.uniform(0, 2 * np.pi, n_tgt)
    pos = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    spd, hd = rng.uniform(3.0, 15.0, n_tgt), rng.uniform(0, 2 * np.pi, n_tgt)
    w = np.where(rng.uniform(size=n_tgt) < 0.3, rng.choice([-1.0, 1.0], n_tgt) * rng.uniform(0.02, 0.08, n_tgt), 0.0)
    vel = np.stack([spd * np.cos(hd), spd * np.sin(hd)], axis=1)
    lam = 2e-7
    trk = Tracker(ct, period, lam, LAMBDA_NU, P_d=0.9, N=4, eta2=ETA2, useInitiator=True, liftBirths=True, maxTargets=2048, maxNodes=1 << 19,
                  maxMeasurements=2048)
    try:
        for k in range(n_scans):
            live = start <= k
            c, s = np.cos(w * period), np.sin(w * period)
            vel = np.stack([c * vel[:, 0] - s * vel[:, 1], s * vel[:, 0] + c * vel[:, 1]], axis=1)
            pos = pos + period * vel
            seen = live & (rng.uniform(size=n_tgt) <= 0.9)
            n_cl = rng.poisson(lam * np.pi * radius ** 2)
            rc, tc = radius * np.sqrt(rng.uniform(size=n_cl)), rng.uniform(0, 2 * np.pi, n_cl)
            z = np.concatenate([pos[seen] + rng.normal(0, 2.5, (int(seen.sum()), 2)), np.stack([rc * np.cos(tc), rc * np.sin(tc)], axis=1)])
            rng.shuffle(z, axis=0)
            trk.addMeasurementList(MeasurementList(1000.0 + (k + 1) * period, np.ascontiguousarray(z, np.float32)))
            print("scan %2d: %4d targets present, %4d measurements, tracker holds %4d targets" % (k + 1, int(live.sum()), len(z), trk.nTargets), flush=True)
    finally:
        trk.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
    if mode == "ab":
        ab(int(sys.argv[2]) if len(sys.argv) > 2 else 100, int(sys.argv[3]) if len(sys.argv) > 3 else 4)
    elif mode == "trace":
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 60
        rate, nT = cfg5_run(make_config("cfg5", seed=1234, n_scans=8 + n, confine=True), True, 8)
        print("(b) lifted initiator %.1f scans/s over %d scans, %d targets" % (rate, n, nT))
    elif mode == "stagger":
        stagger(int(sys.argv[2]) if len(sys.argv) > 2 else 600, int(sys.argv[3]) if len(sys.argv) > 3 else 150)
