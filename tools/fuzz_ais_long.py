"""Development / campaign tool: AIS-aided fuzz cases with long N-scan windows (N in [8, 12]: 32-int path records) against the live oracle,
scan by scan (tests/ais_long_util.py::run_trace).  usage: fuzz_ais_long.py SEED0 COUNT [SECONDS: no case starts after that]"""
import os
import sys
import time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
from ais_long_util import run_trace
from pymht_amd._lib import MhtError, MHT_E_CAPACITY


def case(seed):
    rng = np.random.default_rng(seed)
    N = int(rng.integers(8, 13))
    scene = dict(T=int(rng.integers(1, 5)), radius=float(rng.uniform(150, 900)), lambda_phi=float(rng.choice([0.0, 1e-6, 1e-5])),
                 P_d=float(rng.uniform(0.8, 0.99)), period=float(rng.choice([1.0, 2.5, 4.0])), equipped=float(rng.choice([0.3, 0.6, 1.0])),
                 p_report=float(rng.choice([0.4, 0.8])), msg_every=int(rng.integers(2, 5)), n_scans=N + int(rng.integers(2, 7)))
    ais_init = bool(rng.uniform() < 0.5)
    desc = "seed %d: N=%d init=%d " % (seed, N, ais_init) + " ".join("%s=%.3g" % kv for kv in scene.items())
    t0 = time.time()
    try:
        n, deepest, nf, stop = run_trace(seed, N, ais_init, max_leaves=20000, budget_s=30.0, **scene)
    except AssertionError as e:
        return False, desc, "MISMATCH %s" % (e,)
    except MhtError as e:      # (a capacity the scene outgrew: reported, not a mismatch)
        if e.code != MHT_E_CAPACITY:
            raise
        return None, desc, "capacity: %s" % (str(e)[:160],)
    return True, desc, "scans %d%s deepest %s fused %d %.1fs" % (n, " (%s)" % stop if stop else "", deepest, nf, time.time() - t0)


if __name__ == "__main__":
    seed0, n = int(sys.argv[1]), int(sys.argv[2])      # (first seed, then count)
    deadline = time.time() + (float(sys.argv[3]) if len(sys.argv) > 3 else 1e9)
    bad = cap = done = 0
    for s in range(seed0, seed0 + n):
        if time.time() > deadline:
            break
        ok, desc, msg = case(s)
        done += 1
        bad += 1 if ok is False else 0
        cap += 1 if ok is None else 0
        print({True: "ok  ", False: "BAD ", None: "CAP "}[ok] + desc + " | " + msg, flush=True)
    print("cases %d bad %d capacity %d" % (done, bad, cap))
