"""Development: what the N-scan window costs an AIS-aided forest, on a scene every window from 5 to 12 fits -- the headline scene's density
(cfg3: 500 targets in a 5 km disc) cut to 50 ships in a 1.58 km disc, 20 % of the ships equipped, messages on every third scan,
similar-state pruning on two scans of three (the tests' schedule, tests/ais_long_util.py).  The headline scene itself outgrows any node
pool from N = 8 on (2^N leaves per target, 500 targets).  Scans per second, timed from scan N + 2 (window full) to the end, radar only
(aisAided forest, no messages) and with messages (aisInitialization=False).
usage: ais_window_cost.py N [n_scans after the window is full, default 12] [log2 maxNodes, default 21]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from pymht_amd.tracker import Tracker
from pymht_amd.pyTarget import Target
from pymht_amd.models import pv
from pymht_amd.ais import AisMessage, AisMessageList
from pymht_amd.utils.classDefinitions import MeasurementList
from pymht_amd.utils.scenario import make_scenario, make_ais

N = int(sys.argv[1])
n_timed = int(sys.argv[2]) if len(sys.argv) > 2 else 12
max_nodes = 1 << (int(sys.argv[3]) if len(sys.argv) > 3 else 21)
t0_scan = N + 2
n_scans = t0_scan + n_timed
sc = make_scenario(T=50, radius=1581.0, lambda_phi=6.4e-7, n_scans=n_scans, P_d=0.9, period=2.5, seed=5446, confine=True)
ais = make_ais(sc, seed=11, equipped=0.2, p_report=0.7)
ais = [a if k % 3 == 1 else [] for k, a in enumerate(ais)]
for mode in ("radar only (aisAided forest)", "with AIS messages"):
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=N, eta2=5.99, radarRange=float(sc["radius"]) * 1.5,
                  position=np.asarray(sc["centre"], dtype=float), aisAided=True, maxTargets=128, maxNodes=max_nodes, maxMeasurements=256)
    trk._add_targets([Target(sc["t0"], None, x.copy(), pv.P0, status="preinitialized") for x in sc["x0"]])
    t0, L, k = None, [], 0
    try:
        for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
            if k == t0_scan:
                trk.synchronize(); t0 = time.perf_counter()
            msgs = AisMessageList([AisMessage(*m) for m in ais[k]]) if mode == "with AIS messages" else AisMessageList()
            trk.addMeasurementList(MeasurementList(float(t), z), msgs, aisInitialization=False, pruneSimilar=(k % 3 != 0))
            if k >= t0_scan and k % 4 == 0:
                L.append(trk.lastScanStats["L"])
        trk.synchronize()
        dt = time.perf_counter() - t0
        print("N=%-2d %-30s %8.1f scans/s  %7.3f ms/scan  leaves (sampled) %s  ILPs %d" % (N, mode, n_timed / dt, 1e3 * dt / n_timed, L, trk.nOptimSolved), flush=True)
    except Exception as e:      # (a pool too small for the window: MHT_E_CAPACITY)
        print("N=%-2d %-30s FAILED at scan %d: %s" % (N, mode, k, str(e)[:160]), flush=True)
    finally:
        trk.close()
