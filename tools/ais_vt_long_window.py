"""Development: the value-table test's scene (tests/test_ais_long_window_gpu.py::test_long_window_trace_across_value_table_generations:
N = 12, 40 scans, seed 4600) under MHT_VTAB_CAP = CAP, oracle-checked scan by scan: ids handed out and generation switches per scan.
usage: ais_vt_long_window.py CAP"""
import sys, os, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT]
import numpy as np
os.environ["MHT_VTAB_CAP"] = sys.argv[1]
from ais_long_util import long_window_scenario, make_pair, msgs_of, oracle_msgs_of, prune_on, compare_scan
from pymht_amd.utils.classDefinitions import MeasurementList
N = 12
sc, ais = long_window_scenario(4600, N, n_scans=40)
trk, o = make_pair(sc, N, False)
del os.environ["MHT_VTAB_CAP"]
try:
    for k, (z, t) in enumerate(zip(sc["scans"], sc["times"])):
        info = o.add_scan(float(t), z, prune_similar=prune_on(k), ais=oracle_msgs_of(ais[k]), ais_initialization=False)
        trk.addMeasurementList(MeasurementList(float(t), z), msgs_of(ais[k]), aisInitialization=False, pruneSimilar=prune_on(k))
        v, r = np.zeros(1, np.uint32), np.zeros(1, np.int32)
        trk._lib.mht_forest_debug_read(trk._ctx.handle, b"vcount", v.ctypes.data_as(C.c_void_p), 4)
        trk._lib.mht_forest_debug_read(trk._ctx.handle, b"vt_rebuilds", r.ctypes.data_as(C.c_void_p), 4)
        compare_scan(trk, o, info, "scan %d" % k)
        print("cap %s scan %2d L %6d msgs %d vcount %8d rebuilds %d" % (sys.argv[1], k, info["L"], len(ais[k]), int(v[0]), int(r[0])), flush=True)
    print("cap %s OK rebuilds %d" % (sys.argv[1], int(r[0])))
finally:
    trk.close()
