"""Shared by tests/test_blp_sweep_cpu.py and tests/test_blp_sweep_gpu.py: the recorded sweep of synthetic 0-1 ILPs on the dispatch
thresholds of csrc/mht_blp.hip (tests/golden/g24_ilp_sweep.npz, written by oracle/gen_ilp_sweep.py) with its tags, and the
feasibility check of a selection.  NumPy only."""
import os

import numpy as np

SWEEP = "g24_ilp_sweep.npz"
GAP = 1e-6      # obj - lp above this: the LP relaxation is not tight, no dual certificate exists
FAMILIES = ("small", "wide", "middle", "tier", "rowedge", "depth")
TAGS = ("lp", "second", "family", "variant", "K", "nH", "nR", "PD", "bf", "bf_obj", "bf_ties")


def load_sweep(gold_dir):
    """The instances (the layout of test_cluster_blp_gpu.load_instances) with their tags; read once per process, nobody writes to it."""
    if load_sweep.cache is None:
        g = np.load(os.path.join(gold_dir, SWEEP))
        tags = {k: g[k] for k in TAGS}
        out = []
        for i in range(int(g["n_inst"])):
            p = "i%03d_" % i
            ptr, rows = g[p + "col_ptr"], g[p + "col_rows"]
            inst = dict(index=i, cols=[rows[ptr[c]:ptr[c + 1]] for c in range(len(ptr) - 1)], sizes=g[p + "sizes"], cost=g[p + "cost"],
                        sel=g[p + "sel"], obj=float(g[p + "obj"]), unique=bool(g[p + "unique"]))
            for k in TAGS:
                v = tags[k][i]
                inst[k] = str(v) if k in ("family", "variant") else (bool(v) if k == "bf" else (float(v) if k in ("lp", "second", "bf_obj") else int(v)))
            inst["gap"] = inst["obj"] - inst["lp"] > GAP
            out.append(inst)
        load_sweep.cache = out
    return load_sweep.cache


load_sweep.cache = None


def check_feasible(inst, sel):
    """`sel` (one column per target, ascending) picks inside every target's group and uses no row twice."""
    sizes = np.asarray(inst["sizes"])
    starts = np.concatenate([[0], np.cumsum(sizes)])
    sel = list(sel)
    assert len(sel) == len(sizes)
    used = set()
    for t, h in enumerate(sel):
        assert starts[t] <= h < starts[t + 1], (inst["index"], t, h)
        for r in inst["cols"][h]:
            assert int(r) not in used, (inst["index"], t, h, int(r))
            used.add(int(r))
