"""CPU: the streams of the initiator shape tests (tests/initiator_util.py) reach the sizes at which the device initiator changes path, and
the two shortcuts the large streams take through the oracle change nothing.

(a) Boundary table: per case, the figures of the oracle run that test_initiator_shapes_gpu.py relies on (its docstring lists them).
(b) gnn_assign_by_component returns the pairs of the whole-matrix oracle.gnn_assign on every problem of the `dense` and `seeds` streams and
    of the first three scans of `wide` (the whole matrix of a later `wide` scan takes the Hungarian solve 8-10 s).
(c) The oracle with both shortcuts (assignment by component, similarity skipped between tracks that are far_apart) returns bit for bit
    what the plain oracle returns, scan by scan, on `dense`, `seeds`, `edges`, `ais` and the first three scans of `wide`."""
import numpy as np
import pytest

import initiator_util as iu


def _figures(name):
    run = iu.oracle_run(name)
    print(iu.describe(run))
    return run, run["figures"]


def test_wide_stream_passes_one_workgroup_and_the_node_limit():
    run, f = _figures("wide")
    assert f["max_unused"] > 2 * iu.NT                      # three passes of the unused compaction
    assert f["max_M"] % 64 != 0 and f["max_M"] > 2 * iu.NT   # ... of a bit mask with a ragged last word
    assert f["max_prelim"] > iu.NT and f["max_prelim_in"] > iu.NT      # two passes of the predict / verdict loops
    assert f["max_V"] > 2 * iu.NT                           # gnn_core's third find loop
    assert f["max_born"] > 256                              # more than the Python wrapper's MAX_BORN
    assert f["max_seeds"] > 128                             # more than two blocks of 64 initiators
    assert f["n_global"] >= 8 and f["n_lds"] == 0           # every table in global memory
    assert f["max_born"] <= run["cfg"]["max_born"] and f["max_prelim"] <= run["cfg"]["max_prelim"] and f["max_M"] <= run["cfg"]["max_meas"]


def test_dense_stream_straddles_the_lds_limit():
    run, f = _figures("dense")
    sizes = sorted(p["lds_bytes"] for p in run["problems"] if p["E"] > 0)
    print("dense: table bytes", sizes)
    assert f["n_lds"] >= 2 and f["n_global"] >= 2
    assert f["max_prelim"] > 64 and f["max_born"] > 4      # what the capacity case overflows with max_prelim = 64, max_born = 4


def test_seeds_stream_has_more_initiators_than_threads():
    run, f = _figures("seeds")
    assert f["max_seeds"] > iu.NT
    assert f["n_E0"] >= 1                                   # tracks but no allowed pair: gnn_core's early return
    assert f["max_V"] > 2 * iu.NT


def test_edges_stream_holds_every_edge():
    run, f = _figures("edges")
    unused = [w["n_unused"] for w in run["want"]]
    assert len(run["scans"][0][0]) == 0
    assert {0, 1, 64, 65, iu.NT, iu.NT + 1} <= set(unused)
    assert f["frozen_with_tracks"] >= 2 and f["all_used"] >= 1      # an empty scan and an all-used scan while preliminary tracks exist
    assert any(len(z) == 1 for z, _, _ in run["scans"])
    t = np.array([iu.T0] + [s[2] for s in run["scans"]])
    assert {1.0, 2.5, 4.0} <= set(np.diff(t).tolist())
    assert f["n_merged"] >= 1
    assert f["max_seeds"] > 64 and f["n_lds"] >= 2 and f["n_global"] >= 2 and f["n_E0"] >= 1


def test_ais_stream_covers_the_seeding_phase():
    run, f = _figures("ais")
    n = [len(m) for m in run["ais"]]
    assert min(n) == 0 and 30 <= max(n) <= 40
    assert f["ais_started"] >= 20
    assert f["ais_known"] >= 1              # a message whose identity already has a preliminary track
    assert f["ais_similar_old"] >= 1        # ... similar to a track there was before the scan
    assert f["ais_similar_new"] >= 1        # ... similar to a track an earlier message of the same scan started
    assert f["ais_used"] >= 1               # messages flagged used
    assert f["ais_only_scans"] >= 1         # messages and no unused radar measurement: processed, not frozen
    for k in iu.AIS_NULL_USED_SCANS:        # flags passed as NULL
        assert run["ais"][k] and not any(m.used for m in run["ais"][k])
    assert f["n_lds"] >= 2 and f["n_global"] >= 2


@pytest.mark.parametrize("name,n_scans", [("dense", None), ("seeds", None), ("wide", 3)])
def test_assignment_by_component_equals_the_whole_matrix(name, n_scans):
    import m_of_n_oracle as orc
    run = iu.oracle_run(name, keep_matrices=True, large=False, n_scans=n_scans)
    n_pairs = 0
    for p in run["problems"]:
        whole = [(int(r), int(c)) for r, c in orc.gnn_assign(p["delta"], p["gate"])]
        parts = [(int(r), int(c)) for r, c in iu.gnn_assign_by_component(p["delta"], p["gate"])]
        assert parts == whole, p["where"]
        n_pairs += len(whole)
    print("%s: %d problems, %d pairs" % (name, len(run["problems"]), n_pairs))
    assert n_pairs >= 2 and len(run["problems"]) >= 3


@pytest.mark.parametrize("name,n_scans", [("dense", None), ("seeds", None), ("edges", None), ("ais", None), ("wide", 3)])
def test_shortcuts_of_the_large_streams_change_nothing(name, n_scans):
    plain = iu.oracle_run(name, keep_matrices=True, large=False, n_scans=n_scans)      # (the run of the test above)
    quick = iu.oracle_run(name, large=True, n_scans=n_scans)
    assert len(plain["want"]) == len(quick["want"])
    for k, (a, b) in enumerate(zip(plain["want"], quick["want"])):
        assert np.array_equal(a["meas"], b["meas"]) and np.array_equal(a["x"], b["x"]) and np.array_equal(a["P"], b["P"]), (name, k)
        assert (a["n_prelim"], a["n_seeds"]) == (b["n_prelim"], b["n_seeds"]), (name, k)
    assert [(p["n1"], p["n2"], p["E"]) for p in plain["problems"]] == [(p["n1"], p["n2"], p["E"]) for p in quick["problems"]]
