"""CPU: the helper of the every-scan overlap tests (tests/overlap_util.py) must be able to fail.  Two identical synthetic recordings, then ONE
thing changed at a time -- a selection in a middle scan, one bit of a state, a cluster label, a birth's id, one bit of the used-measurement
words, one leaf covariance -- must make the comparer raise and name the scan; differing node handles must not."""
import copy

import numpy as np
import pytest

import overlap_util as ou

# (the layout of mht_target_report / mht_birth_report for four states, as pymht_amd/tracker.py views them)
REPORT = np.dtype([("id", "<i4"), ("status", "<i4"), ("sel_node", "<i4"), ("sel_meas", "<i4"), ("new_index", "<i4"), ("root_scan", "<i4"), ("root_node", "<i4"),
                   ("n_leaves", "<i4"), ("sel_x", "<f8", (4,)), ("sel_cnllr", "<f8"), ("score", "<f8"), ("root_cnllr", "<f8"), ("root_x", "<f8", (4,)),
                   ("root_meas", "<i4"), ("cluster", "<i4")])
BIRTH = np.dtype([("id", "<i4"), ("meas", "<i4"), ("x0", "<f8", (4,)), ("P0", "<f4", (16,))])
N_SCANS, MID = 12, 7


def _rows(rng, ids, scan):
    n = len(ids)
    r = np.zeros(n, dtype=REPORT)
    r["id"], r["status"] = ids, 0
    r["sel_node"], r["root_node"] = rng.integers(0, 1 << 18, n), rng.integers(0, 1 << 18, n)
    r["sel_meas"] = rng.integers(0, 40, n)
    r["new_index"], r["root_scan"], r["n_leaves"] = np.arange(n), max(scan - 3, 0), rng.integers(1, 9, n)
    r["sel_x"], r["root_x"] = rng.normal(0, 500, (n, 4)), rng.normal(0, 500, (n, 4))
    r["sel_cnllr"], r["score"], r["root_cnllr"] = rng.normal(0, 3, n), rng.normal(0, 3, n), rng.normal(0, 3, n)
    r["root_meas"], r["cluster"] = rng.integers(0, 40, n), np.arange(n) // 3
    return r


def _recording(seed=1):
    rng = np.random.default_rng(seed)
    rec, ids, nxt = ou.Recording(), list(range(20)), 20
    for s in range(1, N_SCANS + 1):
        rec.rows[s] = _rows(rng, ids, s)
        if s % 4 == 3:      # two births behind this scan
            b = np.zeros(2, dtype=BIRTH)
            b["id"], b["meas"], b["x0"], b["P0"] = [nxt, nxt + 1], rng.integers(1, 40, 2), rng.normal(0, 500, (2, 4)), rng.normal(0, 1, (2, 16))
            rec.births[s] = b
            ids, nxt = ids + [nxt, nxt + 1], nxt + 2
    return rec


def _snapshot(seed=2, scan=MID):
    rng = np.random.default_rng(seed)
    rows = _rows(rng, list(range(20)), scan)
    n = int(rows["n_leaves"].sum())
    leaf = dict(ID=np.repeat(rows["id"], rows["n_leaves"]), x=rng.normal(0, 500, (n, 4)), P=rng.normal(0, 1, (n, 4, 4)).astype(np.float32), cnllr=rng.normal(0, 3, n),
                meas=rng.integers(0, 40, n).astype(np.int32), target=np.repeat(np.arange(20), rows["n_leaves"]).astype(np.int32), node=rng.integers(0, 1 << 18, n).astype(np.int32),
                flags=np.zeros(n, np.uint8))
    return ((scan, 20, 20, 70, 150, n, 7, 3), rows, rng.integers(0, 1 << 62, 4).astype(np.uint64), leaf)


@pytest.mark.parametrize("N", [3, 5])
def test_stop_set_is_sorted_unique_and_in_range(N):
    R = N + 4
    for n_scans in (1, R, 30, 64, 200, 240):
        s = ou.stop_set(N, n_scans)
        assert s == sorted(set(s)) and s[0] == 1 and all(1 <= k <= n_scans for k in s)
    full = ou.stop_set(N, 240)
    assert set(full) >= {1, 2, 3, N, N + 1, R - 1, R, R + 1, 2 * R + 1, 59, 60, 61, 63, 64, 65, 128, 200} and full[-1] == 200
    assert ou.stop_set(N, 240, top=ou.STOPS_TOP[:-1])[-1] == 128      # (shortened from the top)
    g = ou.group_stop_set(N, 30)
    assert g == sorted(set(g)) and set(g) == {1, 2, N + 1, R, R + 1, 30}


def test_identical_recordings_pass_and_handles_are_ignored():
    a, b = _recording(), _recording()
    ou.compare_recordings(a, b)
    for s in b.scans():
        b.rows[s]["sel_node"] += 5
        b.rows[s]["root_node"] -= 3
    ou.compare_recordings(a, b)
    sa, sb = _snapshot(), _snapshot()
    sb[3]["node"] = sb[3]["node"] + 11
    sb[1]["sel_node"] += 1
    ou.compare_snapshot(sa, sb, MID)


def _flip_sel_meas(rec):
    rec.rows[MID]["sel_meas"][4] += 1


def _flip_state_bit(rec):
    rec.rows[MID]["sel_x"].view(np.uint64)[9, 2] ^= np.uint64(1)


def _flip_cluster(rec):
    rec.rows[MID]["cluster"][5] = 2


def _flip_birth_id(rec):
    rec.births[MID]["id"][1] += 1


@pytest.mark.parametrize("change,word", [(_flip_sel_meas, "sel_meas"), (_flip_state_bit, "sel_x"), (_flip_cluster, "cluster"), (_flip_birth_id, "births")])
def test_one_change_in_a_middle_scan_is_found_and_named(change, word):
    assert MID % 4 == 3 and 1 < MID < N_SCANS
    a, b = _recording(), _recording()
    change(b)
    with pytest.raises(AssertionError) as ei:
        ou.compare_recordings(a, b)
    assert ("scan %d:" % MID) in str(ei.value) and word in str(ei.value), str(ei.value)
    with pytest.raises(AssertionError):      # (either way round)
        ou.compare_recordings(b, a)


def test_a_dropped_scan_or_birth_is_found():
    a, b = _recording(), _recording()
    del b.births[MID]
    with pytest.raises(AssertionError) as ei:
        ou.compare_recordings(a, b)
    assert ("scan %d:" % MID) in str(ei.value)
    b = _recording()
    del b.rows[N_SCANS]
    with pytest.raises(AssertionError):
        ou.compare_recordings(a, b)
    b = _recording()
    b.rows[MID] = b.rows[MID][:-1]
    with pytest.raises(AssertionError) as ei:
        ou.compare_recordings(a, b)
    assert ("scan %d:" % MID) in str(ei.value)


def test_snapshot_changes_are_found_and_named():
    ref = _snapshot()
    for what, word in (("used", "used"), ("P", "'P'"), ("header", "n_clusters"), ("row", "sel_meas"), ("leaf_count", "leaves")):
        got = copy.deepcopy(ref)
        if what == "used":
            got[2][2] ^= np.uint64(1 << 17)
        elif what == "P":
            got[3]["P"].view(np.uint32)[31, 2, 1] ^= np.uint32(1)
        elif what == "header":
            got = (ref[0][:6] + (ref[0][6] + 1,) + ref[0][7:],) + got[1:]
        elif what == "row":
            got[1]["sel_meas"][0] += 1
        else:
            got[3]["cnllr"] = got[3]["cnllr"][:-1]
        with pytest.raises(AssertionError) as ei:
            ou.compare_snapshot(ref, got, MID)
        assert ("scan %d:" % MID) in str(ei.value) and word in str(ei.value), (what, str(ei.value))


def test_scan_logs_are_compared_key_by_key():
    log = [dict(L=10 + s, G=4, M=30, ilp=2, unused=np.arange(30) % 3 == 0, nTargets=20) for s in range(6)]
    ou.compare_stats(log, copy.deepcopy(log))
    other = copy.deepcopy(log)
    other[3]["unused"][7] ^= True
    with pytest.raises(AssertionError) as ei:
        ou.compare_stats(log, other)
    assert "scan 4:" in str(ei.value) and "unused" in str(ei.value)
    other = copy.deepcopy(log)
    other[2]["ilp"] = 3
    with pytest.raises(AssertionError) as ei:
        ou.compare_stats(log, other)
    assert "scan 3:" in str(ei.value) and "ilp" in str(ei.value)


def test_recording_against_a_reference_trace(gold_dir):
    """`check_scan_against_trace` on a recording built FROM a fixture (config 2: births and deaths) passes on every scan, and fails -- naming
    the scan -- when a selection, a cluster label, a termination or a birth of a middle scan is changed."""
    import os
    g = np.load(os.path.join(gold_dir, "g3b_trace_cfg2.npz"))
    n = int(g["n_scans"])
    rec, stats = ou.Recording(), []
    before = np.arange(int(np.sum(g["accepted"])))
    for s in range(1, n + 1):
        p = "s%02d_" % (s - 1)
        new, dead, after = g[p + "new_ids"], g[p + "dead"], g[p + "ids"]
        assert np.array_equal(np.setdiff1d(before, dead), after[:len(after) - len(new)])
        r = np.zeros(len(before), dtype=REPORT)
        r["id"], r["status"] = before, np.isin(before, dead) * 2
        live = r["status"] == 0
        k = int(live.sum())
        r["sel_meas"][live], r["sel_x"][live], r["sel_cnllr"][live] = g[p + "sel_meas"][:k], g[p + "sel_x"][:k], g[p + "sel_cnllr"][:k]
        ptr, mem = g[p + "cl_ptr"], g[p + "cl_members"]
        for c in range(len(ptr) - 1):
            r["cluster"][mem[ptr[c]:ptr[c + 1]]] = c
        rec.rows[s] = r
        if len(new):
            b = np.zeros(len(new), dtype=BIRTH)
            b["id"], b["meas"], b["x0"], b["P0"] = new, g[p + "sel_meas"][k:], g[p + "born_x"], g[p + "born_P"].reshape(len(new), 16)
            rec.births[s] = b
        L, G, M = g[p + "LGM"].tolist()
        stats.append(dict(L=L, G=G, M=M, unused=g[p + "unused"].copy(), nTargets=len(after)))
        before = after
    assert sum(len(b) for b in rec.births.values()) >= 5 and sum(int((r["status"] != 0).sum()) for r in rec.rows.values()) >= 4

    def check(rc):
        for s in range(1, n + 1):
            ou.check_scan_against_trace(g, s, rc.rows[s], rc.births_of(s), stats[s - 1], 2e-5)

    check(rec)
    mid = 7      # (fixture index 6: three births, one termination)
    assert len(rec.births[mid]) == 3 and int((rec.rows[mid]["status"] != 0).sum()) == 1

    def sel(rc): rc.rows[mid]["sel_meas"][3] += 1
    def state(rc): rc.rows[mid]["sel_x"].view(np.uint64)[2, 0] ^= np.uint64(1)
    def label(rc):
        lab = rc.rows[mid]["cluster"]
        lab[0] = lab.max() + 1 if np.count_nonzero(lab == lab[0]) > 1 else lab[1]
    def death(rc): rc.rows[mid]["status"][np.flatnonzero(rc.rows[mid]["status"] == 0)[-1]] = 2
    def birth(rc): rc.births[mid]["id"][2] += 1
    def born_state(rc): rc.births[mid]["x0"][0, 1] += 0.5
    def score(rc): rc.rows[mid]["sel_cnllr"][0] += 1e-4

    for change in (sel, state, label, death, birth, born_state, score):
        bad = copy.deepcopy(rec)
        change(bad)
        with pytest.raises(AssertionError) as ei:
            check(bad)
        assert ("scan %d " % mid) in str(ei.value), (change.__name__, str(ei.value))
