"""GPU: mht_ospa2_windows (csrc/mht_ospa2.hip) through pymht_amd.evaluation.ospa2_windows, the raw ABI and Tracker.getOspa2, against the
SciPy reference under the criterion of tests/ospa2_ref.py:
    |loc - loc_true| <= (nAssigned + 2 W + 12) eps64 loc_true,  |total - total_true| <= (nAssigned + 2 W + 14) eps64 total_true,
the counts exact and, where the optimum is unique, the match the reference's.  Nothing exceeds 130 objects a side except the capacity
refusal, which launches nothing."""
import numpy as np
import pytest
import torch

import gospa_ref
import ospa2_ref as ref

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = -7, 16


def windows_of(out):
    """ospa2_windows' dict as one tuple per window, in the order ospa2_ref.hold takes them"""
    return [(out["total"][w], out["localisation"][w], out["nAssigned"][w], out["nTracks"][w], out["nTruths"][w], out["match"][w])
            for w in range(len(out["total"]))]


def same_bits(a, b):
    return (np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes()
            and tuple(int(v) for v in a[2:5]) == tuple(int(v) for v in b[2:5]) and np.array_equal(a[5], b[5]))


def run_and_hold(gpu_ctx, run, wins, c, p=2, label="", match=True, **kw):
    """One call for all windows, each held to the reference; the dict's derived figures checked against its own counts."""
    from pymht_amd.evaluation import ospa2_windows
    out = ospa2_windows(*run, c, p, windows=wins, ctx=gpu_ctx, **kw)
    assert np.array_equal(out["windows"], np.asarray(wins, dtype=np.int32).reshape(-1, 2)) and out["match"].dtype == np.int32
    for got, (lo, hi) in zip(windows_of(out), wins):
        ref.hold(got, ref.reference(*run, lo, hi, c, p), hi - lo + 1, label and "%s [%d, %d] p %d" % (label, lo, hi, p), match=match)
    N = np.maximum(out["nTracks"], out["nTruths"])
    cp = c * c if p == 2 else c
    assert np.array_equal(out["cardinality"], cp * (N - out["nAssigned"]))
    mean = np.where(N > 0, out["total"] / np.maximum(N, 1), 0.0)
    assert np.array_equal(out["ospa2"], mean if p == 1 else np.sqrt(mean))
    return out


@pytest.fixture(scope="module")
def scene30():
    return ref.tracker_scene(30, seed=30)


def test_the_split_track_known_answer(gpu_ctx):
    run = ref.split_track()
    out = run_and_hold(gpu_ctx, run, [(0, 19)], 10.0, 1, "split track", match=False)
    assert (out["total"][0], out["localisation"][0], out["nAssigned"][0], out["cardinality"][0], out["ospa2"][0]) == (15.0, 5.0, 1, 10.0, 7.5)
    out = run_and_hold(gpu_ctx, run, [(0, 19)], 10.0, 2, "split track", match=False)
    assert (out["total"][0], out["localisation"][0], out["nAssigned"][0], out["nTracks"][0], out["nTruths"][0]) == (125.0, 25.0, 1, 2, 1)
    assert sorted(out["match"][0].tolist()) == [-1, 0]
    # per-scan GOSPA of the same data, on the device: 0 at every scan
    from pymht_amd.evaluation import gospa_steps
    per_scan = gospa_steps([run[0][t][run[1][t] != 0] for t in range(20)], [run[2][t] for t in range(20)], 10.0, ctx=gpu_ctx)
    assert (per_scan["total"] == 0.0).all()
    whole = run_and_hold(gpu_ctx, (run[2], run[3], run[2], run[3]), [(0, 19), (3, 3)], 10.0)      # the unbroken track
    assert (whole["total"] == 0.0).all() and (whole["nAssigned"] == 1).all()


def test_a_window_of_one_step_with_equal_counts_is_gospa_on_the_device(gpu_ctx):
    from pymht_amd.evaluation import gospa_steps, ospa2_windows
    rng = np.random.default_rng(4)
    for n in (1, 7, 64, 65, 130):
        run = ref.random_run(rng, n, n, 3, field=12.0 * np.sqrt(n), p_on=1.0)
        for p in (1, 2):
            got = run_and_hold(gpu_ctx, run, [(0, 0), (1, 1), (2, 2)], 15.0, p, "W = 1, %d x %d" % (n, n))
            steps = gospa_steps(list(run[0]), list(run[2]), 15.0, p, ctx=gpu_ctx)
            assert np.array_equal(got["nAssigned"], steps["nAssigned"])
            for w in range(3):
                want = gospa_ref.reference(run[0][w], run[2][w], 15.0, p)
                for total in (got["total"][w], steps["total"][w]):
                    assert abs(np.longdouble(total) - want["total"]) <= (want["nAssigned"] + 2 + 14) * ref.EPS * want["total"]


@pytest.mark.parametrize("p", [1, 2])
def test_member_counts_around_the_lane_stride_and_the_tile_edges(gpu_ctx, p):
    """0, 1, 63, 64, 65 and 130 members on either side, both orientations: the lane stride of a sweep, more than two columns per lane,
    a partial last tile of the base-distance kernel in rows (8) and in columns (64); whole run, one step, and a step where flags are off."""
    runs = ref.shape_runs()
    assert {r[1][1].shape[1] for r in runs} | {r[1][3].shape[1] for r in runs} >= {0, 1, 63, 64, 65, 130}
    most = 0
    for label, run, c in runs:
        out = run_and_hold(gpu_ctx, run, [(0, 4), (2, 2), (0, 0), (3, 4)], c, p, label)
        assert out["nTracks"][1] == run[1].shape[1] and out["nTruths"][1] == run[3].shape[1]      # (everybody is present at step 2)
        most = max(most, int(out["nAssigned"].max()))
    assert most > 64


def test_ragged_windows_of_1_2_5_and_all_steps_in_one_call(gpu_ctx, scene30):
    from pymht_amd.evaluation import ospa2_windows
    K = ref.K_SCENE
    wins, parts = [], {}
    for W in (1, 2, 5, K):
        for every in (1, 3):
            parts[W, every] = (len(wins), ref.sliding(K, W, every))
            wins += parts[W, every][1]
    for p in (1, 2):
        whole = windows_of(run_and_hold(gpu_ctx, scene30, wins, ref.C_SCENE, p, "ragged"))
        for (W, every), (at, part) in parts.items():
            slid = ospa2_windows(*scene30, ref.C_SCENE, p, window=W, every=every, ctx=gpu_ctx)
            assert slid["windows"].tolist() == [list(w) for w in part]
            assert all(same_bits(a, b) for a, b in zip(windows_of(slid), whole[at:at + len(part)]))
    one = ospa2_windows(*scene30, ref.C_SCENE, ctx=gpu_ctx)      # window=None: the whole run
    assert one["windows"].tolist() == [[0, K - 1]] and same_bits(windows_of(one)[0], windows_of(run_and_hold(gpu_ctx, scene30, [(0, K - 1)], ref.C_SCENE))[0])


@pytest.mark.parametrize("T", [5, 30, 64])
def test_tracker_like_scenes(gpu_ctx, T):
    run = ref.tracker_scene(T, seed=T)
    wins = [w for W in (1, 5, 16) for w in ref.sliding(ref.K_SCENE, W, every=3) + [(ref.K_SCENE - W, ref.K_SCENE - 1)]]
    for p in (1, 2):
        out = run_and_hold(gpu_ctx, run, wins, ref.C_SCENE, p, "T %d" % T)
        assert out["nAssigned"][-1] < out["nTracks"][-1]      # (fragments and false tracks: more tracks than can be assigned)
    swapped = run_and_hold(gpu_ctx, (run[2], run[3], run[0], run[1]), wins, ref.C_SCENE)
    for w, (lo, hi) in enumerate(wins):      # the roles swapped: the same total within the criterion
        want = ref.reference(*run, lo, hi, ref.C_SCENE)
        assert abs(np.longdouble(swapped["total"][w]) - want["total"]) <= ref.bounds(want, hi - lo + 1)[1]
    perfect = run_and_hold(gpu_ctx, (run[2], run[3], run[2], run[3]), wins, ref.C_SCENE)
    assert (perfect["total"] == 0.0).all() and (perfect["ospa2"] == 0.0).all()


def test_batches_of_1_2_and_300_windows_their_permutation_and_chunks(gpu_ctx, scene30):
    """More windows than the chip has compute units; a window's bits do not depend on its place, its neighbours or the chunk it is in."""
    from pymht_amd.evaluation import ospa2_windows
    rng = np.random.default_rng(8)
    lo = rng.integers(0, ref.K_SCENE, size=300)
    wins = [(int(a), int(rng.integers(a, ref.K_SCENE))) for a in lo]
    whole = windows_of(run_and_hold(gpu_ctx, scene30, wins, ref.C_SCENE))
    for count in (1, 2):
        part = windows_of(ospa2_windows(*scene30, ref.C_SCENE, windows=wins[10:10 + count], ctx=gpu_ctx))
        assert all(same_bits(a, b) for a, b in zip(part, whole[10:10 + count]))
    perm = rng.permutation(300)
    shuffled = windows_of(ospa2_windows(*scene30, ref.C_SCENE, windows=[wins[i] for i in perm], ctx=gpu_ctx))
    assert all(same_bits(shuffled[k], whole[i]) for k, i in enumerate(perm))
    n, m = scene30[1].shape[1], scene30[3].shape[1]
    budget = int(gpu_ctx.lib.mht_ospa2_work_bytes(n, m, ref.K_SCENE, 120))      # 300 windows in chunks of at most 120: three or more
    assert int(gpu_ctx.lib.mht_ospa2_work_bytes(n, m, ref.K_SCENE, 150)) > budget
    chunked = windows_of(ospa2_windows(*scene30, ref.C_SCENE, windows=wins, maxWorkBytes=budget, ctx=gpu_ctx))
    assert all(same_bits(a, b) for a, b in zip(chunked, whole))
    tight = windows_of(ospa2_windows(*scene30, ref.C_SCENE, windows=wins[:7], maxWorkBytes=int(gpu_ctx.lib.mht_ospa2_work_bytes(n, m, ref.K_SCENE, 1)),
                                     ctx=gpu_ctx))      # one window per chunk
    assert all(same_bits(a, b) for a, b in zip(tight, whole[:7]))


def test_poison_where_the_flags_are_off_changes_no_bit(gpu_ctx, scene30):
    from pymht_amd.evaluation import ospa2_windows
    rng = np.random.default_rng(1)
    filled = (np.where(np.isnan(scene30[0]), rng.uniform(-1e3, 1e3, size=scene30[0].shape), scene30[0]), scene30[1],
              np.where(np.isnan(scene30[2]), rng.uniform(-1e3, 1e3, size=scene30[2].shape), scene30[2]), scene30[3])
    assert np.isnan(scene30[0]).any() and np.isnan(scene30[2]).any() and not np.isnan(filled[0]).any() and not np.isnan(filled[2]).any()
    wins = [(0, 15), (4, 8), (15, 15), (0, 0), (7, 8)]
    for p in (1, 2):
        a = windows_of(ospa2_windows(*scene30, ref.C_SCENE, p, windows=wins, ctx=gpu_ctx))
        b = windows_of(ospa2_windows(*filled, ref.C_SCENE, p, windows=wins, ctx=gpu_ctx))
        assert all(same_bits(x, y) for x, y in zip(a, b))
        assert all(np.isfinite(x[0]) for x in a)


class Raw:
    """The raw ABI on buffers pre-filled with a sentinel and GUARD cells behind each array."""

    def __init__(self, ctx, run, wins):
        self.ctx, dev = ctx, ctx.device
        self.K, self.n, self.m = len(run[1]), run[1].shape[1], run[3].shape[1]
        self.lo = np.ascontiguousarray([w[0] for w in wins], dtype=np.int32)
        self.hi = np.ascontiguousarray([w[1] for w in wins], dtype=np.int32)
        self.n_win = len(wins)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        self.trk, self.trk_on, self.tru, self.tru_on = up(run[0], np.float64), up(run[1], np.uint8), up(run[2], np.float64), up(run[3], np.uint8)
        self.win = torch.full((2 * self.n_win + GUARD,), float(SENTINEL), dtype=torch.float64, device=dev)
        self.count = torch.full((3 * self.n_win + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.match = torch.full((self.n_win * self.n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.need = int(ctx.lib.mht_ospa2_work_bytes(self.n, self.m, self.K, self.n_win))
        self.work = torch.empty(self.need + 256, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

    def call(self, c=10.0, p=2, **over):
        a = dict(n_steps=self.K, n_trk=self.n, trk=self.trk.data_ptr(), trk_on=self.trk_on.data_ptr(), n_tru=self.m, tru=self.tru.data_ptr(),
                 tru_on=self.tru_on.data_ptr(), n_win=self.n_win, lo=self.lo.ctypes.data, hi=self.hi.ctypes.data, win=self.win.data_ptr(),
                 count=self.count.data_ptr(), match=self.match.data_ptr(), work=self.work.data_ptr(), work_bytes=self.need, ctx=self.ctx.handle)
        a.update(over)
        return self.ctx.lib.mht_ospa2_windows(a["ctx"], a["n_steps"], a["n_trk"], a["trk"], a["trk_on"], a["n_tru"], a["tru"], a["tru_on"], a["n_win"],
                                              a["lo"], a["hi"], c, p, a["win"], a["count"], a["match"], a["work"], a["work_bytes"])

    def outputs(self):
        torch.cuda.synchronize(self.ctx.device)
        return self.win.cpu().numpy(), self.count.cpu().numpy(), self.match.cpu().numpy()

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.outputs())

    def window(self, w):
        win, count, match = self.outputs()
        return (win[2 * w], win[2 * w + 1]) + tuple(count[3 * w:3 * w + 3]) + (match[w * self.n:(w + 1) * self.n],)


def test_every_output_cell_is_written_and_nothing_behind_them(gpu_ctx):
    runs = {r[0]: r for r in ref.shape_runs()}
    for label in ("0x3", "3x0", "0x0", "65x64", "63x130", "1x1"):
        _, run, c = runs[label]
        wins = [(0, 4), (2, 2), (0, 0), (1, 3)]
        raw = Raw(gpu_ctx, run, wins)
        assert raw.call(c=c) == 0
        win, count, match = raw.outputs()
        k, n = raw.n_win, raw.n
        assert not (win[:2 * k] == SENTINEL).any() and not (count[:3 * k] == SENTINEL).any() and not (match[:k * n] == SENTINEL).any()
        assert (win[2 * k:] == SENTINEL).all() and (count[3 * k:] == SENTINEL).all() and (match[k * n:] == SENTINEL).all()
        for w, (lo, hi) in enumerate(wins):
            ref.hold(raw.window(w), ref.reference(*run, lo, hi, c), hi - lo + 1, "%s [%d, %d]" % (label, lo, hi))


def test_refusals_through_the_raw_abi_leave_the_outputs_alone(gpu_ctx):
    from pymht_amd import _lib
    run = ref.random_run(np.random.default_rng(2), 3, 4, 5)
    wins = [(0, 4), (1, 2)]
    raw = Raw(gpu_ctx, run, wins)
    neg, late, crossed = np.array([-1, 1], dtype=np.int32), np.array([4, 5], dtype=np.int32), np.array([0, 3], dtype=np.int32)
    bad = [dict(n_steps=-1), dict(n_trk=-1), dict(n_tru=-1), dict(n_win=-1), dict(trk=None), dict(trk_on=None), dict(tru=None), dict(tru_on=None),
           dict(lo=None), dict(hi=None), dict(win=None), dict(count=None), dict(match=None), dict(work=None), dict(ctx=None),
           dict(lo=neg.ctypes.data), dict(hi=late.ctypes.data), dict(lo=crossed.ctypes.data), dict(n_steps=4),
           dict(work_bytes=raw.need - 1), dict(work_bytes=0)]
    for over in bad:
        assert raw.call(**over) == _lib.MHT_E_INVALID, over
        assert raw.untouched(), over
    for c in (0.0, -3.0, float("inf"), float("nan"), 1e200, 1e-200):
        assert raw.call(c=c) == _lib.MHT_E_INVALID and raw.untouched(), c
    for p in (0, 3, -1):
        assert raw.call(p=p) == _lib.MHT_E_INVALID and raw.untouched(), p
    assert raw.call(n_win=0) == _lib.MHT_OK and raw.untouched()      # (an empty batch: done, nothing written)
    assert raw.call(n_steps=0) == _lib.MHT_OK and raw.untouched()
    # 2 049 a side: refused before anything is launched (the arrays are never read at that size)
    for side in ("n_trk", "n_tru"):
        assert raw.call(**{side: 2049, "work_bytes": 1 << 40}) == _lib.MHT_E_CAPACITY and raw.untouched(), side
    assert "2048" in gpu_ctx.lib.mht_last_error().decode()
    assert raw.call() == 0 and not raw.untouched()      # (and the same buffers are good for a proper call)
    for w, (lo, hi) in enumerate(wins):
        ref.hold(raw.window(w), ref.reference(*run, lo, hi, 10.0), hi - lo + 1, match=False)


def test_tracker_histories_against_the_scenario_truth(gpu_ctx):
    """Eight targets initiated from the scenario's x0, fifteen scans (the scenario of tests/test_gospa_gpu.py); getOspa2 on the filtered
    and on the smoothed positions equals ospa2_windows on the arrays collected here from the track nodes, bit for bit, and is held to the
    reference on them."""
    from pymht_amd.evaluation import ospa2_windows
    from pymht_amd.models import pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    from pymht_amd.utils.scenario import make_scenario
    sc = make_scenario(T=8, radius=600, lambda_phi=2e-6, n_scans=15)
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=3, eta2=5.99, useInitiator=False)
    try:
        for x0 in sc["x0"]:
            trk.initiateTarget(Target(sc["t0"], None, x0.copy(), pv.P0))
        for zk, tk in zip(sc["scans"], sc["times"]):
            trk.addMeasurementList(MeasurementList(float(tk), zk))
        truth = (sc["times"], sc["truth"])
        nodes = list(trk.getTrackNodes()) + list(trk.__terminatedTargets__)
        chains = [n.backtrackNodes() for n in nodes]
        n_initial = sum(1 for ch in chains for nd in ch if float(nd.time) == sc["t0"])
        assert n_initial > 0
        smoothed = trk.getSmoothTracks(terminated=True)
        truXY = np.stack([np.asarray(y, dtype=np.float64)[:, 0:2] for y in sc["truth"]])
        truOn = np.ones(truXY.shape[:2], dtype=np.uint8)
        for smooth in (False, True):
            trkXY = np.full((15, len(chains), 2), np.nan)
            trkOn = np.zeros((15, len(chains)), dtype=np.uint8)
            for i, ch in enumerate(chains):
                for k, nd in enumerate(ch):
                    hit = np.flatnonzero(sc["times"] == float(nd.time))
                    if len(hit):
                        trkXY[hit[0], i] = smoothed[i][0][k] if smooth and len(ch) >= 2 else nd.x_0[0:2]
                        trkOn[hit[0], i] = 1
            for window, every in ((None, 1), (5, 2)):
                got = trk.getOspa2(truth, c=20, window=window, every=every, smooth=smooth)
                direct = ospa2_windows(trkXY, trkOn, truXY, truOn, 20, window=window, every=every, ctx=gpu_ctx)
                assert got["nIgnored"] == n_initial and len(got["trackIds"]) == len(chains)
                assert np.array_equal(got["windows"], direct["windows"]) and np.array_equal(got["times"], sc["times"][direct["windows"][:, 1]])
                for w, (a, b) in enumerate(zip(windows_of(got), windows_of(direct))):
                    assert same_bits(a, b), w
                    lo, hi = direct["windows"][w]
                    ref.hold(a, ref.reference(trkXY, trkOn, truXY, truOn, lo, hi, 20.0), hi - lo + 1,
                             "window [%d, %d]%s" % (lo, hi, ", smoothed" if smooth else ""))
                assert (got["nTruths"] == 8).all() and got["meanOspa2"] == float(np.mean(got["ospa2"]))
                print("smooth=%s window=%s: mean OSPA(2) %.4f, assigned %s of %s tracks" % (smooth, window, got["meanOspa2"], got["nAssigned"].tolist(),
                                                                                        got["nTracks"].tolist()))
        ids = [[("t", r) for r in range(8)] for _ in sc["times"]]
        named = trk.getOspa2(truth, c=20, truthIds=ids)
        assert same_bits(windows_of(named)[0], windows_of(trk.getOspa2(truth, c=20))[0])
        with pytest.raises(ValueError, match="smooth"):
            trk.getOspa2(truth, c=20, constantTurn=True)
        with pytest.raises(ValueError, match="constant-turn"):
            trk.getOspa2(truth, c=20, smooth=True, constantTurn=True)
    finally:
        trk.close()
