"""GPU: mht_gospa_steps (csrc/mht_gospa.hip) through pymht_amd.evaluation.gospa_steps, the raw ABI and Tracker.getGospa, against the
SciPy reference under the criterion of tests/gospa_ref.py:
    |loc - loc_true| <= (nAssigned + 8) eps64 loc_true,  |total - total_true| <= (nAssigned + 10) eps64 total_true,
the counts exact and, where the optimum is unique, the match the reference's.  Nothing exceeds 130 objects a side except the capacity
refusal, which launches nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import gospa_ref as ref

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = -7, 16


def steps_of(out):
    """gospa_steps' dict as one tuple per step, in the order gospa_ref.hold takes them"""
    return [(out["total"][s], out["localisation"][s], out["nAssigned"][s], out["nMissed"][s], out["nFalse"][s], out["match"][s])
            for s in range(len(out["total"]))]


def run_and_hold(gpu_ctx, cases, p=2, match=True):
    """cases: (label, X, Y, c) with ONE c; one launch for all of them, each held to the reference.  Returns the dict."""
    from pymht_amd.evaluation import gospa_steps
    c = cases[0][3]
    assert all(k[3] == c for k in cases)
    out = gospa_steps([k[1] for k in cases], [k[2] for k in cases], c, p, ctx=gpu_ctx)
    for got, (label, X, Y, _) in zip(steps_of(out), cases):
        ref.hold(got, ref.reference(X, Y, c, p), "%s p %d" % (label, p), match=match)
    cp = c * c if p == 2 else c
    assert np.array_equal(out["missed"], cp / 2 * out["nMissed"]) and np.array_equal(out["false"], cp / 2 * out["nFalse"])
    assert np.array_equal(out["gospa"], out["total"] if p == 1 else np.sqrt(out["total"]))
    assert all(m.dtype == np.int32 and len(m) == len(k[1]) for m, k in zip(out["match"], cases))
    return out


def same_bits(a, b):
    """two step tuples, bit for bit"""
    return (np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes()
            and tuple(int(v) for v in a[2:5]) == tuple(int(v) for v in b[2:5]) and np.array_equal(a[5], b[5]))


def test_greedy_traps_the_boundary_and_an_empty_step(gpu_ctx):
    cases = [("nearest pair first fails", [(0, 0), (2, 0)], [(1.1, 0), (3.3, 0)], 10.0),
             ("row-order greedy fails", [(0, 0), (2, 0)], [(1.2, 0), (-1.5, 0)], 10.0),
             ("both sides empty", np.zeros((0, 2)), np.zeros((0, 2)), 10.0)]
    out = run_and_hold(gpu_ctx, cases)
    assert abs(out["total"][0] - 2.90) < 1e-12 and out["match"][0].tolist() == [0, 1]      # (greedy: 11.70)
    assert abs(out["total"][1] - 2.89) < 1e-12 and out["match"][1].tolist() == [1, 0]      # (greedy: 13.69)
    assert out["total"][2] == 0.0 and out["gospa"][2] == 0.0 and len(out["match"][2]) == 0
    for p in (1, 2):
        at = run_and_hold(gpu_ctx, [("d == c", [(0, 0)], [(3, 4)], 5.0)], p)
        assert (at["nAssigned"][0], at["nMissed"][0], at["nFalse"][0]) == (0, 1, 1) and at["match"][0].tolist() == [-1]
        assert at["localisation"][0] == 0.0 and at["total"][0] == 5.0 ** p
        inside = run_and_hold(gpu_ctx, [("d < c", [(0, 0)], [(3, 4)], 5.000001)], p)
        assert (inside["nAssigned"][0], inside["nMissed"][0], inside["nFalse"][0]) == (1, 0, 0) and inside["match"][0].tolist() == [0]
        assert inside["localisation"][0] == 5.0 ** p == inside["total"][0]


@pytest.mark.parametrize("p", [1, 2])
def test_set_sizes_around_the_lane_stride_in_one_ragged_batch(gpu_ctx, p):
    """A side of 0, 1, 63, 64, 65 or 130 objects, n > m and m > n (gospa_ref.shape_cases), all in one launch: empty steps next to
    the largest."""
    cases = ref.shape_cases()
    assert {len(k[1]) for k in cases} | {len(k[2]) for k in cases} >= {0, 1, 63, 64, 65, 130}
    out = run_and_hold(gpu_ctx, cases, p)
    assert out["nAssigned"].max() > 64


def test_sparse_and_dense_scenes(gpu_ctx):
    """Nobody within c (no edges, every row leaves at once); tracker-like scenes of 64 and 130 targets; 137 x 130 inside one cut-off
    (long chains, exits that displace rows)."""
    rng = np.random.default_rng(3)
    grid = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0)), axis=-1).reshape(-1, 2) * 100.0
    cases = [("nobody within c", grid + rng.uniform(20.0, 30.0, size=grid.shape), grid, ref.C_SCENE)]
    cases += [("sparse scene of %d" % T,) + ref.sparse_scene(T, seed=T) + (ref.C_SCENE,) for T in (64, 130)]
    cases.append(("dense 137 x 130",) + ref.dense_scene() + (ref.C_SCENE,))
    for p in (1, 2):
        out = run_and_hold(gpu_ctx, cases, p)
        assert out["nAssigned"][0] == 0 and out["localisation"][0] == 0.0 and (out["match"][0] == -1).all()
        assert out["nAssigned"][3] == 130 and out["nFalse"][3] == 7 and out["nMissed"][3] == 0


def test_ties_give_the_reference_figures(gpu_ctx):
    """Two estimates on one point and one truth, and a truth midway between two estimates: the match is not unique, totals and
    counts are."""
    cases = [("two estimates on one point", [(1, 1), (1, 1)], [(2, 1)], 10.0), ("a truth midway", [(0, 0), (2, 0)], [(1, 0)], 10.0),
             ("two truths on one point", [(0, 3)], [(0, 0), (0, 0)], 10.0)]
    for p in (1, 2):
        out = run_and_hold(gpu_ctx, cases, p, match=False)
        assert sorted(out["match"][0].tolist()) == [-1, 0] and sorted(out["match"][1].tolist()) == [-1, 0] and out["match"][2][0] in (0, 1)


def _small_steps(n_steps, seed):
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n_steps):
        n, m = rng.integers(0, 13, size=2)
        out.append(("step %d (%dx%d)" % (s, n, m),) + ref.random_sets(rng, n, m, field=40.0) + (12.0,))
    return out


def test_batches_of_1_2_and_300_steps_and_their_permutation(gpu_ctx):
    """More steps than the chip has compute units, ragged; a step's bits do not depend on its place or on its neighbours."""
    from pymht_amd.evaluation import gospa_steps
    big = [k for k in ref.shape_cases() if k[0] in ("130x130", "0x0", "65x64")]
    cases = _small_steps(297, seed=8)
    cases[10:10] = [(k[0], k[1], k[2], 12.0) for k in big]      # (empty and largest next to each other, in the middle)
    assert len(cases) == 300
    whole = steps_of(run_and_hold(gpu_ctx, cases))
    for count in (1, 2):
        part = steps_of(run_and_hold(gpu_ctx, cases[10:10 + count]))
        assert all(same_bits(a, b) for a, b in zip(part, whole[10:10 + count]))
    alone = steps_of(gospa_steps([cases[11][1]], [cases[11][2]], 12.0, ctx=gpu_ctx))      # (65x64, between the empty step and the largest)
    assert same_bits(alone[0], whole[11])
    perm = np.random.default_rng(5).permutation(300)
    shuffled = steps_of(gospa_steps([cases[i][1] for i in perm], [cases[i][2] for i in perm], 12.0, ctx=gpu_ctx))
    assert all(same_bits(shuffled[k], whole[i]) for k, i in enumerate(perm))


class Raw:
    """The raw ABI on buffers pre-filled with a sentinel and GUARD cells behind each array."""

    def __init__(self, ctx, X, Y):
        self.ctx, dev = ctx, ctx.device
        self.est_off = np.concatenate([[0], np.cumsum([len(x) for x in X])]).astype(np.int32)
        self.tru_off = np.concatenate([[0], np.cumsum([len(y) for y in Y])]).astype(np.int32)
        self.n_steps, self.n_est, self.n_tru = len(X), int(self.est_off[-1]), int(self.tru_off[-1])
        up = lambda sets: torch.from_numpy(np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in sets] + [np.zeros((1, 2))])).to(dev)
        self.est, self.tru = up(X), up(Y)
        self.step = torch.full((2 * self.n_steps + GUARD,), float(SENTINEL), dtype=torch.float64, device=dev)
        self.count = torch.full((3 * self.n_steps + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.match = torch.full((self.n_est + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.need = int(ctx.lib.mht_gospa_work_bytes(self.n_steps, self.n_est, self.n_tru))
        self.work = torch.empty(self.need + 256, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

    def call(self, c=10.0, p=2, **over):
        a = dict(n_steps=self.n_steps, est_off=self.est_off.ctypes.data, est=self.est.data_ptr(), tru_off=self.tru_off.ctypes.data,
                 tru=self.tru.data_ptr(), step=self.step.data_ptr(), count=self.count.data_ptr(), match=self.match.data_ptr(),
                 work=self.work.data_ptr(), work_bytes=self.need, ctx=self.ctx.handle)
        a.update(over)
        return self.ctx.lib.mht_gospa_steps(a["ctx"], a["n_steps"], a["est_off"], a["est"], a["tru_off"], a["tru"], c, p, a["step"], a["count"],
                                            a["match"], a["work"], a["work_bytes"])

    def outputs(self):
        torch.cuda.synchronize(self.ctx.device)
        return self.step.cpu().numpy(), self.count.cpu().numpy(), self.match.cpu().numpy()

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.outputs())


def test_every_output_cell_is_written_and_nothing_behind_them(gpu_ctx):
    cases = [k for k in ref.shape_cases() if k[0] in ("0x3", "3x0", "0x0", "65x64", "63x130", "1x1")]
    raw = Raw(gpu_ctx, [k[1] for k in cases], [k[2] for k in cases])
    assert raw.call(c=15.0) == 0
    step, count, match = raw.outputs()
    n = raw.n_steps
    assert not (step[:2 * n] == SENTINEL).any() and not (count[:3 * n] == SENTINEL).any() and not (match[:raw.n_est] == SENTINEL).any()
    assert (step[2 * n:] == SENTINEL).all() and (count[3 * n:] == SENTINEL).all() and (match[raw.n_est:] == SENTINEL).all()
    for s, (label, X, Y, c) in enumerate(cases):
        got = (step[2 * s], step[2 * s + 1]) + tuple(count[3 * s:3 * s + 3]) + (match[raw.est_off[s]:raw.est_off[s + 1]],)
        ref.hold(got, ref.reference(X, Y, 15.0), label)


def test_refusals_through_the_raw_abi_leave_the_outputs_alone(gpu_ctx):
    from pymht_amd import _lib
    rng = np.random.default_rng(2)
    X, Y = [rng.uniform(0, 20, (3, 2)), rng.uniform(0, 20, (2, 2))], [rng.uniform(0, 20, (2, 2)), rng.uniform(0, 20, (4, 2))]
    raw = Raw(gpu_ctx, X, Y)
    dec, late = np.array([0, 4, 3], dtype=np.int32), np.array([1, 3, 5], dtype=np.int32)
    bad = [dict(n_steps=-1), dict(est_off=None), dict(tru_off=None), dict(est=None), dict(tru=None), dict(step=None), dict(count=None),
           dict(match=None), dict(work=None), dict(ctx=None), dict(est_off=dec.ctypes.data), dict(tru_off=dec.ctypes.data),
           dict(est_off=late.ctypes.data), dict(tru_off=late.ctypes.data), dict(work_bytes=raw.need - 1), dict(work_bytes=0)]
    for over in bad:
        assert raw.call(**over) == _lib.MHT_E_INVALID, over
        assert raw.untouched(), over
    for c in (0.0, -3.0, float("inf"), float("nan"), 1e200, 1e-200):
        assert raw.call(c=c) == _lib.MHT_E_INVALID and raw.untouched(), c
    for p in (0, 3, -1):
        assert raw.call(p=p) == _lib.MHT_E_INVALID and raw.untouched(), p
    assert raw.call(n_steps=0) == _lib.MHT_OK and raw.untouched()      # (an empty batch: done, nothing written)
    # a 2 049-object step: refused before anything is launched (the arrays behind the offsets are never read)
    for side in ("est_off", "tru_off"):
        over = {side: np.array([0, 1, 2050], dtype=np.int32).ctypes.data}
        assert raw.call(**over) == _lib.MHT_E_CAPACITY and raw.untouched(), side
    assert "2048" in gpu_ctx.lib.mht_last_error().decode()
    assert raw.call() == 0 and not raw.untouched()      # (and the same buffers are good for a proper call)
    step, count, match = raw.outputs()
    for s in range(2):
        got = (step[2 * s], step[2 * s + 1]) + tuple(count[3 * s:3 * s + 3]) + (match[raw.est_off[s]:raw.est_off[s + 1]],)
        ref.hold(got, ref.reference(X[s], Y[s], 10.0))


def test_tracker_histories_against_the_scenario_truth(gpu_ctx):
    """Eight targets initiated from the scenario's x0, fifteen scans; getGospa on the filtered and on the smoothed positions equals
    gospa_steps on the same estimates, collected here from the track nodes, and the reference on them."""
    from pymht_amd.evaluation import gospa_steps
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
        means = {}
        for smooth in (False, True):
            got = trk.getGospa(truth, c=20, smooth=smooth)
            X = [[] for _ in sc["times"]]
            for i, ch in enumerate(chains):
                for k, nd in enumerate(ch):
                    hit = np.flatnonzero(sc["times"] == float(nd.time))
                    if len(hit):
                        X[hit[0]].append(smoothed[i][0][k] if smooth and len(ch) >= 2 else nd.x_0[0:2])
            X = [np.array(x, dtype=np.float64).reshape(-1, 2) for x in X]
            Y = [y[:, 0:2] for y in sc["truth"]]
            direct = gospa_steps(X, sc["truth"], 20, ctx=gpu_ctx)
            assert got["nIgnored"] == n_initial and np.array_equal(got["times"], sc["times"])
            for s, (a, b) in enumerate(zip(steps_of(got), steps_of(direct))):
                assert same_bits(a, b), s
                ref.hold(a, ref.reference(X[s], Y[s], 20.0), "scan %d%s" % (s, ", smoothed" if smooth else ""))
            assert np.array_equal(got["nAssigned"] + got["nMissed"], np.full(15, 8))
            assert [len(t) for t in got["trackIds"]] == [len(x) for x in X]
            assert got["idSwitches"][0] == sum(got["idSwitches"][1].values()) >= 0
            assert got["meanLocalisation"] == float(np.mean(got["localisation"])) and got["meanGospa"] == float(np.mean(got["gospa"]))
            means[smooth] = got["meanLocalisation"]
            print("smooth=%s: mean GOSPA %.4f, mean localisation %.4f, missed %.4f, false %.4f, id switches %d, ignored %d"
                  % (smooth, got["meanGospa"], got["meanLocalisation"], got["meanMissed"], got["meanFalse"], got["idSwitches"][0], got["nIgnored"]))
        print("mean localisation error (sum of d^2 per scan): filtered %.4f, smoothed %.4f" % (means[False], means[True]))
        with pytest.raises(ValueError, match="smooth"):
            trk.getGospa(truth, c=20, constantTurn=True)
        with pytest.raises(ValueError, match="constant-turn"):
            trk.getGospa(truth, c=20, smooth=True, constantTurn=True)
    finally:
        trk.close()
