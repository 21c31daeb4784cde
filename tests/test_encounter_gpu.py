"""GPU: the device encounters (`mht_encounters`, include/mht_amd.h; pymht_amd.evaluation.encounters) and the drop-in path on top
(Tracker.getEncounters), against tests/encounter_ref.py.

The criterion is the project's (tests/test_encounter_cpu.py states it and holds the host twin of the same header to it), per output
family: with the np.longdouble evaluation of the reference as the truth -- pc: mpmath at 30 digits with the rule's own 64 nodes --
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
and e_dev <= 8 * max(e_np, eps64); the NaN cells and the zeros of pc by the rule are the truth's exactly; tpc, an arg max, is held
by encounter_ref.hold_tpc.  On the tables too large for mpmath pc is held to the float64 reference with e_np from the mpmath case.
Every test prints the device's own ratios -- measured on an MI355X, tcpa / dcpa / md2 / pc:
    cells N 4, K 1 and 7     1 / 1 / 1 / 1.01    (e_np 4.6e-13 / 7.8e-14 / 1.7e-15 at K 7; pc's 6.1e-16 from the mpmath case)
    cells N 6, K 1 and 7     1 / 1 / 1 / 0.997   (e_np 8.0e-13 / 8.4e-14 / 4.7e-16 at K 7; pc's 1.0e-15)
    against mpmath           N 4: 1 / 1 / 1 / 1      N 6: 1 / 1 / 1 / 1
    getEncounters            all pairs 1 / 1 / 1 / 0.056      own ship 1 / 1 / 1 / 0.39
both builds alike: the device does the reference's operations in the reference's order, and its largest errors are the same cells'
-- and tools/encounter_cost.py writes them into profiles/encounter_cost.txt.  Nothing here is larger than 70 entries and 7 steps.  The shapes at which the kernels go round their grid-stride loops are
held in tests/test_encounter_strides_gpu.py."""
import numpy as np
import pytest

import encounter_ref as ref
from test_encounter_cpu import N_ENTRIES, RADIUS, hold, pc_case

pytestmark = pytest.mark.gpu

SENTINEL = -7.03125e10
DT = 5.0


@pytest.fixture(scope="module")
def ctxs():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (pymht_amd has no CPU fallback)")
    from pymht_amd.device import Context
    c = {4: Context(0, nx=4), 6: Context(0, nx=6)}
    yield c
    for v in c.values():
        v.close()


GUARD_BYTE = 0xA5


def guarded_work(need, guard, dev):
    """The work buffer of a raw call: `need` bytes (256 at least) and `guard` bytes behind them, all of it GUARD_BYTE -- as doubles about
    -1e-127 -- so that nothing a call forgets to write is found there from an earlier call"""
    import torch
    return torch.full((max(need, 256) + guard,), GUARD_BYTE, dtype=torch.uint8, device=dev)


def guard_untouched(work, need):
    return bool((work[max(need, 256):] == GUARD_BYTE).all())


def _raw(ctx, x, P, Phi, Q, K, dt, R, first=None, nulls=(), nx=None, n=None, short=0, guard=0):
    """One call of the seam on x [n, N], P [n, N, N], the output preset to SENTINEL: (return code, out [5, first, n]).  guard > 0: that
    many bytes of a pattern lie behind the sizer's figure and must be the pattern after the call."""
    import torch
    dev = ctx.device
    N = x.shape[1]
    n = len(x) if n is None else n
    first = n if first is None else first
    xp, Pp = ref.pack(x, P)
    Phi, Q = np.ascontiguousarray(Phi, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    arrays = dict(x=torch.from_numpy(xp).to(dev), P=torch.from_numpy(Pp).to(dev))
    out = torch.full((5, max(first, 0), max(n, 0)), SENTINEL, dtype=torch.float64, device=dev)
    need = int(ctx.lib.mht_encounter_work_bytes(len(x), min(max(K, 1), 64)))
    work = guarded_work(need, guard, dev)
    host = dict(Phi=Phi.ctypes.data, Q=Q.ctypes.data)
    ptr = lambda k: None if k in nulls else host[k] if k in host else arrays[k].data_ptr()
    torch.cuda.synchronize(dev)
    rc = ctx.lib.mht_encounters(ctx.handle, N if nx is None else nx, n, first, K, dt, R, ptr("Phi"), ptr("Q"), ptr("x"), ptr("P"),
                                None if "out" in nulls else out.data_ptr(), None if "work" in nulls else work.data_ptr(), need - short)
    torch.cuda.synchronize(dev)
    assert guard_untouched(work, need), "the call wrote behind the work buffer the sizer asks for"
    return rc, out.cpu().numpy()


_cases = {}


def cell_case(N, K):
    """encounter_ref.make_batch of models/pv or models/ca, 70 entries, all pairs, dt = 5, R = 80 (the cases of
    tests/test_encounter_cpu.py), evaluated once: (x, P, Phi, Q, truth, f64)"""
    if (N, K) not in _cases:
        from pymht_amd.models import ca, pv
        model = pv if N == 4 else ca
        x, P = ref.make_batch(model, N_ENTRIES, seed=3)
        Phi, Q = ref.model_matrices(model, DT)
        _cases[N, K] = (x, P, Phi, Q, ref.encounters(x, P, Phi, Q, K, DT, RADIUS, truth=True, pc_mp=False), ref.encounters(x, P, Phi, Q, K, DT, RADIUS))
    return _cases[N, K]


@pytest.mark.parametrize("N,K,lib_nx", [(4, 1, 4), (4, 7, 4), (4, 1, 6), (4, 7, 6), (6, 1, 6), (6, 7, 6), (6, 1, 4), (6, 7, 4)])
def test_cell_cases_meet_the_accuracy_criterion_and_every_cell_is_written(ctxs, N, K, lib_nx):
    """70 entries: a row of 70 cells straddles a wavefront, a tile of 256 lanes is partly filled.  first = 70, 3 and 1, the output
    preset to a sentinel, none left; tcpa, dcpa and md2 against the longdouble truth, pc against the float64 reference with e_np from
    the mpmath case; the special pairs -- a NaN in x, a NaN in P, identical states, P = 0 twice, a stationary pair, a CPA beyond the
    horizon and one at t = 0 -- as the reference has them; the rows of the first = 3 and first = 1 calls are the first rows of the
    full call bit for bit."""
    assert np.finfo(np.longdouble).eps < 1e-18
    x, P, Phi, Q, truth, f64 = cell_case(N, K)
    rc, out = _raw(ctxs[lib_nx], x, P, Phi, Q, K, DT, RADIUS)
    assert rc == 0 and not (out == SENTINEL).any()
    got = ref.seam_dict(out)
    hold("encounter cells N %d K %d, %d-state build" % (N, K, lib_nx), got, truth, f64, DT, pc_scale=pc_case(N)[8])
    ref.check_special_cells(got, K, DT)
    for first in (3, 1):
        rc, part = _raw(ctxs[lib_nx], x, P, Phi, Q, K, DT, RADIUS, first=first)
        assert rc == 0 and part.shape == (5, first, N_ENTRIES) and np.array_equal(part, out[:, :first], equal_nan=True)


@pytest.mark.parametrize("N,lib_nx", [(4, 4), (4, 6), (6, 6), (6, 4)])
def test_pc_and_tpc_against_mpmath(ctxs, N, lib_nx):
    """pc_case(N) of tests/test_encounter_cpu.py -- first = 4 of 70 entries, K = 4: 262 pairs, mpmath's truth computed once for both
    files -- every figure under the criterion, e_np the float64 reference's own error there."""
    x, P, Phi, Q, K, dt, truth, f64, e_np = pc_case(N)
    rc, out = _raw(ctxs[lib_nx], x, P, Phi, Q, K, dt, RADIUS, first=4)
    assert rc == 0 and not (out == SENTINEL).any()
    hold("encounters against mpmath N %d, %d-state build" % (N, lib_nx), ref.seam_dict(out), truth, f64, dt)


def test_raw_abi_errors_and_the_call_behind_them(ctxs):
    """A bad nx, K, R, dt or first, a null array, a work buffer one byte short: MHT_E_INVALID with the sentinel untouched; an empty
    call is MHT_OK and launches nothing; the sizer."""
    from pymht_amd import _lib
    ctx = ctxs[4]
    x, P, Phi, Q, _, _ = cell_case(4, 1)
    x, P = x[:6], P[:6]
    nan = float("nan")
    for kw in (dict(nx=5), dict(nx=3), dict(K=0), dict(K=65), dict(K=-1), dict(R=0.0), dict(R=-1.0), dict(R=nan), dict(dt=0.0), dict(dt=-2.0), dict(dt=nan),
               dict(first=7), dict(first=-1), dict(n=-1, first=0), dict(nulls=("Phi",)), dict(nulls=("Q",)), dict(nulls=("x",)), dict(nulls=("P",)),
               dict(nulls=("out",)), dict(nulls=("work",)), dict(short=1)):
        rc, out = _raw(ctx, x, P, Phi, Q, kw.get("K", 3), kw.get("dt", DT), kw.get("R", RADIUS), first=kw.get("first"), nulls=kw.get("nulls", ()),
                       nx=kw.get("nx"), n=kw.get("n"), short=kw.get("short", 0))
        assert rc == _lib.MHT_E_INVALID and ctx.lib.mht_last_error() and (out == SENTINEL).all(), kw
    assert ctx.lib.mht_encounters(ctx.handle, 4, 0, 0, 3, DT, RADIUS, None, None, None, None, None, None, 0) == _lib.MHT_OK
    rc, out = _raw(ctx, x, P, Phi, Q, 3, DT, RADIUS, first=0)
    assert rc == _lib.MHT_OK and out.shape == (5, 0, 6)
    for lib in (ctxs[4].lib, ctxs[6].lib):
        up = lambda b: (b + 255) // 256 * 256      # (5 (K + 1) n doubles, rounded up to 256 bytes)
        assert lib.mht_encounter_work_bytes(70, 7) == up(5 * 8 * 70 * 8) and lib.mht_encounter_work_bytes(3, 1) == 256
        assert lib.mht_encounter_work_bytes(2000, 24) == up(5 * 25 * 2000 * 8) and lib.mht_encounter_work_bytes(2000, 64) == up(5 * 65 * 2000 * 8)
        assert lib.mht_encounter_work_bytes(0, 3) == 0 and lib.mht_encounter_work_bytes(-1, 3) == 0
        assert lib.mht_encounter_work_bytes(5, 0) == 0 and lib.mht_encounter_work_bytes(5, 65) == 0
    rc, out = _raw(ctx, x, P, Phi, Q, 3, DT, RADIUS)
    assert rc == _lib.MHT_OK and not (out == SENTINEL).any()


def test_module_function_gives_the_seams_bits(ctxs):
    """evaluation.encounters on a Context and on a device ordinal: the dict of the raw call's rows"""
    from pymht_amd import evaluation
    x, P, Phi, Q, _, _ = cell_case(6, 7)
    rc, out = _raw(ctxs[6], x, P, Phi, Q, 7, DT, RADIUS, first=3)
    assert rc == 0
    for kw in (dict(ctx=ctxs[6]), dict(device=0)):
        res = evaluation.encounters(x, P, Phi, Q, 7, DT, RADIUS, first=3, **kw)
        assert sorted(res) == sorted(ref.NAMES) and all(np.array_equal(res[k], out[f], equal_nan=True) for f, k in enumerate(ref.NAMES))
    assert evaluation.encounters(x, P, Phi, Q, 7, DT, RADIUS, ctx=ctxs[4])["pc"].shape == (N_ENTRIES, N_ENTRIES)


def test_tracker_encounters_of_a_short_run():
    """Six targets initiated from known states, five scans of their true positions plus unit noise (no clutter): two of them, 124 m
    apart at the last scan, meet 17.5 s after it; the others are kilometres away and opening.  getEncounters over 40 s, radius 50,
    all pairs and with an own ship: the figures are encounter_ref's on the tracker's own getFilteredTracks() last rows, under the
    criterion with mpmath's pc; the pair on the collision course has the largest pc and a tcpa inside the horizon."""
    from pymht_amd.models import pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    from pymht_amd.utils.classDefinitions import MeasurementList
    period, t0, horizon, radius = 2.5, 1000.0, 40.0, 50.0
    x0 = np.array([[0.0, 0.0, 5.0, 0.0], [150.0, -150.0, 0.0, 5.0], [2000.0, 2000.0, 6.0, 3.0], [-2000.0, 1800.0, -7.0, 2.0],
                   [-1900.0, -2100.0, -3.0, -8.0], [2200.0, -1700.0, 9.0, -4.0]])
    rng = np.random.default_rng(8)
    trk = Tracker(pv, period, 2e-6, 1e-4, P_d=0.9, N=3, eta2=5.99, useInitiator=False)
    try:
        for s in x0:
            trk.initiateTarget(Target(t0, None, s.copy(), pv.P0))
        for k in range(1, 6):
            z = x0[:, :2] + x0[:, 2:] * (k * period) + rng.normal(size=(6, 2))
            trk.addMeasurementList(MeasurementList(t0 + k * period, z))
        last = [(xf[-1], Pf[-1]) for xf, Pf in trk.getFilteredTracks()]
        assert len(last) == 6
        x, P = np.array([a for a, _ in last]), np.array([b for _, b in last])
        steps, dt = 16, 2.5
        Phi, Q = ref.model_matrices(pv, dt)
        got = trk.getEncounters(horizon, radius)
        assert sorted(got) == sorted(ref.NAMES + ("ids",)) and len(got["ids"]) == 6 and len(set(got["ids"])) == 6 and got["pc"].shape == (6, 6)
        truth, f64 = ref.encounters(x, P, Phi, Q, steps, dt, radius, truth=True), ref.encounters(x, P, Phi, Q, steps, dt, radius)
        hold("getEncounters, all pairs", {k: got[k] for k in ref.NAMES}, truth, f64, dt)
        pc = np.where(np.isnan(got["pc"]), -1.0, got["pc"])
        i, j = np.unravel_index(np.argmax(pc), pc.shape)
        near = [int(np.argmin(np.hypot(*(x[:, :2] - (x0[t, :2] + x0[t, 2:] * 5 * period)).T))) for t in (0, 1)]
        print("collision pair", (i, j), "pc", pc[i, j], "tcpa", got["tcpa"][i, j], "dcpa", got["dcpa"][i, j], "runner-up pc", np.sort(pc.ravel())[-2])
        assert sorted((i, j)) == sorted(near) and 0 < got["tcpa"][i, j] < horizon and pc[i, j] > 10 * np.sort(pc.ravel())[-2] and got["dcpa"][i, j] < radius
        # the own ship, on target 0's course 30 m abeam, as entry 0: one row
        own = np.array([x[near[0], 0], x[near[0], 1] + 30.0, 5.0, 0.0])
        cov = np.diag([4.0, 4.0])
        row = trk.getEncounters(horizon, radius, ownShip=own, ownCovariance=cov, steps=8)
        assert row["pc"].shape == (1, 7) and row["ids"][0] is None and row["ids"][1:] == got["ids"]
        Po = np.zeros((4, 4))
        Po[:2, :2] = cov
        xs, Ps = np.vstack([own, x]), np.concatenate([Po[None], P])
        Phi, Q = ref.model_matrices(pv, 5.0)
        truth, f64 = ref.encounters(xs, Ps, Phi, Q, 8, 5.0, radius, first=1, truth=True), ref.encounters(xs, Ps, Phi, Q, 8, 5.0, radius, first=1)
        hold("getEncounters, own ship", {k: row[k] for k in ref.NAMES}, truth, f64, 5.0)
        assert int(np.nanargmax(row["pc"][0])) == 1 + near[0] and row["pc"][0, 1 + near[0]] > 0.5
        two = trk.getEncounters(horizon, radius, ownShip=own[:2])
        assert two["pc"].shape == (1, 7) and np.isfinite(two["dcpa"][0, 1:]).all()
        for bad in (dict(horizon=0.0), dict(radius=-1.0), dict(steps=65), dict(steps=0), dict(ownShip=np.zeros(3)), dict(ownCovariance=np.eye(2)),
                    dict(ownShip=own, ownCovariance=np.eye(3))):
            kw = dict(horizon=horizon, radius=radius)
            kw.update(bad)
            with pytest.raises(ValueError, match="getEncounters"):
                trk.getEncounters(**kw)
    finally:
        trk.close()


def test_tracker_without_two_entries_makes_no_device_call():
    from pymht_amd.models import pv
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    trk = Tracker(pv, 2.5, 2e-6, 1e-4, P_d=0.9, N=3, eta2=5.99, useInitiator=False)
    try:
        none = trk.getEncounters(30.0, 50.0)
        assert none["ids"] == [] and all(none[k].shape == (0, 0) for k in ref.NAMES)
        own = trk.getEncounters(30.0, 50.0, ownShip=[0.0, 0.0, 1.0, 1.0])
        assert own["ids"] == [None] and all(own[k].shape == (1, 1) and np.isnan(own[k]).all() for k in ref.NAMES)
        trk.initiateTarget(Target(1000.0, None, np.array([10.0, 20.0, 1.0, 0.0]), pv.P0))
        one = trk.getEncounters(30.0, 50.0)
        assert len(one["ids"]) == 1 and all(one[k].shape == (1, 1) and np.isnan(one[k]).all() for k in ref.NAMES)
        both = trk.getEncounters(30.0, 50.0, ownShip=[0.0, 0.0, 1.0, 1.0])
        assert both["pc"].shape == (1, 2) and np.isfinite(both["dcpa"][0, 1]) and np.isnan(both["dcpa"][0, 0])
    finally:
        trk.close()
