"""GPU: the device Rauch-Tung-Striebel smoother (`mht_smooth_tracks`, include/mht_amd.h seam (v); pymht_amd/smoothing.py) against its NumPy
restatement tests/smooth_ref.py, and the drop-in path on top of it (Target.getSmoothTrack, Tracker.getSmoothTracks, the <SmoothedStates>
of _storeRun(smooth=True)).

There is no bit-exact target: the device's operation order is its own (fused multiply-adds, a Cholesky solve where the reference inverts).
The tolerance is therefore relative to what float64 itself can do.  With the np.longdouble (80-bit) evaluation of the recursion as the
truth, over a whole batch
    e_dev = max |device - truth| / (1 + |truth|),   e_np = the same for the float64 NumPy evaluation,
means and covariances separately, and the requirement is  e_dev <= 8 * e_np  (three bits: a float32 intermediate or a wrong operand
misses it by orders of magnitude).  The float64 reference sets the scale, not the device.  Every test prints the ratios it measured."""
import ctypes as C
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import smooth_ref as sr

pytestmark = pytest.mark.gpu

PERIOD = 2.5
FACTOR = 8.0


def _model(name):
    from pymht_amd.models import pv, ca
    return {"pv": pv, "ca": ca}[name]


@pytest.fixture(scope="module")
def ctxs():
    """One context per library build: the seam takes nx at run time, so both builds run both models."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (pymht_amd has no CPU fallback)")
    from pymht_amd.device import Context
    c = {4: Context(0, nx=4), 6: Context(0, nx=6)}
    yield c
    for v in c.values():
        v.close()


def _truth_is_better_than_float64():
    eps = float(np.finfo(np.longdouble).eps)
    assert eps < 1e-18, "np.longdouble is no wider than float64 here (eps %.3g): the accuracy criterion would be empty" % eps


def _references(model, tracks):
    mats = sr.model_matrices(model, PERIOD)
    truth = [sr.rts(*mats, x0, P0, z, dtype=np.longdouble) for x0, P0, z in tracks]
    f64 = [sr.rts(*mats, x0, P0, z, dtype=np.float64) for x0, P0, z in tracks]
    return truth, f64


def _worst(got, truth, key):
    return max(sr.err(g, t[key]) for g, t in zip(got, truth))


def _check(label, dev, truth, f64):
    """The criterion of the module docstring over a batch; dev = [(xs, Ps)]."""
    e_dev = (_worst([d[0] for d in dev], truth, "xs"), _worst([d[1] for d in dev], truth, "Ps"))
    e_np = (_worst([f["xs"] for f in f64], truth, "xs"), _worst([f["Ps"] for f in f64], truth, "Ps"))
    print("%s: means e_dev %.3g e_np %.3g ratio %.3g | covariances e_dev %.3g e_np %.3g ratio %.3g"
          % (label, e_dev[0], e_np[0], e_dev[0] / e_np[0] if e_np[0] else 0.0, e_dev[1], e_np[1], e_dev[1] / e_np[1] if e_np[1] else 0.0))
    assert e_dev[0] <= FACTOR * e_np[0], "%s: means: e_dev %.3g > %g x e_np %.3g" % (label, e_dev[0], FACTOR, e_np[0])
    assert e_dev[1] <= FACTOR * e_np[1], "%s: covariances: e_dev %.3g > %g x e_np %.3g" % (label, e_dev[1], FACTOR, e_np[1])
    return e_dev, e_np


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_accuracy_against_the_longdouble_truth(ctxs, name, lib_nx):
    """40 tracks of 2 .. 400 nodes, 80 % detections, T = 2.5 (the batch the criterion was stated for)."""
    from pymht_amd.smoothing import smooth_tracks
    _truth_is_better_than_float64()
    model = _model(name)
    rng = np.random.default_rng(20240)
    lengths = [int(v) for v in rng.integers(2, 401, 40)]
    tracks = sr.make_batch(model, PERIOD, lengths, seed=17, p_detect=0.8)
    dev = smooth_tracks(model, PERIOD, tracks, ctx=ctxs[lib_nx])
    truth, f64 = _references(model, tracks)
    _check("accuracy models/%s, %d-state build" % (name, lib_nx), dev, truth, f64)


@pytest.mark.parametrize("lib_nx", [4, 6])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_mixed_batch_shapes_and_properties(ctxs, name, lib_nx):
    """One call with lengths from 1 to several hundred, more tracks than a wavefront has lanes and not a multiple of 64; tracks never
    detected after node 0, tracks always detected; plus the properties that need no reference."""
    from pymht_amd.smoothing import smooth_tracks
    _truth_is_better_than_float64()
    model = _model(name)
    rng = np.random.default_rng(5)
    lengths = [1, 2, 300, 1, 2, 3, 250] + [int(v) for v in rng.integers(1, 90, 123)]
    n = len(lengths)
    assert n == 130 and n > 64 and n % 64 != 0
    p_detect = np.full(n, 0.8)
    never, always = [1, 5, 9, 20, 40, 70, 100], [2, 6, 10, 21, 41, 71, 101]
    p_detect[never], p_detect[always] = 0.0, 1.0
    tracks = sr.make_batch(model, PERIOD, lengths, seed=23, p_detect=p_detect)
    dev = smooth_tracks(model, PERIOD, tracks, ctx=ctxs[lib_nx])
    truth, f64 = _references(model, tracks)
    label = "mixed models/%s, %d-state build" % (name, lib_nx)
    e_dev, e_np = _check(label, dev, truth, f64)
    nx = np.asarray(model.C_RADAR).shape[1]
    for (x0, P0, z), (xs, Ps) in zip(tracks, dev):
        assert xs.shape == (len(z), nx) and Ps.shape == (len(z), nx, nx) and xs.dtype == np.float64 and Ps.dtype == np.float64
        if len(z) == 1:      # nothing to smooth: output = input, exactly
            assert np.array_equal(xs[0], x0) and np.array_equal(Ps[0], P0)
        assert np.array_equal(Ps, Ps.transpose(0, 2, 1)), "Ps is not symmetric"
    # never detected: the smoothed covariance IS the filtered (= predicted) one, so Ps_0 = P_init; measured like everything else -- the
    # device's error against the truth's Pf within FACTOR of the float64 reference's own
    sub = [t for t in never if lengths[t] > 1]
    assert sub
    e_d = max(sr.err(dev[t][1], truth[t]["Pf"]) for t in sub)
    e_n = max(sr.err(f64[t]["Ps"], truth[t]["Pf"]) for t in sub)
    print("%s: never detected: Ps vs the truth's Pf: e_dev %.3g e_np %.3g" % (label, e_d, e_n))
    eps64 = float(np.finfo(np.float64).eps)      # (floor: where the float64 reference happens to be exact, one rounding of the format is the scale)
    assert e_d <= FACTOR * max(e_n, eps64)
    e_d0 = max(sr.err(dev[t][1][0], tracks[t][1]) for t in sub)
    e_n0 = max(sr.err(f64[t]["Ps"][0], tracks[t][1]) for t in sub)
    print("%s: never detected: Ps_0 vs P_init: e_dev %.3g e_np %.3g" % (label, e_d0, e_n0))
    assert e_d0 <= FACTOR * max(e_n0, eps64)
    for t in always:
        assert not np.isnan(tracks[t][2][1:]).any()
    # the last node is the forward filter's last node (same criterion, against the truth's filtered state)
    e_d = (max(sr.err(d[0][-1], t["xf"][-1]) for d, t in zip(dev, truth)), max(sr.err(d[1][-1], t["Pf"][-1]) for d, t in zip(dev, truth)))
    e_n = (max(sr.err(f["xf"][-1], t["xf"][-1]) for f, t in zip(f64, truth)), max(sr.err(f["Pf"][-1], t["Pf"][-1]) for f, t in zip(f64, truth)))
    print("%s: last node vs the filter's: means e_dev %.3g e_np %.3g | covariances e_dev %.3g e_np %.3g" % (label, e_d[0], e_n[0], e_d[1], e_n[1]))
    assert e_d[0] <= FACTOR * e_n[0] and e_d[1] <= FACTOR * e_n[1]
    # smoothing never adds uncertainty: trace(Ps_k) <= trace(Pf_k), Pf from the reference.  Slack 1e-9 relative: two orders above the
    # float64 reference's own covariance error on such batches (1e-13 .. 1e-11), nine below the traces themselves
    tr = lambda M: np.trace(M, axis1=1, axis2=2)
    for (xs, Ps), f in zip(dev, f64):
        assert np.all(tr(Ps) <= tr(f["Pf"]) * (1 + 1e-9) + 1e-9)
    # a track's result does not depend on its place in the batch or on its neighbours: permuting the batch permutes the outputs bit for bit
    perm = rng.permutation(n)
    dev_p = smooth_tracks(model, PERIOD, [tracks[i] for i in perm], ctx=ctxs[lib_nx])
    for j, i in enumerate(perm):
        assert np.array_equal(dev_p[j][0], dev[i][0]) and np.array_equal(dev_p[j][1], dev[i][1])
    # ... nor on the others being there at all, nor on whether the covariances are asked for
    alone = smooth_tracks(model, PERIOD, [tracks[2]], ctx=ctxs[lib_nx])[0]
    assert np.array_equal(alone[0], dev[2][0]) and np.array_equal(alone[1], dev[2][1])
    means = smooth_tracks(model, PERIOD, tracks, ctx=ctxs[lib_nx], covariances=False)
    for (xs, Ps), (xs_m, none) in zip(dev, means):
        assert none is None and np.array_equal(xs, xs_m)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_raw_abi_error_codes_leave_the_outputs_untouched(ctxs, lib_nx):
    import torch
    from pymht_amd import _lib
    from pymht_amd.models import pv
    ctx = ctxs[lib_nx]
    lib, dev = ctx.lib, ctx.device
    nx, n, L = 4, 3, 5
    keep = [np.ascontiguousarray(np.asarray(m, dtype=np.float32).ravel()) for m in sr.model_matrices(pv, PERIOD)]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    model = lambda nx_: _lib.MhtModelX(nx_, fp(keep[0]), fp(keep[1]), fp(keep[2]), fp(keep[3]), 0.0, 0.0, 0, PERIOD)
    x = torch.zeros((nx, n), dtype=torch.float64, device=dev)
    P = torch.eye(nx, dtype=torch.float64, device=dev).reshape(nx * nx, 1).repeat(1, n).contiguous()
    z = torch.zeros((L, 2, n), dtype=torch.float64, device=dev)
    h = torch.ones((L, n), dtype=torch.uint8, device=dev)
    xs = torch.full((L, nx, n), -7.0, dtype=torch.float64, device=dev)
    Ps = torch.full((L, nx * (nx + 1) // 2, n), -7.0, dtype=torch.float64, device=dev)
    need = int(lib.mht_smooth_work_bytes(nx, n, L))
    assert need > 0 and int(lib.mht_smooth_work_bytes(5, n, L)) == 0
    work = torch.zeros(need, dtype=torch.uint8, device=dev)

    def call(m, lens, work_bytes):
        lens = np.asarray(lens, dtype=np.int32)
        return lib.mht_smooth_tracks(ctx.handle, C.byref(m), n, L, lens.ctypes.data_as(C.c_void_p), x.data_ptr(), P.data_ptr(), z.data_ptr(),
                                     h.data_ptr(), xs.data_ptr(), Ps.data_ptr(), work.data_ptr(), work_bytes)

    untouched = lambda: bool((xs == -7.0).all()) and bool((Ps == -7.0).all())
    assert call(model(5), [5, 5, 5], need) == _lib.MHT_E_INVALID and untouched()
    assert call(model(4), [5, 0, 5], need) == _lib.MHT_E_INVALID and untouched()
    assert call(model(4), [5, 6, 5], need) == _lib.MHT_E_INVALID and untouched()
    assert call(model(4), [5, 5, 5], need - 1) == _lib.MHT_E_CAPACITY and untouched()
    assert b"workspace" in lib.mht_last_error()
    ct_like = model(4)
    ct_like.transition = 1
    assert call(ct_like, [5, 5, 5], need) == _lib.MHT_E_INVALID and untouched()
    assert call(model(4), [5, 2, 1], need) == _lib.MHT_OK
    got = xs.cpu().numpy()
    assert not (got[:, :, 0] == -7.0).any() and (got[2:, :, 1] == -7.0).all() and not (got[:2, :, 1] == -7.0).any() and (got[1:, :, 2] == -7.0).all()


# What every track seam of pymht_amd.smoothing._SEAMS returns for the six bad calls of the sweep below -- a null model, nx = 5, the other
# kind's transition, a length 0 and a length L + 1 in the middle track, a workspace one byte short -- as read off the library in front
# of the change that gave the seams one host path: -1 is MHT_E_INVALID, -3 MHT_E_CAPACITY, which only the smoothers return, and only for
# the workspace (mht_smooth_tracks_em* document MHT_E_INVALID for theirs, include/mht_amd.h).
SWEEP_CASES = ("null model", "nx", "transition", "length 0", "length L + 1", "workspace")
SWEEP_CODES = {
    "mht_smooth_tracks": (-1, -1, -1, -1, -1, -3), "mht_smooth_tracks_ct": (-1, -1, -1, -1, -1, -3), "mht_smooth_tracks_ais": (-1, -1, -1, -1, -1, -3),
    "mht_smooth_tracks_em": (-1, -1, -1, -1, -1, -1), "mht_smooth_tracks_em_ll": (-1, -1, -1, -1, -1, -1),
    "mht_score_tracks": (-1, -1, -1, -1, -1, -1), "mht_score_tracks_ct": (-1, -1, -1, -1, -1, -1), "mht_score_tracks_ais": (-1, -1, -1, -1, -1, -1),
    "mht_score_tracks_grid": (-1, -1, -1, -1, -1, -1), "mht_score_tracks_ct_grid": (-1, -1, -1, -1, -1, -1),
    "mht_trace_tracks": (-1, -1, -1, -1, -1, -1), "mht_trace_tracks_ct": (-1, -1, -1, -1, -1, -1), "mht_trace_tracks_ais": (-1, -1, -1, -1, -1, -1),
    "mht_filter_tracks": (-1, -1, -1, -1, -1, -1), "mht_filter_tracks_ct": (-1, -1, -1, -1, -1, -1), "mht_filter_tracks_ais": (-1, -1, -1, -1, -1, -1),
    "mht_imm_tracks": (-1, -1, -1, -1, -1, -1), "mht_imm_tracks_ct": (-1, -1, -1, -1, -1, -1),
    "mht_imm_smooth_tracks": (-1, -1, -1, -1, -1, -1), "mht_imm_smooth_tracks_ct": (-1, -1, -1, -1, -1, -1)}


@pytest.mark.parametrize("seam", sorted(SWEEP_CODES))
def test_every_track_seam_refuses_on_the_host_and_leaves_the_outputs_untouched(ctxs, seam):
    """One sweep over all track seams of the Python table at n = 3, L = 5 through the raw ABI, both builds: every bad call returns the
    code of SWEEP_CODES, leaves the -7 prefill of every output as it was and a message that starts with the seam's name; one good call
    returns MHT_OK.  Every bad call is refused on the host, before anything is launched."""
    import torch
    from pymht_amd import _lib, smoothing
    from pymht_amd.models import ct, pv
    assert sorted(SWEEP_CODES) == sorted(row[0] for row in smoothing._SEAMS.values())      # (the sweep is over ALL seams of the table)
    (family, kind), (_, sizer, takes_nx, takes_count) = next(item for item in smoothing._SEAMS.items() if item[1][0] == seam)
    assert (_lib.MHT_E_INVALID, _lib.MHT_E_CAPACITY) == (-1, -3)
    nx, n, L, r = 6 if kind == "ct" else 4, 3, 5, 2
    ns = nx * (nx + 1) // 2
    mx, keep = smoothing._model_x(ct if kind == "ct" else pv, PERIOD, nx, kind == "ct")
    host = lambda a: a.ctypes.data_as(C.c_void_p)
    Qm, Rm, Pi, mu0 = np.stack([np.eye(nx)] * r), np.stack([np.eye(2)] * r), np.full((r, r), 0.5), np.full(r, 0.5)
    for lib_nx in (4, 6):
        ctx = ctxs[lib_nx]
        lib, dev = ctx.lib, ctx.device
        f64 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
        i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=dev)
        x = torch.zeros((nx, n), dtype=torch.float64, device=dev)
        P = torch.eye(nx, dtype=torch.float64, device=dev).reshape(nx * nx, 1).repeat(1, n).contiguous()
        z = torch.zeros((L, 2, n), dtype=torch.float64, device=dev)
        h = torch.ones((L, n), dtype=torch.uint8, device=dev)
        extra, middle, trailing = (), (), ()
        if kind == "ais":      # no node took a message: kind = has_z, an empty leg table
            ais_z, ais_r = torch.zeros((L, 4, n), dtype=torch.float64, device=dev), torch.ones((L, n), dtype=torch.float64, device=dev)
            leg = torch.zeros((L, n), dtype=torch.int32, device=dev)
            extra = (h.data_ptr(), ais_z.data_ptr(), ais_r.data_ptr(), leg.data_ptr(), None, 0)
        if family == "smooth":
            outs = [f64(L, nx, n), f64(L, ns, n)]
        elif family in ("em", "em_ll"):
            middle, outs = (2,), [f64(L, nx, n), f64(L, ns, n), f64(ns, n), f64(3, n)]
            if family == "em_ll":
                outs.append(f64(3, n))
                trailing = (outs[-1].data_ptr(),)
        elif family == "score":
            outs = [f64(n), f64(n), i32(n)] + ([f64(n), i32(n)] if kind == "ais" else [])
        elif family == "score_grid":
            middle, outs = (r, host(Qm), host(Rm)), [f64(r, n), f64(r, n), i32(n)]
        elif family == "trace":
            outs = [f64(L, 7, n)] + ([f64(L, 16, n)] if kind == "ais" else [])
        elif family == "filter":
            outs = [f64(L, nx, n), f64(L, ns, n)]
        else:
            assert family in ("imm", "imm_smooth")
            middle = (r, host(Qm), host(Rm), host(Pi), host(mu0))
            outs = [f64(L, r, n), f64(L, nx, n), f64(L, ns, n)] + ([f64(L, r, n)] if family == "imm_smooth" else []) + [f64(n), i32(n)]
        need = int(getattr(lib, sizer)(*((nx,) if takes_nx else ()), n, L, *((r,) if takes_count else ())))
        assert need > 0
        work = torch.zeros(need, dtype=torch.uint8, device=dev)
        out_ptrs = [o.data_ptr() for o in outs[:len(outs) - len(trailing)]]

        def call(model, lens, work_bytes):
            lens = np.asarray(lens, dtype=np.int32)
            return getattr(lib, seam)(ctx.handle, model, n, L, host(lens), x.data_ptr(), P.data_ptr(), z.data_ptr(), h.data_ptr(), *extra, *middle,
                                      *out_ptrs, work.data_ptr(), work_bytes, *trailing)

        def altered(field, value):      # (a copy of the struct: it points into `keep` as mx does)
            m = _lib.MhtModelX.from_buffer_copy(mx)
            setattr(m, field, value)
            return m

        wrong_nx, wrong_transition = altered("nx", 5), altered("transition", 0 if kind == "ct" else 1)
        bad = {"null model": (None, [5, 5, 5], need), "nx": (C.byref(wrong_nx), [5, 5, 5], need),
               "transition": (C.byref(wrong_transition), [5, 5, 5], need), "length 0": (C.byref(mx), [5, 0, 5], need),
               "length L + 1": (C.byref(mx), [5, 6, 5], need), "workspace": (C.byref(mx), [5, 5, 5], need - 1)}
        for case, want in zip(SWEEP_CASES, SWEEP_CODES[seam]):
            model, lens, work_bytes = bad[case]
            rc = call(model, lens, work_bytes)
            torch.cuda.synchronize(dev)
            label = "%s, %d-state build, %s" % (seam, lib_nx, case)
            print("%s: %d" % (label, rc))
            assert rc == want, (label, rc, want)
            assert all(bool((o == -7).all()) for o in outs), label
            message = lib.mht_last_error()
            assert message and message.startswith(seam.encode() + b":"), (label, message)
            if case == "workspace":
                assert b"workspace" in message and sizer.encode() in message, (label, message)
        assert call(C.byref(mx), [5, 2, 1], need) == _lib.MHT_OK, seam
        torch.cuda.synchronize(dev)
        assert not bool((outs[0] == -7).all()), seam


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_filter_smooth_score_and_trace_agree_bit_for_bit_across_a_wavefront(ctxs, name, n):
    """Tracks of mixed lengths 1 .. 7, one wavefront's worth, one more and a single track, at four and at six states, all four families
    through one launch driver: a track's last filtered row is its last smoothed row, and its score is its trace added up in node
    order -- the same bits."""
    import smooth_trace_ref as tref
    from pymht_amd.smoothing import filter_tracks, score_tracks, smooth_tracks, trace_tracks
    model = _model(name)
    rng = np.random.default_rng(100 + n)
    lengths = [int(v) for v in rng.integers(1, 8, n)]
    if n > 1:
        lengths[0], lengths[-1] = 7, 1
    tracks = sr.make_batch(model, PERIOD, lengths, seed=31 + n, p_detect=0.8)
    ctx = ctxs[4 if name == "pv" else 6]
    smoothed, filtered = smooth_tracks(model, PERIOD, tracks, ctx=ctx), filter_tracks(model, PERIOD, tracks, ctx=ctx)
    scores, traces = score_tracks(model, PERIOD, tracks, ctx=ctx), trace_tracks(model, PERIOD, tracks, ctx=ctx)
    assert len(smoothed) == len(filtered) == len(scores) == len(traces) == n
    for L, (xs, Ps), (xf, Pf), score, trace in zip(lengths, smoothed, filtered, scores, traces):
        assert len(xs) == len(xf) == len(trace["ll"]) == L and not np.isnan(xf).any() and not np.isnan(Pf).any()
        assert np.array_equal(xf[-1], xs[-1]) and np.array_equal(Pf[-1], Ps[-1])
        s = tref.resum(trace)
        assert np.array_equal(np.array([s["ll"], s["nis"], s["nobs"]], dtype=np.float64), np.array(score, dtype=np.float64)), (s, score)


def _run_scenario():
    from pymht_amd.tracker import Tracker
    from pymht_amd.models import pv
    from pymht_amd.utils.classDefinitions import MeasurementList
    from pymht_amd.utils.scenario import make_scenario
    sc = make_scenario(T=30, radius=2000.0, lambda_phi=2e-6, n_scans=40, P_d=0.9, seed=4711)
    trk = Tracker(pv, sc["period"], sc["lambda_phi"], 1e-4, P_d=sc["P_d"], N=5, eta2=5.99)      # (the device M-of-N initiator starts the tracks)
    for zk, tk in zip(sc["scans"], sc["times"]):
        trk.addMeasurementList(MeasurementList(float(tk), zk))
    return trk, sc, pv


def test_drop_in_path_smooths_a_run_and_fills_the_export():
    _truth_is_better_than_float64()
    trk, sc, pv = _run_scenario()
    try:
        nodes = list(trk.getTrackNodes()) + list(trk.__terminatedTargets__)
        assert len(trk.getTrackNodes()) >= 10
        got = trk.getSmoothTracks(terminated=True)
        assert len(got) == len(nodes) and len(trk.getSmoothTracks()) == len(trk.getTrackNodes())
        mats = sr.model_matrices(pv, sc["period"])
        dev, truth, f64, longest = [], [], [], 0
        for i, (node, (pos, vel, ok)) in enumerate(zip(nodes, got)):
            chain = node.backtrackNodes()
            zs = node.backtrackMeasurement()
            assert len(zs) == len(chain) == len(pos) == len(vel)
            if len(chain) < 2:
                assert not ok and np.isnan(vel).all()
                continue
            assert ok
            first = chain[0]
            args = (first.x_0, pv.P0 if first.P_0 is None else first.P_0, zs)
            truth.append(sr.rts(*mats, *args, dtype=np.longdouble))
            f64.append(sr.rts(*mats, *args, dtype=np.float64))
            dev.append(np.concatenate([pos, vel], axis=1))
            if len(chain) > len(nodes[longest].backtrackNodes()):
                longest = i
        assert len(dev) >= 10 and max(len(d) for d in dev) >= 20
        e_dev, e_np = _worst(dev, truth, "xs"), _worst([f["xs"] for f in f64], truth, "xs")
        print("drop-in: %d tracks, longest %d nodes: means e_dev %.3g e_np %.3g ratio %.3g" % (len(dev), max(len(d) for d in dev), e_dev, e_np, e_dev / e_np))
        assert e_dev <= FACTOR * e_np
        # one node on its own: the same numbers as its row of the batch, bit for bit
        pos1, vel1, ok1 = nodes[longest].getSmoothTrack(trk.radarPeriod)
        assert ok1 and np.array_equal(pos1, got[longest][0]) and np.array_equal(vel1, got[longest][1])
        # the export: empty by default, one <S> per node with smooth=True, in the layout and at the precision of <States>
        scen = trk.getScenarioElement()
        trk._storeRun(scen)
        trk._storeRun(scen, smooth=True)
        plain, smooth = scen.findall("Run")
        assert len(plain.findall("Track")) == len(smooth.findall("Track")) == len(nodes)
        for tr_ in plain.findall("Track"):
            assert len(tr_.find("SmoothedStates")) == 0
        filled = 0
        for node, (pos, vel, ok), tr_ in zip(nodes, got, smooth.findall("Track")):
            states, sm = tr_.find("States"), tr_.find("SmoothedStates")
            assert len(states) == int(tr_.attrib["length"]) == len(pos)
            if len(states) < 2:
                assert len(sm) == 0
                continue
            assert len(sm) == len(states)
            filled += 1
            for s_el, f_el, p, v in zip(sm, states, pos, vel):
                assert s_el.tag == "S" and s_el.attrib["t"] == f_el.attrib["t"]
                assert [c.tag for c in s_el] == ["P", "V"] and [c.tag for c in s_el.find("P")] == ["N", "E"] == [c.tag for c in s_el.find("V")]
                assert float(s_el.find("P").find("E").text) == round(float(p[0]), 2) and float(s_el.find("P").find("N").text) == round(float(p[1]), 2)
                assert float(s_el.find("V").find("E").text) == round(float(v[0]), 2) and float(s_el.find("V").find("N").text) == round(float(v[1]), 2)
        assert filled >= 10
        ET.fromstring(ET.tostring(scen))      # (well-formed)
    finally:
        trk.close()


def test_constant_turn_tracker_refuses_to_smooth():
    from pymht_amd.tracker import Tracker
    from pymht_amd.pyTarget import Target
    from pymht_amd.models import ct
    trk = Tracker(ct, PERIOD, 1e-6, 1e-4, P_d=0.9, N=3, useInitiator=False)
    try:
        trk.initiateTarget(Target(1000.0, None, np.array([10.0, 20.0, 3.0, -2.0, 0.01, 0.0]), ct.P0, status="preinitialized"))
        with pytest.raises(NotImplementedError, match="ct"):
            trk.getSmoothTracks()
        with pytest.raises(NotImplementedError, match="ct"):
            trk._storeRun(trk.getScenarioElement(), smooth=True)
    finally:
        trk.close()
