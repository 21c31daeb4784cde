"""CPU: the AIS-aware smoother's yardstick (tests/smooth_ais_ref.py) against itself in np.longdouble and against the linear reference
where the two must be the same; the device arithmetic itself (csrc/mht_smooth_ais_math.h) compiled for the host and held to the criterion
of tests/test_smooth_ais_gpu.py; and the errors the Python layer raises before it needs a device."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import smooth_ais_ref as sa
import smooth_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = sa.ACCURACY_PERIOD
FACTOR = 8.0


@pytest.fixture(scope="module")
def batch_refs():
    pv, tracks = sa.accuracy_batch()
    truth, f64 = sa.references(pv, PERIOD, tracks)
    return pv, tracks, truth, f64


def test_batch_covers_both_kinds_both_classes_and_the_ends(batch_refs):
    pv, tracks, truth, f64 = batch_refs
    assert len(tracks) == 40 and min(len(t[2]) for t in tracks) >= 2 and max(len(t[2]) for t in tracks) <= 400
    kinds = [sa.kinds(z, ais) for _, _, z, ais in tracks]
    allk = np.concatenate([k[1:] for k in kinds])
    counts = [int((allk == v).sum()) for v in range(4)]
    print("nodes per kind 0..3:", counts)
    assert counts[2] >= 100 and counts[3] >= 100 and counts[0] >= 1 and counts[1] >= 100
    assert 0.25 <= (counts[2] + counts[3]) / len(allk) <= 0.35
    high = [bool(a[3]) for t in tracks for a in t[3] if a is not None]
    assert sum(high) >= 100 and len(high) - sum(high) >= 100      # both accuracy classes
    assert len({(a[0], a[1]) for t in tracks for a in t[3] if a is not None}) == 3      # three message instants inside the period
    assert any(k[1] >= 2 for k in kinds), "no track whose node 1 is an AIS node"
    assert any(k[-1] >= 2 for k in kinds), "no track whose last node is an AIS node"
    for x0, P0, z, ais in tracks:
        assert z.dtype == np.float64 and np.isnan(z[0]).all() and ais[0] is None
        seen = ~np.isnan(z).any(axis=1)
        assert np.array_equal(z[seen], z[seen].astype(np.float32).astype(np.float64))      # float32-valued plots ...
        for a in ais:
            if a is not None:      # ... and messages, strictly inside the period
                assert np.array_equal(a[2], a[2].astype(np.float32).astype(np.float64)) and a[0] > 0 and a[1] > 0 and a[0] + a[1] == PERIOD


def test_reference_recursion_is_self_consistent(batch_refs):
    pv, tracks, truth, f64 = batch_refs
    assert np.finfo(np.longdouble).eps < 1e-18
    assert truth[0]["xs"].dtype == np.longdouble
    e_x = max(sr.err(f["xs"], t["xs"]) for f, t in zip(f64, truth))
    e_P = max(sr.err(f["Ps"], t["Ps"]) for f, t in zip(f64, truth))
    print("float64 reference against longdouble: means %.3g covariances %.3g" % (e_x, e_P))
    assert 0 < e_x < 1e-9 and 0 < e_P < 1e-9
    tr = lambda M: np.trace(M, axis1=1, axis2=2)
    for f in f64:
        assert np.all(tr(f["Ps"]) <= tr(f["Pf"]) * (1 + 1e-9))
        assert np.array_equal(f["xs"][-1], f["xf"][-1]) and np.array_equal(f["Ps"][-1], f["Pf"][-1])
    x0, P0, z, ais = tracks[1]
    one = sa.rts_ais(pv, PERIOD, x0, P0, z[:1], ais[:1])
    assert np.array_equal(one["xs"][0], x0) and np.array_equal(one["Ps"][0], P0)


def test_messages_change_the_result_and_shrink_the_covariance(batch_refs):
    """The yardstick is not the radar-only recursion in disguise: with its messages a track's smoothed covariance is smaller."""
    pv, tracks, truth, f64 = batch_refs
    mats = sr.model_matrices(pv, PERIOD)
    tr = lambda M: np.trace(M, axis1=1, axis2=2)
    for (x0, P0, z, ais), f in zip(tracks, f64):
        if sum(a is not None for a in ais) < 3:
            continue
        lin = sr.rts(*mats, x0, P0, z)
        assert not np.array_equal(lin["xs"], f["xs"]) and tr(f["Ps"]).sum() < tr(lin["Ps"]).sum()


def test_without_a_message_the_reference_is_the_linear_one_bit_for_bit():
    from pymht_amd.models import pv
    mats = sr.model_matrices(pv, PERIOD)
    for dtype in (np.float64, np.longdouble):
        for x0, P0, z in sr.make_batch(pv, PERIOD, [1, 2, 37, 150], seed=4):
            a, b = sa.rts_ais(pv, PERIOD, x0, P0, z, [None] * len(z), dtype=dtype), sr.rts(*mats, x0, P0, z, dtype=dtype)
            for key in ("xs", "Ps", "xf", "Pf"):
                assert a[key].dtype == dtype and np.array_equal(a[key], b[key]), key


def _host_lib(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    so = str(tmp_path_factory.mktemp("smooth_ais_host") / "libsmooth_ais_host.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "smooth_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.smooth_ais_host.restype = None
    lib.smooth_ais_host.argtypes = [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 11 + [C.c_int32]
    return lib


def _host_smooth(lib, model, x0, P0, z, ais, cov=True):
    """One track through the host build, its inputs packed by the Python layer's own host-side code (smoothing._ais_inputs)."""
    from pymht_amd.smoothing import _ais_inputs
    A, Q, Cm, R = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in sr.model_matrices(model, PERIOD)]
    ((has_m, msg, r, leg),), legs = _ais_inputs(model, [(x0, P0, z, ais)])
    L = len(z)
    has = sr.detected(z)
    has[0] = False
    zz = np.ascontiguousarray(np.where(has[:, None], z, 0.0))
    hz = np.ascontiguousarray(has.astype(np.uint8))
    kind = np.ascontiguousarray(hz + 2 * has_m.astype(np.uint8))
    assert np.array_equal(kind, sa.kinds(z, ais))
    msg, r, leg, legs = [np.ascontiguousarray(a) for a in (msg, r, leg, legs)]
    x0, P0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(P0, dtype=np.float64)
    xs, Pp = np.full((L, 4), -7.0), np.full((L, 10), -7.0)
    lib.smooth_ais_host(A.ctypes.data, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, L, x0.ctypes.data, P0.ctypes.data, zz.ctypes.data,
                        hz.ctypes.data, kind.ctypes.data, msg.ctypes.data, r.ctypes.data, leg.ctypes.data, legs.ctypes.data,
                        xs.ctypes.data, Pp.ctypes.data, 1 if cov else 0)
    Ps = np.empty((L, 4, 4))
    iu = np.triu_indices(4)
    Ps[:, iu[0], iu[1]] = Pp
    Ps[:, iu[1], iu[0]] = Pp
    return xs, Ps, Pp


def test_device_arithmetic_on_the_host_meets_the_accuracy_criterion(batch_refs, tmp_path_factory):
    """csrc/mht_smooth_ais_math.h compiled for the host, one track at a time: e <= 8 e_np against the longdouble truth, means and
    covariances separately, as on the device."""
    pv, tracks, truth, f64 = batch_refs
    assert np.finfo(np.longdouble).eps < 1e-18
    lib = _host_lib(tmp_path_factory)
    got = [_host_smooth(lib, pv, *t) for t in tracks]
    e_h = (max(sr.err(g[0], t["xs"]) for g, t in zip(got, truth)), max(sr.err(g[1], t["Ps"]) for g, t in zip(got, truth)))
    e_np = (max(sr.err(f["xs"], t["xs"]) for f, t in zip(f64, truth)), max(sr.err(f["Ps"], t["Ps"]) for f, t in zip(f64, truth)))
    print("host build of the device arithmetic: means e %.3g e_np %.3g ratio %.3g | covariances e %.3g e_np %.3g ratio %.3g"
          % (e_h[0], e_np[0], e_h[0] / e_np[0], e_h[1], e_np[1], e_h[1] / e_np[1]))
    assert e_h[0] <= FACTOR * e_np[0] and e_h[1] <= FACTOR * e_np[1]
    # means only: the same means, bit for bit, and the covariance output untouched; one node: output = input
    x0, P0, z, ais = tracks[3]
    xs_m, _, packed = _host_smooth(lib, pv, x0, P0, z, ais, cov=False)
    assert np.array_equal(xs_m, got[3][0]) and (packed == -7.0).all()
    xs1, Ps1, _ = _host_smooth(lib, pv, x0, P0, z[:1], ais[:1])
    assert np.array_equal(xs1[0], x0) and np.array_equal(Ps1[0], P0)


def test_host_side_packing_builds_one_leg_entry_per_time_pair():
    from pymht_amd.models import pv
    from pymht_amd.smoothing import _ais_inputs
    m = np.arange(4.0)
    tracks = [(np.zeros(4), pv.P0, [None] * 4, [None, (0.625, 1.875, m, True), None, (1.25, 1.25, m + 1, False)]),
              (np.zeros(4), pv.P0, [None] * 3, [(9.0, -1.0, m, True), (0.625, 1.875, m, False), None])]      # (entry 0 is not looked at)
    per_track, legs = _ais_inputs(pv, tracks)
    assert legs.shape == (2, 52) and legs.dtype == np.float64
    iu = np.triu_indices(4)
    f = lambda a: np.asarray(a, dtype=np.float64)
    assert np.array_equal(legs[0], np.concatenate([f(pv.Phi(0.625)).ravel(), f(pv.Q(0.625))[iu], f(pv.Phi(1.875)).ravel(), f(pv.Q(1.875))[iu]]))
    assert np.array_equal(legs[1][:16], f(pv.Phi(1.25)).ravel()) and np.array_equal(legs[1][42:], f(pv.Q(1.25))[iu])
    (has0, msg0, r0, leg0), (has1, msg1, r1, leg1) = per_track
    assert has0.tolist() == [False, True, False, True] and leg0.tolist() == [0, 0, 0, 1] and r0.tolist() == [1.0, 1.0, 1.0, 9.0]
    assert np.array_equal(msg0[3], m + 1) and has1.tolist() == [False, True, False] and r1[1] == 9.0 and leg1[1] == 0


def test_errors_are_raised_before_a_device_is_needed():
    from pymht_amd.models import pv, ca, ct
    from pymht_amd.smoothing import smooth_tracks_ais, smooth_nodes
    from pymht_amd.pyTarget import Target
    msg = np.zeros(4)
    for model, nx in ((ca, 6), (ct, 6)):      # not a 4-state linear model
        with pytest.raises(ValueError, match="4-state linear"):
            smooth_tracks_ais(model, PERIOD, [(np.zeros(nx), model.P0, [None, np.zeros(2)], [None, (1.0, 1.5, msg, True)])])
    for dT1, dT2 in ((0.0, 2.5), (2.5, 0.0), (-0.5, 3.0), (3.0, -0.5), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="positive"):
            smooth_tracks_ais(pv, PERIOD, [(np.zeros(4), pv.P0, [None, np.zeros(2)], [None, (dT1, dT2, msg, True)])])
    with pytest.raises(ValueError, match="AIS entries"):
        smooth_tracks_ais(pv, PERIOD, [(np.zeros(4), pv.P0, [None, np.zeros(2)], [None])])
    assert smooth_tracks_ais(pv, PERIOD, []) == []
    tgt = Target(0.0, None, np.zeros(4), pv.P0)
    with pytest.raises(ValueError, match="Tracker"):      # a node no tracker stands behind has no AIS history
        tgt.getSmoothTrack(PERIOD, ais=True)
    with pytest.raises(ValueError, match="constantTurn"):
        smooth_nodes(pv, PERIOD, [tgt], constantTurn=True, ais=lambda scan, mmsi: None)
    # a node that took a message the look-up does not have is never smoothed as radar-only
    kid = Target(2.5, 1, np.zeros(4), pv.P0, parent=tgt, mmsi=257000001)
    with pytest.raises(RuntimeError, match="257000001"):
        smooth_nodes(pv, PERIOD, [kid], ais=lambda scan, mmsi: None)


def test_the_keyword_defaults_to_off_everywhere():
    from pymht_amd import smoothing
    from pymht_amd.pyTarget import Target
    from pymht_amd.tracker import Tracker
    assert inspect.signature(smoothing.smooth_nodes).parameters["ais"].default is None
    for fn in (Tracker.getSmoothTracks, Tracker._storeRun, Target.getSmoothTrack):
        assert inspect.signature(fn).parameters["ais"].default is False
