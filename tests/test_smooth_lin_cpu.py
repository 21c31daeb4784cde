"""CPU: the linear smoother's walk and arithmetic (csrc/mht_smooth_walk.h: smooth_walk with LinearSteps, the code a lane of
smooth_rts_kernel runs) compiled for the host and held to the criterion of tests/test_smooth_gpu.py on that test's own accuracy batch;
and the AIS policy on a batch without messages against it, bit for bit -- the CPU twin of
tests/test_smooth_ais_gpu.py::test_without_a_message_the_output_is_the_linear_smoothers_bit_for_bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import smooth_ref as sr
from test_smooth_ais_cpu import _host_smooth as _host_smooth_ais

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 2.5
FACTOR = 8.0      # (tests/test_smooth_gpu.py's)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    so = str(tmp_path_factory.mktemp("smooth_host") / "libsmooth_host.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "hostmath", "smooth_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.smooth_lin_host.restype = None
    lib.smooth_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
    lib.smooth_ais_host.restype = None
    lib.smooth_ais_host.argtypes = [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 11 + [C.c_int32]
    return lib


def _host_smooth(lib, model, x0, P0, z, cov=True):
    A, Q, Cm, R = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in sr.model_matrices(model, PERIOD)]
    nx, L = A.shape[0], len(z)
    ns = nx * (nx + 1) // 2
    has = sr.detected(z)
    has[0] = False
    zz = np.ascontiguousarray(np.where(has[:, None], z, 0.0))
    hz = np.ascontiguousarray(has.astype(np.uint8))
    x0, P0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(P0, dtype=np.float64)
    xs, Pp = np.full((L, nx), -7.0), np.full((L, ns), -7.0)
    lib.smooth_lin_host(nx, A.ctypes.data, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, L, x0.ctypes.data, P0.ctypes.data, zz.ctypes.data,
                        hz.ctypes.data, xs.ctypes.data, Pp.ctypes.data, 1 if cov else 0)
    Ps = np.empty((L, nx, nx))
    iu = np.triu_indices(nx)
    Ps[:, iu[0], iu[1]] = Pp
    Ps[:, iu[1], iu[0]] = Pp
    return xs, Ps, Pp


@pytest.mark.parametrize("name", ["pv", "ca"])
def test_device_walk_on_the_host_meets_the_accuracy_criterion(lib, name):
    """The 40 tracks of tests/test_smooth_gpu.py::test_accuracy_against_the_longdouble_truth, one at a time: e <= 8 e_np against the
    longdouble truth, means and covariances separately, as on the device."""
    from pymht_amd.models import pv, ca
    model = {"pv": pv, "ca": ca}[name]
    assert np.finfo(np.longdouble).eps < 1e-18
    rng = np.random.default_rng(20240)
    lengths = [int(v) for v in rng.integers(2, 401, 40)]
    tracks = sr.make_batch(model, PERIOD, lengths, seed=17, p_detect=0.8)
    mats = sr.model_matrices(model, PERIOD)
    truth = [sr.rts(*mats, x0, P0, z, dtype=np.longdouble) for x0, P0, z in tracks]
    f64 = [sr.rts(*mats, x0, P0, z, dtype=np.float64) for x0, P0, z in tracks]
    got = [_host_smooth(lib, model, *t) for t in tracks]
    e_h = (max(sr.err(g[0], t["xs"]) for g, t in zip(got, truth)), max(sr.err(g[1], t["Ps"]) for g, t in zip(got, truth)))
    e_np = (max(sr.err(f["xs"], t["xs"]) for f, t in zip(f64, truth)), max(sr.err(f["Ps"], t["Ps"]) for f, t in zip(f64, truth)))
    print("host build of the device walk, models/%s: means e %.3g e_np %.3g ratio %.3g | covariances e %.3g e_np %.3g ratio %.3g"
          % (name, e_h[0], e_np[0], e_h[0] / e_np[0], e_h[1], e_np[1], e_h[1] / e_np[1]))
    assert e_h[0] <= FACTOR * e_np[0] and e_h[1] <= FACTOR * e_np[1]
    # means only: the same means, bit for bit, and the covariance output untouched; one node: output = input
    x0, P0, z = tracks[3]
    xs_m, _, packed = _host_smooth(lib, model, x0, P0, z, cov=False)
    assert np.array_equal(xs_m, got[3][0]) and (packed == -7.0).all()
    xs1, Ps1, _ = _host_smooth(lib, model, x0, P0, z[:1])
    assert np.array_equal(xs1[0], x0) and np.array_equal(Ps1[0], P0)


def test_without_a_message_the_ais_walk_is_the_linear_one_bit_for_bit(lib):
    """The batch of the GPU test: the plain step of the AIS policy is the linear policy's, the same arithmetic in the same order."""
    from pymht_amd.models import pv
    rng = np.random.default_rng(8)
    lengths = [1, 2, 200] + [int(v) for v in rng.integers(1, 120, 97)]
    tracks = sr.make_batch(pv, PERIOD, lengths, seed=12, p_detect=0.8)
    for cov in (True, False):
        for x0, P0, z in tracks:
            xs, _, packed = _host_smooth(lib, pv, x0, P0, z, cov=cov)
            xs_a, _, packed_a = _host_smooth_ais(lib, pv, x0, P0, z, [None] * len(z), cov=cov)
            assert np.array_equal(xs, xs_a) and np.array_equal(packed, packed_a)
            assert cov or (packed == -7.0).all()
