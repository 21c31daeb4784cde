"""CPU: the EM walk (csrc/mht_smooth_em.h: smooth_em_walk, the walks the launches of smooth_em_kernel run per lane) compiled for the host
and held to the criterion of tests/test_smooth_em_gpu.py on that test's own batch, one track at a time; and with n_iter = 0 against the
linear walk's host twin, bit for bit.

The measured ratios e / max(e_np, eps) on this batch, n_iter = 5, are in the docstring of
test_em_walk_on_the_host_meets_the_accuracy_criterion."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import smooth_em_ref as er
import smooth_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 2.5
FACTOR = 8.0      # (the smoothers')


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    gxx = shutil.which("g++") or "g++"
    d = tmp_path_factory.mktemp("smooth_em_host")
    out = []
    for src in ("smooth_em_host.cpp", "smooth_host.cpp"):
        so = str(d / ("lib%s.so" % src[:-4]))
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", os.path.join(ROOT, "tests", "hostmath", src), "-o", so])
        out.append(C.CDLL(so))
    out[0].smooth_em_host.restype = None
    out[0].smooth_em_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 4
    out[1].smooth_lin_host.restype = None
    out[1].smooth_lin_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]
    return out


def _unpack(packed, nx):
    full = np.empty(packed.shape[:-1] + (nx, nx))
    iu = np.triu_indices(nx)
    full[..., iu[0], iu[1]] = packed
    full[..., iu[1], iu[0]] = packed
    return full


def host_em(lib, model, x0, P0, z, n_iter, start="model", cov=True):
    """One track through smooth_em_host: dict(xs, Ps (None without cov), Q, R) plus the packed Ps."""
    Q, R, P = er.start_values(model, PERIOD, P0, start)
    A, Q, Cm, R = [np.ascontiguousarray(np.asarray(m, dtype=np.float64)) for m in (model.Phi(PERIOD), Q, model.C_RADAR, R)]
    nx, L = A.shape[0], len(z)
    ns = nx * (nx + 1) // 2
    has = sr.detected(z)
    has[0] = False
    zz = np.ascontiguousarray(np.where(has[:, None], z, 0.0))
    hz = np.ascontiguousarray(has.astype(np.uint8))
    x0, P = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(P, dtype=np.float64)
    xs, Pp, Qp, Rp = np.full((L, nx), -7.0), np.full((L, ns), -7.0), np.full(ns, -7.0), np.full(3, -7.0)
    lib.smooth_em_host(nx, A.ctypes.data, Q.ctypes.data, Cm.ctypes.data, R.ctypes.data, L, x0.ctypes.data, P.ctypes.data, zz.ctypes.data,
                       hz.ctypes.data, n_iter, xs.ctypes.data, Pp.ctypes.data if cov else None, Qp.ctypes.data, Rp.ctypes.data)
    return dict(xs=xs, Ps=_unpack(Pp, nx) if cov else None, Q=_unpack(Qp, nx), R=Rp[[0, 1, 1, 2]].reshape(2, 2), packed=Pp)


@pytest.mark.parametrize("start", ["model", "reference"])
@pytest.mark.parametrize("name", ["pv", "ca"])
def test_em_walk_on_the_host_meets_the_accuracy_criterion(libs, name, start):
    """e <= 8 max(e_np, eps) against the longdouble evaluation of tests/smooth_em_ref.py, for xs, Ps, Q and R separately.
    Measured, host build (g++ -O2 -mfma), ratios e / max(e_np, eps64) for xs / Ps / Q / R, with e_np between 5.6e-13 and 1.5e-11:
        pv, start=model       1.15 / 0.80 / 2.88 / 1.43          pv, start=reference   1.15 / 1.09 / 1.13 / 0.99
        ca, start=model       1.26 / 1.20 / 0.08 / 1.03          ca, start=reference   1.14 / 0.58 / 0.17 / 1.98
    The worst is 2.88 (Q, pv from the model's start values): iterating costs the walk's own operation order nothing near the factor 8."""
    from pymht_amd.models import pv, ca
    model = {"pv": pv, "ca": ca}[name]
    assert np.finfo(np.longdouble).eps < 1e-18
    tracks, truth, f64 = er.accuracy_reference(model, PERIOD, start)
    _, one, never, always = er.accuracy_batch(model, PERIOD)
    got = [host_em(libs[0], model, *t, 5, start=start) for t in tracks]
    res = er.ratios(got, truth, f64)
    print("host build of the EM walk, models/%s, start=%s: " % (name, start)
          + " | ".join("%s e %.3g e_np %.3g ratio %.3g" % ((k,) + v) for k, v in res.items()))
    assert all(np.isfinite(g[k]).all() for g in got for k in ("xs", "Ps", "Q", "R"))
    for k, (e, e_np, ratio) in res.items():
        assert ratio <= FACTOR, (k, e, e_np, ratio)
    # one node: output = input, Q and R as given; never detected: R stays and Ps_0 is P_init under the criterion
    Q0, R0, P0 = er.start_values(model, PERIOD, tracks[one][1], start)
    assert np.array_equal(got[one]["xs"][0], tracks[one][0]) and np.array_equal(got[one]["Ps"][0], P0)
    assert np.array_equal(got[one]["Q"], Q0) and np.array_equal(got[one]["R"], R0)
    assert np.array_equal(got[never]["R"], R0) and not np.array_equal(got[never]["Q"], Q0)
    assert sr.err(got[never]["Ps"][0], P0) <= FACTOR * max(sr.err(f64[never]["Ps"][0], truth[never]["Ps"][0]), np.finfo(np.float64).eps)
    assert not np.array_equal(got[always]["R"], R0)
    # means only: the same means and the same learned Q and R, bit for bit
    m = host_em(libs[0], model, *tracks[7], 5, start=start, cov=False)
    assert np.array_equal(m["xs"], got[7]["xs"]) and np.array_equal(m["Q"], got[7]["Q"]) and np.array_equal(m["R"], got[7]["R"]) and (m["packed"] == -7.0).all()


@pytest.mark.parametrize("name", ["pv", "ca"])
def test_without_an_iteration_the_em_walk_is_the_linear_one_bit_for_bit(libs, name):
    from pymht_amd.models import pv, ca
    from test_smooth_lin_cpu import _host_smooth
    model = {"pv": pv, "ca": ca}[name]
    rng = np.random.default_rng(8)
    lengths = [1, 2, 200] + [int(v) for v in rng.integers(1, 120, 27)]
    for x0, P0, z in sr.make_batch(model, PERIOD, lengths, seed=12, p_detect=0.8):
        xs, _, packed = _host_smooth(libs[1], model, x0, P0, z)
        got = host_em(libs[0], model, x0, P0, z, 0)
        Q0, R0, _ = er.start_values(model, PERIOD, P0, "model")
        assert np.array_equal(got["xs"], xs) and np.array_equal(got["packed"], packed)
        assert np.array_equal(got["Q"], Q0) and np.array_equal(got["R"], R0)
