"""CPU: the seam table of pymht_amd/smoothing.py (`_SEAMS`: (family, kind) -> seam, sizer, the sizer's argument shape) against the
libraries, and what every public `*_tracks*` function does before it needs a device: an empty batch gives the documented empty value
without a Context, and the modes / candidates are checked even then."""
import numpy as np
import pytest

from pymht_amd import _lib, smoothing
from pymht_amd.models import ct, pv

PERIOD = 2.5
KINDS = {"smooth": 3, "em": 1, "em_ll": 1, "score": 3, "score_grid": 2, "trace": 3, "filter": 3, "imm": 2, "imm_smooth": 2}


def test_the_table_holds_every_family_and_kind():
    assert len(smoothing._SEAMS) == sum(KINDS.values()) == 20
    for family, count in KINDS.items():
        kinds = [k for f, k in smoothing._SEAMS if f == family]
        assert kinds == ["linear", "ct", "ais"][:count], (family, kinds)
    seams = [row[0] for row in smoothing._SEAMS.values()]
    assert len(set(seams)) == len(seams)


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_every_seam_and_sizer_is_exported_and_declared(lib_nx):
    lib = _lib.load(build_if_missing=False, nx=lib_nx)
    exported = set(_lib.exported_symbols())
    for key, (seam, sizer, takes_nx, takes_count) in smoothing._SEAMS.items():
        for name in (seam, sizer):
            assert name in exported, (key, name)
            assert getattr(lib, name).argtypes is not None, (key, name)
        assert getattr(lib, seam).restype is _lib.C.c_int and getattr(lib, sizer).restype is _lib.C.c_size_t, key
        assert len(getattr(lib, sizer).argtypes) == 2 + takes_nx + takes_count, key


@pytest.mark.parametrize("lib_nx", [4, 6])
def test_every_sizer_called_as_the_table_says_gives_a_size(lib_nx):
    lib = _lib.load(build_if_missing=False, nx=lib_nx)
    for (family, kind), (seam, sizer, takes_nx, takes_count) in smoothing._SEAMS.items():
        nx = 6 if kind == "ct" else 4
        need = int(getattr(lib, sizer)(*((nx,) if takes_nx else ()), 3, 5, *((2,) if takes_count else ())))
        assert need >= 256, (family, kind, need)      # (the lengths alone are rounded up to 256 bytes)


def _modes(nx, r=2):
    return np.stack([np.eye(nx)] * r), np.stack([np.eye(2)] * r), np.full((r, r), 1.0 / r), np.full(r, 1.0 / r)


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("a Context was asked for")
    monkeypatch.setattr(smoothing, "Context", refuse)


def test_an_empty_batch_gives_the_empty_value_without_a_device(no_device):
    s = smoothing
    for fn, model in ((s.smooth_tracks, pv), (s.smooth_tracks_ct, ct), (s.smooth_tracks_ais, pv), (s.smooth_tracks_em, pv),
                      (s.score_tracks, pv), (s.score_tracks_ct, ct), (s.score_tracks_ais, pv), (s.trace_tracks, pv), (s.trace_tracks_ct, ct),
                      (s.trace_tracks_ais, pv), (s.filter_tracks, pv), (s.filter_tracks_ct, ct), (s.filter_tracks_ais, pv)):
        got = fn(model, PERIOD, [])
        assert isinstance(got, list) and got == [], fn.__name__
    assert s.smooth_tracks_em(pv, PERIOD, [], likelihoods=True) == []
    assert s.smooth_tracks(pv, PERIOD, [], covariances=False) == []
    for fn, model, nx in ((s.imm_tracks, pv, 4), (s.imm_tracks_ct, ct, 6)):
        per, ll, nobs = fn(model, PERIOD, [], *_modes(nx))
        assert per == [] and ll.shape == (0,) and ll.dtype == np.float64 and nobs.shape == (0,) and nobs.dtype == np.int32, fn.__name__
    for fn, model, nx in ((s.imm_smooth_tracks, pv, 4), (s.imm_smooth_tracks_ct, ct, 6)):
        assert fn(model, PERIOD, [], *_modes(nx)) == [], fn.__name__
    for fn, model, nx in ((s.score_tracks_grid, pv, 4), (s.score_tracks_ct_grid, ct, 6)):
        Q, R = _modes(nx, 3)[:2]
        ll, nis, nobs = fn(model, PERIOD, [], Q, R)
        assert ll.shape == nis.shape == (3, 0) and nobs.shape == (0,) and nobs.dtype == np.int32, fn.__name__
    # the *_nodes functions over no node, and the public functions they are built on, agree
    assert s.smooth_nodes(pv, PERIOD, []) == s.score_nodes(pv, PERIOD, []) == s.trace_nodes(pv, PERIOD, []) == s.filter_nodes(pv, PERIOD, []) == []


def test_the_model_is_checked_in_front_of_everything_else(no_device):
    s = smoothing
    with pytest.raises(NotImplementedError):
        s.smooth_tracks(ct, PERIOD, [])
    with pytest.raises(ValueError, match="transition"):
        s.filter_tracks_ct(pv, PERIOD, [])
    with pytest.raises(ValueError, match="four states"):
        s.score_tracks_ais(ct, PERIOD, [])
    with pytest.raises(NotImplementedError):      # (the model in front of the modes)
        s.imm_tracks(ct, PERIOD, [], "no modes", None, None)
    with pytest.raises(ValueError, match="AIS-aware track"):      # (the AIS inputs without a device, in front of the early return's batch)
        s.trace_tracks_ais(pv, PERIOD, [(np.zeros(4), np.eye(4), [None, None])])


def test_bad_modes_and_candidates_are_refused_on_an_empty_batch(no_device):
    s = smoothing
    for fn, model, nx in ((s.imm_tracks, pv, 4), (s.imm_tracks_ct, ct, 6), (s.imm_smooth_tracks, pv, 4), (s.imm_smooth_tracks_ct, ct, 6)):
        Q, R, Pi, mu0 = _modes(nx)
        with pytest.raises(ValueError, match="Pi holds probabilities"):
            fn(model, PERIOD, [], Q, R, Pi * 0.5, mu0)
        with pytest.raises(ValueError, match="mu0 holds probabilities"):
            fn(model, PERIOD, [], Q, R, Pi, mu0 * 2.0)
        with pytest.raises(ValueError, match="modes a call"):
            fn(model, PERIOD, [], *_modes(nx, 5))
        with pytest.raises(ValueError, match="candidates are"):
            fn(model, PERIOD, [], Q[:, :3, :3], R, Pi, mu0)
    for fn, model, nx in ((s.score_tracks_grid, pv, 4), (s.score_tracks_ct_grid, ct, 6)):
        Q, R = _modes(nx)[:2]
        skew = Q.copy()
        skew[1, 0, 1] = 0.5
        with pytest.raises(ValueError, match="not symmetric"):
            fn(model, PERIOD, [], skew, R)
        with pytest.raises(ValueError, match="candidates are"):
            fn(model, PERIOD, [], Q, R[:1])
        with pytest.raises(ValueError, match="candidates a call"):
            fn(model, PERIOD, [], Q[:0], R[:0])
