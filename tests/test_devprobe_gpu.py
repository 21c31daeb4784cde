"""GPU: the helpers under both per-scan launches, one at a time, through the test-only probe library (tests/devprobe/probe.hip,
built by tests/devprobe_util.py with the library's flags): csrc/mht_wave.h against plain NumPy, csrc/mht_uf.h against a host
union-find and the oracle's find_clusters, csrc/mht_vtab.h against a Python dict keyed by (kind, value bits, P_d bits).  A failure
here names the primitive; the whole-scan tests say only that a scan differs.

Wavefront helpers: every wavefront works on its own 64 inputs, every lane active (the header's contract; partial wavefronts are out
of scope), every lane's result is read; blocks of 64 and of 256 threads; each probe runs twice and must answer bit for bit the same.
The 64 one-hot inputs of each helper pin its whole 64 x 64 lane-dependency matrix.  NaN VALUES with a valid index in the
(value, index) minima are outside the contract -- no caller passes them -- and are left out."""
import numpy as np
import pytest

import devprobe_util as U
import mht_oracle

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (pymht_amd has no CPU fallback)")
    return {nx: U.build(tmp_path_factory.mktemp("devprobe%d" % nx), nx) for nx in (4, 6)}


@pytest.fixture(scope="module")
def lib(libs):
    return libs[4]      # (mht_wave.h and mht_uf.h do not depend on the state dimension)


_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).to("cuda")


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def pad4(x):
    """whole blocks of 256: the number of rows (wavefronts) a multiple of four, the padding repeats the last row"""
    r = (-len(x)) % 4
    return np.concatenate([x, np.repeat(x[-1:], r, axis=0)]) if r else x


def run_wave(lib, name, x, width=64):
    """probe_<name> on the rows of x (one wavefront each) with 64- and 256-thread blocks, twice each: the output, the same shape"""
    import torch
    x = pad4(np.ascontiguousarray(x))
    n = x.shape[0] * 64
    assert x.shape[1] == width and x.shape[0] <= 512
    d_in, outs = dev(x.reshape(-1)), []
    for block in (64, 256, 64, 256):
        d_out = torch.full_like(d_in, 0x5a)
        rc = getattr(lib, "probe_" + name)(block, n, d_in.data_ptr(), d_out.data_ptr())
        assert rc == 0, (name, block, rc)
        outs.append(host(d_out, x.dtype).reshape(x.shape))
    for o in outs[1:]:
        assert o.tobytes() == outs[0].tobytes(), name + ": two calls / two block sizes differ"
    return x, outs[0]


def run_pair(lib, name, v, i):
    import torch
    v, i = pad4(np.ascontiguousarray(v, dtype=np.float64)), pad4(np.ascontiguousarray(i, dtype=np.int32))
    n = v.size
    d_v, d_i, outs = dev(v.reshape(-1)), dev(i.reshape(-1)), []
    for block in (64, 256, 64, 256):
        o_v, o_i = torch.full_like(d_v, -7.0), torch.full_like(d_i, -7)
        rc = getattr(lib, "probe_" + name)(block, n, d_v.data_ptr(), d_i.data_ptr(), o_v.data_ptr(), o_i.data_ptr())
        assert rc == 0, (name, block, rc)
        outs.append((host(o_v, np.float64).reshape(v.shape), host(o_i, np.int32).reshape(i.shape)))
    for o in outs[1:]:
        assert o[0].tobytes() == outs[0][0].tobytes() and o[1].tobytes() == outs[0][1].tobytes(), name + ": two calls / two block sizes differ"
    return v, i, outs[0][0], outs[0][1]


def every_lane(out):
    """'in every lane': the 64 lanes of a row hold the same bits"""
    assert (out.view(np.uint8).reshape(out.shape[0], 64, -1) == out.view(np.uint8).reshape(out.shape[0], 64, -1)[:, 63:64]).all(), "the lanes of a wavefront disagree"
    return out[:, 63]


# ---- A. mht_wave.h -----------------------------------------------------------------------------------------------------------------
def test_wave_scan_u32(lib):
    rng = np.random.default_rng(1)
    x = np.concatenate([np.eye(64, dtype=np.uint32), rng.integers(0, 2 ** 32, (64, 64), dtype=np.uint64).astype(np.uint32),
                        np.full((1, 64), 0xffffffff, dtype=np.uint32), np.ones((1, 64), dtype=np.uint32), np.zeros((1, 64), dtype=np.uint32),
                        rng.integers(0, 40, (32, 64)).astype(np.uint32)])
    x, out = run_wave(lib, "scan_u32", x)
    ref = (np.cumsum(x.astype(np.uint64), axis=1) & np.uint64(0xffffffff)).astype(np.uint32)
    assert (out == ref).all(), "rows %s" % np.flatnonzero((out != ref).any(axis=1))[:8]


def test_wave_scan_two_halves(lib):
    """the grow launch's idiom for a chunk of up to 128 leaves: scan(m1) + readlane(scan(m0), 63)"""
    rng = np.random.default_rng(2)
    x = np.concatenate([np.eye(128, dtype=np.uint32), rng.integers(0, 2 ** 32, (32, 128), dtype=np.uint64).astype(np.uint32),
                        np.full((1, 128), 0xffffffff, dtype=np.uint32), np.ones((1, 128), dtype=np.uint32), rng.integers(0, 70, (62, 128)).astype(np.uint32)])
    x, out = run_wave(lib, "scan_halves", x, width=128)
    ref = (np.cumsum(x.astype(np.uint64), axis=1) & np.uint64(0xffffffff)).astype(np.uint32)
    assert (out == ref).all(), "rows %s" % np.flatnonzero((out != ref).any(axis=1))[:8]


def test_wave_sum_i32(lib):
    rng = np.random.default_rng(3)
    x = np.concatenate([np.eye(64, dtype=np.int32), -np.eye(64, dtype=np.int32), rng.integers(I32_MIN, I32_MAX + 1, (64, 64)).astype(np.int32),
                        rng.integers(-1000, 1000, (32, 64)).astype(np.int32), np.full((1, 64), I32_MIN, dtype=np.int32), np.full((1, 64), -1, dtype=np.int32)])
    x, out = run_wave(lib, "sum_i32", x)
    _, scan = run_wave(lib, "scan_u32", x.view(np.uint32))
    got = every_lane(out)
    assert (got == scan[:, 63].view(np.int32)).all()
    assert (got == (x.astype(np.int64).sum(axis=1) & 0xffffffff).astype(np.uint32).view(np.int32)).all()


def _minmax_inputs(rng, neutral, mark):
    onehot = np.full((64, 64), neutral, dtype=np.int64)
    onehot[np.arange(64), np.arange(64)] = mark
    return np.concatenate([onehot, rng.integers(I32_MIN, I32_MAX + 1, (64, 64)), rng.integers(-50, 50, (32, 64)), -rng.integers(1, 2 ** 31, (16, 64)),
                           np.full((1, 64), I32_MIN), np.full((1, 64), I32_MAX), np.full((1, 64), -3), np.where(np.arange(64) == 40, I32_MIN, I32_MAX)[None],
                           np.where(np.arange(64) == 17, I32_MAX, I32_MIN)[None]]).astype(np.int32)


def test_wave_min_i32(lib):
    x, out = run_wave(lib, "min_i32", _minmax_inputs(np.random.default_rng(4), I32_MAX, -5))
    assert (every_lane(out) == x.min(axis=1)).all()
    x, out = run_wave(lib, "min_i32", _minmax_inputs(np.random.default_rng(40), 1000, 999))      # (the smallest possible margin)
    assert (every_lane(out) == x.min(axis=1)).all()


def test_wave_max_i32(lib):
    x, out = run_wave(lib, "max_i32", _minmax_inputs(np.random.default_rng(5), I32_MIN, 5))
    assert (every_lane(out) == x.max(axis=1)).all()
    x, out = run_wave(lib, "max_i32", _minmax_inputs(np.random.default_rng(50), -1000, -999))
    assert (every_lane(out) == x.max(axis=1)).all()


def test_wave_box_reduction(lib):
    """min, max, min, max back to back, as the grow launch reduces a target's bounding box (the sortable-float words of its four sides)"""
    import torch
    rng = np.random.default_rng(6)
    W = 132
    x = np.stack([_minmax_inputs(rng, I32_MAX, -9)[:W], _minmax_inputs(rng, I32_MIN, 9)[:W], _minmax_inputs(rng, 7, 6)[:W], _minmax_inputs(rng, -7, -6)[:W]])
    assert x.shape == (4, W, 64)
    n = W * 64
    d_in, outs = dev(x.reshape(-1)), []
    for block in (64, 256, 64, 256):
        d_out = torch.full_like(d_in, 0x5a)
        assert lib.probe_box_i32(block, n, d_in.data_ptr(), d_out.data_ptr()) == 0
        outs.append(host(d_out, np.int32).reshape(x.shape))
    for o in outs[1:]:
        assert (o == outs[0]).all()
    for k, ref in enumerate((x[0].min(axis=1), x[1].max(axis=1), x[2].min(axis=1), x[3].max(axis=1))):
        assert (every_lane(outs[0][k]) == ref).all(), k


def test_wave_sum_f64_order_and_error(lib):
    """wave_sum IS the balanced pairwise tree over the lanes -- bit for bit, -0.0 included -- and so within 6 * 2^-53 * sum|v| of math.fsum"""
    x, out = run_wave(lib, "sum_f64", U.sum_inputs())
    got = every_lane(out)
    tree = U.pairwise_tree(x)
    assert np.isfinite(tree).all()
    bad = np.flatnonzero(got.view(np.uint64) != tree.view(np.uint64))
    assert bad.size == 0, "rows %s: device %s, tree %s" % (bad[:8], got[bad[:8]], tree[bad[:8]])
    exact, mag = U.fsum_rows(x)
    ok = mag > 0
    print("wave_sum: worst |error| = %.2f * 2^-53 * sum|v| over %d rows" % (np.max(np.abs(got - exact)[ok] / mag[ok]) / 2.0 ** -53, len(x)))
    assert (np.abs(got - exact) <= U.FSUM_BOUND * mag).all()


def test_wave_sum_f64_nonfinite(lib):
    rng = np.random.default_rng(7)
    x = rng.standard_normal((8 + 64, 64))
    x[0, 11] = np.inf
    x[1, 63] = -np.inf
    x[2, 0], x[2, 63] = np.inf, -np.inf      # -> NaN
    x[3, 30] = np.nan
    x[4, 15], x[4, 16] = np.inf, np.inf
    x[5, 47] = np.nan
    x[5, 48] = np.inf
    x[6] = 1e308                              # overflows to +inf on the way
    x[7] = -1e308
    x[8 + np.arange(64), np.arange(64)] = np.nan      # one NaN, at every lane
    x, out = run_wave(lib, "sum_f64", x)
    got, tree = out[:, 63], U.pairwise_tree(x)
    assert (np.isnan(out) == np.isnan(tree)[:, None]).all()
    fin = ~np.isnan(tree)
    assert (out[fin].view(np.uint64) == tree[fin].view(np.uint64)[:, None]).all()
    assert np.isnan(got[2]) and np.isnan(got[3]) and got[0] == np.inf and got[1] == -np.inf and got[6] == np.inf and got[7] == -np.inf and np.isnan(got[8:72]).all()


def _min_value_inputs():
    rng = np.random.default_rng(8)
    onehot = np.full((64, 64), 1e300)
    onehot[np.arange(64), np.arange(64)] = -1e300
    close = np.full((64, 64), 1.0)
    close[np.arange(64), np.arange(64)] = np.nextafter(1.0, 0.0)      # one ulp below
    x = rng.standard_normal((24, 64)) * 10.0 ** rng.uniform(-8, 8, (24, 64))
    x[0] = np.inf                                   # the ILP launch's call on a row without a candidate
    x[1] = np.nan
    x[2, :] = np.nan
    x[2, 9] = 4.0                                   # one number among NaNs
    x[3, 20] = np.nan                               # one NaN among numbers
    x[4] = 0.0
    x[4, 33] = -0.0
    x[5] = -0.0
    x[5, 2] = 0.0
    x[6] = np.inf
    x[6, 63] = -np.inf
    x[7, ::2] = np.nan
    x[8] = np.inf
    x[8, 0] = 1e308
    x[9, 16:32] = np.nan                            # a whole row of 16 NaN
    x[10, :] = np.inf
    x[10, 48:] = np.nan
    return np.concatenate([onehot, close, x])


def _same_value(got, ref):
    """equal by value (+0.0 == -0.0), NaN where and only where the reference has one"""
    assert (np.isnan(got) == np.isnan(ref)).all(), "NaN where the reference has a number, or the other way round"
    ok = ~np.isnan(ref)
    assert (got[ok] == ref[ok]).all()


def test_wave_min_value(lib):
    """np.fmin.reduce: a NaN loses to a number, all NaN gives NaN, all +inf gives +inf"""
    x, out = run_wave(lib, "min_value", _min_value_inputs())
    got = every_lane(out)
    _same_value(got, np.fmin.reduce(x, axis=1))
    assert got[128] == np.inf and np.isnan(got[129]) and got[130] == 4.0 and got[132] == 0.0 and got[133] == 0.0 and got[134] == -np.inf


def test_row16_min_value(lib):
    """the same per row of 16 lanes, read from lanes 15, 31, 47, 63 only"""
    x, out = run_wave(lib, "row16_min_value", _min_value_inputs())
    _same_value(out[:, 15::16], np.fmin.reduce(x.reshape(-1, 4, 16), axis=2))


def _pair_inputs():
    rng = np.random.default_rng(9)
    vs, ix = [], []
    # one valid lane among 63 invalid ones that hold smaller values, at each of the 64 positions
    v = np.full((64, 64), -1e9)
    i = np.full((64, 64), -1)
    v[np.arange(64), np.arange(64)] = rng.standard_normal(64)
    i[np.arange(64), np.arange(64)] = rng.integers(0, I32_MAX, 64)
    vs.append(v), ix.append(i)
    # every lane valid, the smallest value at each of the 64 positions, by one ulp; arbitrary indices
    v = np.full((64, 64), 1.0)
    v[np.arange(64), np.arange(64)] = np.nextafter(1.0, 0.0)
    vs.append(v), ix.append(rng.integers(0, I32_MAX, (64, 64)))
    # all values equal: the smallest index, at each of the 64 positions
    i = rng.integers(1000, I32_MAX, (64, 64))
    i[np.arange(64), np.arange(64)] = rng.integers(0, 1000, 64)
    vs.append(np.full((64, 64), 2.5)), ix.append(i)
    # random, a quarter of the lanes invalid
    vs.append(rng.standard_normal((32, 64)) * 10.0 ** rng.uniform(-8, 8, (32, 64)))
    ix.append(np.where(rng.random((32, 64)) < 0.25, -1, rng.integers(0, I32_MAX, (32, 64))))
    # values from a set of three: ties everywhere, some lanes invalid, indices with duplicates
    vs.append(rng.choice([1.0, 2.0, 3.0], (32, 64)))
    ix.append(np.where(rng.random((32, 64)) < 0.3, -1, rng.integers(0, 40, (32, 64))))
    # valid lanes holding +inf: all of them / next to numbers / next to invalid lanes with numbers
    v = np.full((8, 64), np.inf)
    i = rng.integers(0, I32_MAX, (8, 64))
    v[1, 5] = 7.0
    i[2, ::2] = -1
    v[2, ::2] = -3.0
    i[3, :63] = -1
    v[4, 40] = -np.inf
    i[5] = np.arange(64)[::-1]
    i[6] = 0
    i[7, 16:] = -1
    vs.append(v), ix.append(i)
    # nobody valid
    vs.append(rng.standard_normal((2, 64))), ix.append(np.full((2, 64), -1))
    # one row of 16 without a valid lane
    v = rng.standard_normal((4, 64))
    i = rng.integers(0, I32_MAX, (4, 64))
    for r in range(4):
        i[r, 16 * r:16 * r + 16] = -1
        v[r, 16 * r:16 * r + 16] = -50.0
    vs.append(v), ix.append(i)
    return np.concatenate(vs), np.concatenate(ix).astype(np.int32)


def _pair_ref(v, i):
    """lexicographic minimum of (value, index) over the entries with index >= 0 along the last axis; (nan, -1) without one"""
    rv, ri = np.full(v.shape[:-1], np.nan), np.full(v.shape[:-1], -1, dtype=np.int32)
    for k in np.ndindex(v.shape[:-1]):
        c = sorted((float(a), int(b)) for a, b in zip(v[k], i[k]) if b >= 0)
        if c:
            rv[k], ri[k] = c[0]
    return rv, ri


def test_wave_min_pair(lib):
    v, i, ov, oi = run_pair(lib, "min_pair", *_pair_inputs())
    assert not np.isnan(v).any()
    rv, ri = _pair_ref(v, i)
    gi, gv = every_lane(oi), every_lane(ov)
    assert (gi == ri).all(), "rows %s" % np.flatnonzero(gi != ri)[:8]
    some = ri >= 0
    assert (gv[some] == rv[some]).all()
    assert (~some).sum() >= 2


def test_row16_min_pair(lib):
    v, i, ov, oi = run_pair(lib, "row16_min_pair", *_pair_inputs())
    rv, ri = _pair_ref(v.reshape(-1, 4, 16), i.reshape(-1, 4, 16))
    gi, gv = oi[:, 15::16], ov[:, 15::16]
    assert (gi == ri).all(), "rows %s" % np.flatnonzero((gi != ri).any(axis=1))[:8]
    some = ri >= 0
    assert (gv[some] == rv[some]).all()
    assert (~some).sum() >= 12


# ---- B. mht_uf.h -------------------------------------------------------------------------------------------------------------------
def _link(lib, d_parent, T, epoch, ex, ey):
    d_x, d_y = dev(ex if len(ex) else np.zeros(1, np.int32)), dev(ey if len(ey) else np.zeros(1, np.int32))
    rc = lib.probe_uf_link(d_parent.data_ptr(), T, epoch, d_x.data_ptr(), d_y.data_ptr(), len(ex))
    assert rc == 0, rc
    return host(d_parent, np.uint64)


@pytest.mark.parametrize("name", sorted(U.link_graphs()))
def test_uf_link(lib, name):
    """one edge per lane: afterwards every walk ends at the smallest member of its component, every other member holds a parent word of
    this epoch naming a smaller index, the smallest holds none"""
    import torch
    T, ex, ey = U.link_graphs()[name]
    d_parent = torch.zeros(T, dtype=torch.int64, device="cuda")
    U.check_forest(_link(lib, d_parent, T, 5, ex, ey), 5, U.host_uf(T, ex, ey))


def test_uf_link_epochs_on_one_array(lib):
    """a parent array that is never cleared: words of epoch 3 with arbitrary low halves, then three graphs under epochs 6, 7 (the grow
    launch's `epoch | 1` redo) and 8 -- after each, the labels are that graph's alone"""
    rng = np.random.default_rng(12)
    T = 20000
    old = (np.uint64(3) << np.uint64(32)) | rng.integers(0, 2 ** 32, T, dtype=np.uint64)
    d_parent = dev(old)
    for epoch, T_, ex, ey in U.epoch_graphs():
        assert T_ == T
        words = _link(lib, d_parent, T, epoch, ex, ey)
        U.check_forest(words, epoch, U.host_uf(T, ex, ey))
        assert ((words >> np.uint64(32)) >= np.uint64(3)).all()      # (atomic max: no word goes back)


def _claim(lib, d_owner, d_parent, bits, AW, epoch, cap):
    import torch
    T = len(bits)
    d_assoc = dev(bits.reshape(-1))
    d_nconf = torch.full((T,), -9, dtype=torch.int32, device="cuda")
    rc = lib.probe_uf_claim(d_assoc.data_ptr(), T, AW, d_owner.data_ptr(), d_parent.data_ptr(), epoch, cap, d_nconf.data_ptr())
    assert rc == 0, rc
    return host(d_parent, np.uint64), host(d_nconf, np.int32)


@pytest.mark.parametrize("AW", U.CLAIM_AW)
def test_uf_claim(lib, AW):
    """a workgroup per target, shaped like the grow launch's: the last wavefront exchanges the owner words of the target's nodes
    (uf_claim, a conflict list of `cap` entries in LDS, the conflicts beyond it linked at once) and links the list behind a barrier.
    The components are the oracle's at every cap, 0 included; the NUMBER of conflicts a target sees depends on who came first and is
    only held to 0 <= nconf <= cap (and to 0 where no two targets share a node)."""
    import torch
    for name, sets in U.claim_scenes(AW).items():
        T, bits = len(sets), U.sets_as_bits(sets, AW)
        ref = U.labels_of_clusters(mht_oracle.find_clusters(sets), T)
        for cap in U.CLAIM_CAP:
            d_owner = torch.zeros(AW * 64, dtype=torch.int64, device="cuda")
            d_parent = torch.zeros(T, dtype=torch.int64, device="cuda")
            words, nconf = _claim(lib, d_owner, d_parent, bits, AW, 2, cap)
            assert ((nconf >= 0) & (nconf <= cap)).all(), (name, cap, nconf.min(), nconf.max())
            if name == "disjoint":
                assert (nconf == 0).all()
            try:
                U.check_forest(words, 2, ref)
            except AssertionError as e:
                raise AssertionError("AW %d, %s, cap %d: %s" % (AW, name, cap, e))
            owner = host(d_owner, np.uint64)
            used = np.zeros(AW * 64, dtype=bool)
            used[[m for s in sets for m in s]] = True
            assert ((owner >> np.uint64(32)) == np.where(used, 2, 0).astype(np.uint64)).all(), "owner words: exactly the nodes in use carry this epoch"


@pytest.mark.parametrize("AW", [1, 65])
def test_uf_claim_two_scans_on_the_same_arrays(lib, AW):
    """owner and parent words are never cleared: a scan under epoch 2, then another scene under epoch 4 -- its labels are its own"""
    import torch
    sc = U.claim_scenes(AW)
    d_owner = torch.zeros(AW * 64, dtype=torch.int64, device="cuda")
    d_parent = torch.zeros(3000, dtype=torch.int64, device="cuda")
    for epoch, name in ((2, "one_shared_node"), (4, "sparse"), (6, "dense_rows")):
        sets = sc[name]
        words, nconf = _claim(lib, d_owner, d_parent, U.sets_as_bits(sets, AW), AW, epoch, 3)
        assert ((nconf >= 0) & (nconf <= 3)).all()
        U.check_forest(words, epoch, U.labels_of_clusters(mht_oracle.find_clusters(sets), len(sets)))


# ---- C. mht_vtab.h -----------------------------------------------------------------------------------------------------------------
SENT64 = np.uint64(0xa5a5a5a5a5a5a5a5)
GUARD = 256      # words behind Pv, pdv and Gk that nobody may touch


class Table:
    """A VTab in device arrays filled by the host, Pv / pdv / Gk preset to a sentinel and followed by guard regions"""

    def __init__(self, lib, vcap, n_slots):
        import torch
        self.lib, self.vcap, self.n_slots, self.pw = lib, vcap, n_slots, lib.VT_PW
        full = lambda n: dev(np.full(n, SENT64, dtype=np.uint64))
        self.Pv, self.pdv, self.Gk = full(vcap * self.pw + GUARD), full(vcap + GUARD), full(2 * vcap * lib.GKQ * 2 + GUARD)
        self.child = torch.full((2 * vcap,), -1, dtype=torch.int32, device="cuda")
        self.slots = torch.zeros(n_slots, dtype=torch.int64, device="cuda")
        self.count = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.overflow = torch.zeros(1, dtype=torch.int32, device="cuda")

    def _args(self):
        return [t.data_ptr() for t in (self.Pv, self.pdv, self.Gk, self.child, self.slots, self.count, self.overflow)] + [self.vcap, self.n_slots - 1]

    def insert(self, vals, req):
        import torch
        d = [dev(a.reshape(-1)) for a in (req, vals.kind, vals.words, vals.pd)]
        ids = torch.full((len(req),), -5, dtype=torch.int32, device="cuda")
        rc = self.lib.probe_vt_insert(*self._args(), len(req), d[0].data_ptr(), len(vals), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), ids.data_ptr())
        assert rc == 0, rc
        return host(ids, np.int32)

    def load(self, ids, kind):
        import torch
        d_ids, d_kind = dev(np.asarray(ids, dtype=np.int32)), dev(np.asarray(kind, dtype=np.int32))
        out = torch.zeros(len(ids) * 2 * self.pw, dtype=torch.int64, device="cuda")
        rc = self.lib.probe_vt_load(*self._args(), len(ids), d_ids.data_ptr(), d_kind.data_ptr(), out.data_ptr())
        assert rc == 0, rc
        return host(out, np.uint64).reshape(len(ids), 2 * self.pw)

    def read(self):
        self.h_Pv, self.h_pdv, self.h_Gk = host(self.Pv, np.uint64), host(self.pdv, np.uint64), host(self.Gk, np.uint64)
        self.h_slots, self.h_child = host(self.slots, np.uint64), host(self.child, np.int32)
        self.h_count, self.h_overflow = int(host(self.count, np.uint32)[0]), int(host(self.overflow, np.int32)[0])
        return self

    def guards_untouched(self):
        self.read()
        assert (self.h_Pv[self.vcap * self.pw:] == SENT64).all() and (self.h_pdv[self.vcap:] == SENT64).all(), "a store behind the end of Pv / pdv"
        assert (self.h_Gk == SENT64).all() and (self.h_child == -1).all(), "find-or-insert does not touch the gains or the child table"

    def published(self):
        """(slot index, tag, id) of every slot in use; none may be pending"""
        self.read()
        at = np.flatnonzero(self.h_slots)
        low = (self.h_slots[at] & np.uint64(0xffffffff)).astype(np.int64)
        assert (low != U.VT_PENDING).all(), "a slot was left pending"
        assert (low >= 1).all()
        return at, (self.h_slots[at] >> np.uint64(32)).astype(np.int64), low - 1


def ids_by_value(vals, req, ids):
    """equal keys got equal ids and distinct keys distinct ids, in one launch: the id of every value of the list"""
    first = {}
    canon = np.array([first.setdefault(k, v) for v, k in enumerate(vals.keys())])
    assert (ids >= 0).all()
    idof = np.full(len(vals), -1, dtype=np.int64)
    idof[canon[req]] = ids
    assert (ids == idof[canon[req]]).all(), "one value, two ids"
    distinct = np.unique(canon)
    assert (idof[distinct] >= 0).all(), "a value of the list was never requested"
    assert len(np.unique(idof[distinct])) == len(distinct), "two values, one id"
    return idof[canon]


def check_table(tab, vals, idof):
    """everything the table holds, against the list of ALL values ever requested from it and their ids"""
    tab.guards_untouched()
    pw = tab.pw
    assert tab.h_overflow == 0
    assert tab.h_count == vals.n_ids(), "ids leaked or missing: count %d, the values take %d" % (tab.h_count, vals.n_ids())
    owned = np.concatenate([idof, idof[vals.kind == 1] + 1])
    assert len(set(zip(idof.tolist(), vals.kind.tolist()))) == len(set(vals.keys()))
    assert sorted(set(owned.tolist())) == list(range(tab.h_count)), "the ids are not exactly range(count)"
    assert len(set(owned.tolist())) == len(set(idof.tolist())) + len(set(idof[vals.kind == 1].tolist())), "a float64 value's second id belongs to somebody else"
    Pv = tab.h_Pv[:tab.vcap * pw].reshape(tab.vcap, pw)
    for kind in (0, 1):
        sel = np.flatnonzero(vals.kind == kind)
        if not len(sel):
            continue
        nw = pw * (kind + 1)
        stored = np.concatenate([Pv[idof[sel]], Pv[idof[sel] + 1]], axis=1)[:, :nw] if kind else Pv[idof[sel]]
        assert (stored == vals.words[sel, :nw]).all(), "Pv[id] is not the value"
        assert (tab.h_pdv[idof[sel]] == vals.pd[sel].view(np.uint64)).all(), "pdv[id] is not the value's P_d"
        got = tab.load(idof[sel], np.full(len(sel), kind))
        assert (got[:, :nw] == vals.words[sel, :nw]).all(), "vt_load%s reads something else back" % ("64" if kind else "")
    at, tag, sid = tab.published()
    by_id = {int(i): v for v, i in enumerate(idof)}
    assert sorted(sid.tolist()) == sorted(set(idof.tolist())), "the slots in use do not name every value's (first) id once"
    want = vals.tags()[[by_id[i] for i in sid.tolist()]]
    assert (tag == want).all(), "slots %s: the tag is not the hash of the value the slot names" % at[tag != want][:8]
    return at, tag, sid, by_id


@pytest.mark.parametrize("nx", [4, 6])
def test_vtab_concurrent_insert(libs, nx):
    """3 000 new float32 values, each asked for 60 times in shuffled order by 704 workgroups at once"""
    vals = U.random_f32_values(nx, 3000, 21)
    req = U.requests(3000, 60, 4)
    tab = Table(libs[nx], 3000, U.table_size(3000))
    ids = tab.insert(vals, req)
    idof = ids_by_value(vals, req, ids)
    check_table(tab, vals, idof)
    assert tab.h_count == 3000
    again = tab.insert(vals, req)
    assert (again == ids).all(), "a second launch of the same requests answers differently"
    check_table(tab, vals, idof)


@pytest.mark.parametrize("nx", [4, 6])
def test_vtab_what_makes_values_different(libs, nx):
    """one bit in the first word, one bit in the last word, the same P under two P_d, +0.0 against -0.0: different values.  One NaN bit
    pattern asked for twice: one value."""
    vals, distinct = U.near_values(nx)
    req = U.requests(len(vals), 200, 5)
    tab = Table(libs[nx], 16, U.table_size(16))
    idof = ids_by_value(vals, req, tab.insert(vals, req))
    check_table(tab, vals, idof)
    assert tab.h_count == distinct == len(set(idof.tolist())) and idof[6] == idof[7]


@pytest.mark.parametrize("nx", [4, 6])
def test_vtab_float64_kind_and_promotion(libs, nx):
    """float64 values in the same table and the same launch: two ids each; vt_promote(id32) is the id of the exactly converted value"""
    f32, f64 = U.random_f32_values(nx, 500, 31), U.random_f64_values(nx, 300, 32)
    vals = U.Values.concat(f32, f64)
    req = U.requests(len(vals), 20, 6)
    vcap = 500 + 2 * 300 + 2 * 200
    tab = Table(libs[nx], vcap, U.table_size(vcap))
    idof = ids_by_value(vals, req, tab.insert(vals, req))
    check_table(tab, vals, idof)
    assert tab.h_count == 1100
    # the float32 values 0..199 as float64: by promotion of their ids and by a direct request of the converted matrix
    P32 = f32.words[:200, :tab.pw].copy().view(np.float32)
    conv = U.Values(nx, np.ones(200), U.f64_words(P32.astype(np.float64)), f32.pd[:200])
    w = np.zeros((200, 2 * tab.pw), dtype=np.uint64)
    w[:, 0] = idof[:200].astype(np.uint64)
    prom = U.Values(nx, np.full(200, 2), w, f32.pd[:200])
    half = np.arange(200) < 100
    mix = lambda first: U.Values(nx, np.where(half == first, 2, 1), np.where((half == first)[:, None], prom.words, conv.words), conv.pd)
    r2 = U.requests(200, 8, 7)
    a = ids_by_value(mix(True), r2, tab.insert(mix(True), r2))       # 0..99 promoted, 100..199 asked for directly, in one launch
    b = ids_by_value(mix(False), r2, tab.insert(mix(False), r2))     # ... and the other way round
    assert (a == b).all(), "vt_promote and a direct request of the converted value disagree"
    everything = U.Values.concat(vals, conv)
    check_table(tab, everything, np.concatenate([idof, a]))
    assert tab.h_count == vcap


@pytest.mark.parametrize("nx", [4, 6])
def test_vtab_collisions_and_wrap_around(libs, nx):
    """64 slots, 40 values chosen with the restated hash (tests/devprobe_util.py::collision_values): two of them carry ONE tag and start
    at one slot -- told apart by their last word alone --, two more are one covariance under two P_d with ONE tag at one slot -- told
    apart by P_d alone --, and the chains of those that start in the last slots run over the end of the table"""
    vals, pairs = U.collision_values(nx)
    req = U.requests(len(vals), 60, 8)
    tab = Table(libs[nx], 64, U.COLLISION_SLOTS)
    ids = tab.insert(vals, req)
    idof = ids_by_value(vals, req, ids)
    at, tag, sid, by_id = check_table(tab, vals, idof)
    assert tab.h_count == 40
    where = {by_id[i]: (a, t) for a, t, i in zip(at.tolist(), tag.tolist(), sid.tolist())}
    for p, q in pairs:
        assert idof[p] != idof[q] and where[p][1] == where[q][1] and where[p][0] != where[q][0]
    wrapped = sum(1 for v, (a, _) in where.items() if a < (vals.hash(v)[1] & 63))
    print("values stored in front of their start slot (over the end of the table):", wrapped)
    assert wrapped >= 3
    assert (tab.insert(vals, req) == ids).all()
    check_table(tab, vals, idof)


@pytest.mark.parametrize("nx", [4, 6])
@pytest.mark.parametrize("kind", ["float32", "float64", "float64_at_odd_ids"])
def test_vtab_capacity(libs, nx, kind):
    """more values than ids (the documented MHT_E_CAPACITY path), vcap = 100 against 160 float32 values / 160 float64 values (two ids
    each) / the same behind ONE float32 value, so that the float64 values sit at odd ids and the last one would own ids 99 and 100:
    the sticky word goes up, every id handed out is below vcap, every slot in use names a stored value that was asked for, nothing is
    left pending, nothing is written behind the arrays -- and the launch ends"""
    vcap = 100
    vals = U.random_f32_values(nx, 160, 23) if kind == "float32" else U.random_f64_values(nx, 160, 24)
    tab = Table(libs[nx], vcap, U.table_size(vcap))
    if kind == "float64_at_odd_ids":
        one = U.random_f32_values(nx, 1, 25)
        assert (tab.insert(one, U.requests(1, 64, 1)) == 0).all()
        vals = U.Values.concat(vals, one)
    req = U.requests(160, 20, 9)
    ids = tab.insert(vals, req)
    tab.guards_untouched()
    assert tab.h_overflow == 1
    assert ((ids >= 0) & (ids < vcap)).all()
    at, tag, sid = tab.published()
    k64 = (tag >> 31) & 1
    assert len(at) >= vcap // 2 and (sid + k64 < vcap).all()
    if kind != "float32":
        assert ((sid[k64 == 1] & 1) == (kind == "float64_at_odd_ids")).all()
    pw = tab.pw
    Pv = tab.h_Pv[:vcap * pw].reshape(vcap, pw)
    keys = {k: v for v, k in enumerate(vals.keys())}
    tags = vals.tags()
    for a, t, i, k in zip(at.tolist(), tag.tolist(), sid.tolist(), k64.tolist()):
        stored = (k, (np.concatenate([Pv[i], Pv[i + 1]]) if k else Pv[i]).tobytes(), tab.h_pdv[i:i + 1].tobytes())
        assert stored in keys, "slot %d names id %d, which holds no value that was asked for" % (a, i)
        assert t == tags[keys[stored]]
