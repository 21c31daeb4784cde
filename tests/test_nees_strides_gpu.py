"""GPU: `mht_nees_nodes` where its grid strides.  nees_kernel launches at most 2048 workgroups of 256 lanes, one cell a lane, and
strides over the rest; the other GPU tests of the seam end at 7 800 cells, inside the first trip.  N1 is nees_ref.cell_batch(N, 1030,
510, seed 5), 525 300 cells (tests/nees_stride_util.py): trip 2 is row 509 from track 18 on, 1 012 cells, with the batch's four special
cells -- a pivot that is not positive, an absent cell, a NaN in x and one in P -- planted there once more.

The criterion is tests/test_nees_gpu.py's, unchanged: e_dev <= 8 max(e_np, eps64) per family against the np.longdouble evaluation, the
NaN cells the truth's exactly, the output preset to a sentinel with none left, `error` the float64 reference's bit for bit.  Every
test prints the device's ratios and the references' time; profiles/mc_stride_shapes.txt records them."""
import time

import numpy as np
import pytest

import nees_ref as ref
import nees_stride_util as u
from test_encounter_strides_gpu import seam_time
from test_nees_cpu import check_special_cells
from test_nees_gpu import SENTINEL, _hold, _raw

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("N", [6, 4])
def test_n1_525300_cells_the_kernel_strides(ctxs, N):
    """N1, (N, D) = (6, 6) on the six-state build and (4, 4) on the four-state build: every cell to the truth, the special cells of rows
    0 .. 3 and the ones planted in trip 2, at least 400 cells of trip 2 present and finite in the truth"""
    assert np.finfo(np.longdouble).eps < 1e-18
    label = "N1 N %d D %d, 1030 tracks of 510 nodes, %d-state build" % (N, N, N)
    t = time.perf_counter()
    x, P, truth, present = u.batch(N)
    t, made = time.perf_counter(), time.perf_counter() - t
    f64, want = ref.nees_batch(x, P, truth, present, N, np.float64), ref.nees_batch(x, P, truth, present, N, np.longdouble)
    print("%s: batch %.1f s, references %.1f s" % (label, made, time.perf_counter() - t))
    assert int(np.isfinite(u.second_trip(want["nees"])).sum()) >= 400
    with seam_time(label, ctxs[N], "mht_nees_nodes"):
        rc, out = _raw(ctxs[N], N, N, x, P, truth, present)
    assert rc == 0 and out.shape == (u.L_MAX, N + 3, u.N_TRACKS) and not (out == SENTINEL).any()
    got = ref.seam_dict(out, N)
    _hold(label, [got], [want], [f64])
    check_special_cells(got, N, N)
    print("%s: %d cells of trip 2 are finite" % (label, u.check_planted_cells(got, N, N)))
    assert np.array_equal(got["error"], f64["error"], equal_nan=True)
