"""The batch of tests/test_nees_strides_gpu.py and tests/test_nees_strides_cpu.py: nees_ref.cell_batch(N, 1030, 510, seed 5), 525 300
cells.  nees_kernel numbers the cells k * n + t and launches at most 2048 workgroups of 256 lanes, 524 288 cells a trip: its second
trip is row 509 from track 18 on, 1 012 cells.  The four special cells of cell_batch lie in row 0 .. 3; they are planted once more in
row 509, at tracks that are no multiples of 3 (those end two rows early, as cell_batch makes them)."""
import numpy as np

import nees_ref as ref

N_TRACKS, L_MAX, SEED = 1030, 510, 5
TRIP = 2048 * 256
ROW = L_MAX - 1
FIRST_TRACK = TRIP - ROW * N_TRACKS      # 18: the first cell of trip 2 is (509, 18)
BAD_PIVOT, ABSENT, NAN_X, NAN_P = (ROW, 20), (ROW, 22), (ROW, 23), (ROW, 25)

_cache = {}


def batch(N):
    """(x [L_max, N, n], P [L_max, NS, n], truth [L_max, N, n], present [L_max, n]) with the four cells planted, computed once per N"""
    if N not in _cache:
        x, P, truth, present = ref.cell_batch(N, N_TRACKS, L_MAX, SEED)
        iu = np.triu_indices(N)
        at = {(int(i), int(j)): s for s, (i, j) in enumerate(zip(*iu))}
        k, t = BAD_PIVOT
        Pm = np.zeros((N, N))
        Pm[iu] = P[k, :, t]
        U = np.linalg.cholesky(Pm + np.triu(Pm, 1).T).T
        P[k, at[(2, 2)], t] = U[0, 2] ** 2 + U[1, 2] ** 2 - 1.0      # the pivot of component 2 is -1; components 0 and 1 stay fine
        present[BAD_PIVOT], present[ABSENT], present[NAN_X], present[NAN_P] = 1, 0, 1, 1
        x[NAN_X[0], N - 1, NAN_X[1]] = np.nan
        P[NAN_P[0], N * (N + 1) // 2 - 1, NAN_P[1]] = np.nan
        _cache[N] = (x, P, truth, present)
    return _cache[N]


def second_trip(a):
    """The cells of trip 2 of a per-cell array [L_max, n, ...]"""
    return a[ROW, FIRST_TRACK:]


def check_planted_cells(got, N, D):
    """test_nees_cpu.check_special_cells' conditions on the cells planted in trip 2"""
    b = BAD_PIVOT
    assert np.isfinite(got["error"][b][:D]).all() and np.isnan(got["error"][b][D:]).all()
    assert np.isfinite(got["nees2"][b]) and got["nees2"][b] > 0 and np.isnan(got["nees4"][b]) and np.isnan(got["nees"][b])
    for cell in (ABSENT, NAN_X, NAN_P):
        assert all(np.isnan(got[k][cell]).all() for k in ref.NAMES), cell
    live = int(np.isfinite(second_trip(got["nees"])).sum())
    assert D < N or live >= 400, live
    return live
