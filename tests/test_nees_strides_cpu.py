"""CPU: the batch of tests/test_nees_strides_gpu.py reaches nees_kernel's second trip, and the cells planted there are what they are
meant to be in the references.  The threshold is recomputed from the constants of csrc/mht_nees.hip, read as text."""
import numpy as np
import pytest

import nees_ref as ref
import nees_stride_util as u
from test_encounter_strides_cpu import ceil_div, constants


def test_n1_lies_behind_the_cap_and_its_planted_cells_are_in_trip_2():
    c = constants("mht_nees.hip")
    threads, cap = int(c["NEES_THREADS"]), int(c["NEES_MAX_BLOCKS"])
    cells = u.L_MAX * u.N_TRACKS
    assert (threads, cap, threads * cap) == (256, 2048, u.TRIP) and cells == 525300 > u.TRIP and ceil_div(cells - u.TRIP, threads) == 4
    assert u.TRIP // u.N_TRACKS == u.ROW == 509 and u.TRIP % u.N_TRACKS == u.FIRST_TRACK == 18
    for k, t in (u.BAD_PIVOT, u.ABSENT, u.NAN_X, u.NAN_P):
        assert k * u.N_TRACKS + t >= u.TRIP and t % 3 != 0
    assert 130 * 60 < u.TRIP      # (the largest batch of the older tests)


@pytest.mark.parametrize("N", [4, 6])
def test_the_planted_cells_in_the_float64_reference(N):
    x, P, truth, present = u.batch(N)
    got = ref.nees_batch(x, P, truth, present, N, np.float64)
    live = u.check_planted_cells(got, N, N)
    print("N1, %d states: %d cells of trip 2 are finite in the float64 reference" % (N, live))
    assert present[u.ROW, u.FIRST_TRACK:].sum() >= 400
