"""GPU: the device M-of-N initiator (csrc/mht_init_dev.h: initiator_body, launched by mht_initiator_step) against the live oracle
(oracle/m_of_n_oracle.py) past one wavefront, one workgroup and the LDS tables -- scan by scan through the raw ABI, with the `used` BIT mask
(tests/initiator_util.py): births, measurement numbers, float32 states and covariances, list sizes, all with np.array_equal.

What each stream reaches (asserted on the CPU by test_initiator_shapes_cpu.py, printed by the tests here):
  wide      M up to 2301 (36 words of `used`, a ragged last one), 2281 unused (three passes of 1024), 1464 preliminary tracks (two passes),
            V = n1 + n2 up to 3546 (gnn_core's third find loop), 332-356 births per scan, up to 646 initiators (eleven blocks of 64),
            13 assignment problems of up to 1203 edges with tables of 9-86 KB: all in global memory.
  dense     13 problems with tables of 3380-8550 bytes: 10 in LDS (16-bit indices), 3 in global memory (7606, 8212, 8550 > 7424);
            components of up to 26 nodes; up to 178 preliminary tracks, 18 births per scan.
  seeds     clutter only: up to 1380 initiators against 1383 leftovers (22 blocks of 64, V = 2751) with 2-3 edges; two gate problems
            with tracks and no edge (gnn_core's early return).
  edges     unused counts of exactly 0 (an empty first scan; an empty scan and an all-used scan while preliminary tracks exist), 1, 64,
            65, 1024, 1025; time steps of 1.0, 2.5 and 4.0 s; one merged birth; 8 problems in LDS, 3 in global memory, 4 without an edge.
  ais       8 scans with 0-40 messages: 88 start a track, 15 find their identity among the tracks, 6 are similar to an older track, 19 to
            one started by an earlier message of the scan, 41 are flagged used; one scan has messages and no unused radar measurement;
            two scans pass the flags as NULL.  4-state build only.
  capacity  M = max_meas + 1 is refused (MHT_E_INVALID) and the stream goes on matching; max_prelim = 64 and max_born = 4 on the dense
            stream report MHT_E_CAPACITY and stay within their tables.

Wall time on an MI355X host (the oracle's share is paid once per stream and process): see the figures the tests print."""
import time

import numpy as np
import pytest

import initiator_util as iu

pytestmark = pytest.mark.gpu
BUILDS = [4, 6]      # libmht_amd.so and the six-state build: the same initiator behind the same seam


def _run_case(name, nx):
    from pymht_amd.device import Context
    t0 = time.perf_counter()
    run = iu.oracle_run(name)
    t1 = time.perf_counter()
    ctx = Context(0, nx=nx)
    try:
        born = iu.run_device(ctx, run)
    finally:
        ctx.close()
    print("%s | %d-state build: %d births, oracle %.2f s, device and comparison %.2f s" % (iu.describe(run), nx, born, t1 - t0, time.perf_counter() - t1))
    return run, born


@pytest.mark.parametrize("nx", BUILDS)
def test_wide_scans_match_the_oracle(nx):
    run, born = _run_case("wide", nx)
    assert born > 1024


@pytest.mark.parametrize("nx", BUILDS)
def test_dense_scans_match_the_oracle_on_both_sides_of_the_lds_limit(nx):
    run, born = _run_case("dense", nx)
    assert born >= 40


@pytest.mark.parametrize("nx", BUILDS)
def test_clutter_scans_with_more_initiators_than_threads_match_the_oracle(nx):
    run, born = _run_case("seeds", nx)
    assert run["want"][-1]["n_prelim"] > 0


@pytest.mark.parametrize("nx", BUILDS)
def test_edge_scans_match_the_oracle(nx):
    run, born = _run_case("edges", nx)
    assert run["figures"]["n_merged"] >= 1 and born >= 10


def test_ais_messages_start_preliminary_tracks_like_the_oracle():
    run, born = _run_case("ais", 4)
    assert born >= 30


@pytest.mark.parametrize("nx", BUILDS)
def test_overflow_is_reported_and_stays_within_the_tables(nx):
    from pymht_amd import _lib
    from pymht_amd.device import Context
    run = iu.oracle_run("dense")
    cfg = run["cfg"]
    ctx = Context(0, nx=nx)
    try:
        # a scan of more than max_meas measurements is refused; the initiator goes on as if it had not been offered
        dev = iu.DeviceInitiator(ctx, cfg["M"], cfg["N"], cfg["max_meas"], cfg["max_prelim"], cfg["max_born"])
        try:
            for k, ((z, used, t), want) in enumerate(zip(run["scans"], run["want"])):
                if k == 3:
                    assert dev.step(np.zeros((cfg["max_meas"] + 1, 2), np.float32), None, t) == _lib.MHT_E_INVALID
                assert dev.step(z, used, t) == _lib.MHT_OK
                iu.compare_scan(dev.born(), want, ("capacity", k))
        finally:
            dev.close()
        # a full preliminary-track table, a full birth table: reported, and the counts stay within them
        for kw, col, cap in ((dict(max_prelim=64), 5, 64), (dict(max_born=4), 4, 4)):
            dev = iu.DeviceInitiator(ctx, cfg["M"], cfg["N"], **kw)
            try:
                codes, counts = [], []
                for z, used, t in run["scans"]:
                    assert dev.step(z, used, t) == _lib.MHT_OK
                    got = dev.born()
                    codes.append(got[0]); counts.append(got[col])
            finally:
                dev.close()
            print("capacity %s: codes %s, counts %s" % (kw, codes, counts))
            assert set(codes) <= {_lib.MHT_OK, _lib.MHT_E_CAPACITY} and _lib.MHT_E_CAPACITY in codes
            assert max(counts) <= cap
    finally:
        ctx.close()
