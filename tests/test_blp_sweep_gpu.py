"""GPU: the 0-1 ILP solver (csrc/mht_blp.hip through mht_solve_blp) against exact optima ON its dispatch thresholds.

tests/golden/g24_ilp_sweep.npz (oracle/gen_ilp_sweep.py; checked by tests/test_blp_sweep_cpu.py) holds synthetic clusters at every
K / nH / nR / PD where the solver changes its path -- K 1 2 3 4 5 | 8 9 10 11 12 (pair rounds, straight to branch and bound, fused
wavefront forms, exact enumeration), 511 / 512 / 513 columns (the column copy's wrap, ENUM_WIDE), K 23 24 25 (teams), 63 64 65
(prefetch), (K, nH) = (256, 2048) (256, 2049) (257, 2056) and nR = 1022 .. 1025 (the LDS tier), PD 8 9 15 -- with the HiGHS optimum, its
uniqueness and the LP relaxation's value.  Every structure comes with grid costs (multiples of 2^-10: every partial sum is exact, the
objective has to match BIT FOR BIT; on ties the selection has to be feasible) and with continuous costs (objective within
1e-9 * max(1, |obj|), the bound of the recorded-instance tests; the selection equal wherever the optimum is unique).  Both builds
(libmht_amd.so, libmht_amd6.so) compile the solver, both are run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from blp_sweep_util import FAMILIES, SWEEP, check_feasible, load_sweep
from pymht_amd import _lib
from test_cluster_blp_gpu import gpu_blp, load_instances

pytestmark = pytest.mark.gpu

CERTIFIED, BRANCHED = 1, 2      # include/mht_amd.h: MHT_BLP_CERTIFIED, MHT_BLP_BRANCHED (3 = MHT_BLP_NODE_LIMIT never shows)


@pytest.fixture(scope="module")
def sweep(gold_dir):
    """The instances as load_instances reads them, with the generator's tags; read once, never written to."""
    insts = load_instances(os.path.join(gold_dir, SWEEP))
    tagged = load_sweep(gold_dir)
    assert len(insts) == len(tagged)
    out = []
    for a, b in zip(insts, tagged):
        assert a["obj"] == b["obj"] and np.array_equal(a["sel"], b["sel"])
        out.append(dict(b, **a))
    return out


@pytest.fixture(scope="module")
def ctx_of(gpu_ctx):
    from pymht_amd.device import Context
    c6 = Context(0, nx=6)
    yield {4: gpu_ctx, 6: c6}
    c6.close()


def solve(ctx, inst, where, **kw):
    """gpu_blp + check; an error of the call (MHT_E_LIMIT: the node limit) names the instance."""
    try:
        got = gpu_blp(ctx, inst, **kw)
    except _lib.MhtError as e:
        pytest.fail("%s: instance %d (%s %s, K=%d nH=%d nR=%d PD=%d): %s" % (
            where, inst["index"], inst["family"], inst["variant"], inst["K"], inst["nH"], inst["nR"], inst["PD"], e))
    check(inst, got, where)
    return got


def check(inst, got, where=""):
    sel, obj, st, it, nd = got
    tag = (where, inst["index"], inst["family"], inst["variant"], inst["K"], inst["nH"], inst["nR"], inst["PD"], st, it, nd, obj, inst["obj"])
    assert st in (CERTIFIED, BRANCHED), tag
    check_feasible(inst, sel)
    assert obj == float(np.sum(inst["cost"][sel])) or inst["variant"] == "cont", tag      # (the reported value is the selection's)
    if inst["variant"] == "grid":
        assert obj == inst["obj"], tag
    else:
        assert abs(obj - inst["obj"]) <= 1e-9 * max(1.0, abs(obj)), tag
    if inst["unique"]:
        assert sel == inst["sel"].tolist(), tag


@pytest.mark.parametrize("nx", [4, 6])
@pytest.mark.parametrize("family", FAMILIES)
def test_sweep_default_switches(ctx_of, sweep, family, nx):
    """Every instance with the switches as shipped.  Where the LP relaxation is not tight (obj - lp > 1e-6) no dual certificate exists:
    the status has to be BRANCHED -- except for two targets, whose pair enumeration reports CERTIFIED."""
    mine = [i for i in sweep if i["family"] == family]
    assert mine
    n_gap, stats, max_nodes = 0, {CERTIFIED: 0, BRANCHED: 0}, 0
    for inst in mine:
        got = solve(ctx_of[nx], inst, "default")
        st, nd = got[2], got[4]
        stats[st] += 1
        max_nodes = max(max_nodes, nd)
        if inst["gap"]:
            n_gap += 1
            assert st == BRANCHED or inst["K"] == 2, (inst["index"], inst["K"], inst["nH"], st, got[3], nd, inst["obj"] - inst["lp"])
    print("sweep %-8s nx=%d: %d instances, %d with an LP gap, %d certified, %d branched, most nodes %d" % (
        family, nx, len(mine), n_gap, stats[CERTIFIED], stats[BRANCHED], max_nodes))


@pytest.mark.parametrize("nx", [4, 6])
def test_sweep_without_dual_phase(ctx_of, sweep, nx):
    """max_iter = 0: no coordinate round at all, the search has to prove optimality on its own (every third instance)."""
    for inst in sweep[::3]:
        solve(ctx_of[nx], inst, "max_iter=0", max_iter=0)


@pytest.mark.parametrize("nx", [4, 6])
@pytest.mark.parametrize("switch", ["MHT_BLP_FORCE_HBM", "MHT_BLP_NO_ENUM", "MHT_BLP_NO_TEAMS", "MHT_BLP_NO_REDUCE"])
def test_sweep_environment_switches(ctx_of, sweep, monkeypatch, switch, nx):
    """Each switch of the seam (read per call) on the small-K and middle-K families: everything on HBM scratch, branch and bound in place
    of the enumeration, one workgroup in place of a team, no reduced-cost fixing -- the last one on the tier-edge family as well."""
    monkeypatch.setenv(switch, "1")
    families = ("small", "middle", "tier") if switch == "MHT_BLP_NO_REDUCE" else ("small", "middle")
    for inst in sweep:
        if inst["family"] in families:
            solve(ctx_of[nx], inst, switch)


@pytest.mark.parametrize("nx", [4, 6])
def test_sweep_second_call_gives_the_same_selection(ctx_of, sweep, nx):
    """A second call on the same context holds to the reference like the first and -- where the optimum is unique -- returns the same
    selection (the members of a team race on one incumbent; the scratch of the first call is the second one's)."""
    for inst in sweep:
        if inst["K"] < 24 and inst["index"] % 4 >= 2:      # (below the team size: every other structure)
            continue
        a = solve(ctx_of[nx], inst, "first call")
        b = solve(ctx_of[nx], inst, "second call")
        if inst["unique"]:
            assert a[0] == b[0], inst["index"]


# ---- row numbering at the top of the accepted range ----------------------------------------------------------------------------------
def blp_lds_bytes(n_rows):
    """Dynamic LDS of the seam's launch for `n_rows` measurement rows: csrc/mht_blp.hip, blp_lds_bytes(cap_h, cap_r, cap_k, cap_uw) at the
    default tier (BIG_MAXH = 2048 columns, BIG_MAXR = 1024 rows, BIG_MAXK = 256 targets; 256 threads: RED_SLOT = 512, ENUM_LDS = 768) with
    cap_uw = the 64-bit words of the row bitset, rounded up to an even count after adding one (blp_set_tier):
        cap_uw * 8 + RED_SLOT + cap_uw * 4 + 16 + cap_h * 16 + cap_h * 8 * 2 + cap_r * 8 + 7 * (cap_k + 4) * 8
        + 2 * cap_r * 4 + 6 * (cap_k + 4) * 4 + cap_h * 2 * 2 + ENUM_LDS + cap_h * 16 + cap_h * 4"""
    cap_h, cap_r, kpad, red_slot, enum_lds = 2048, 1024, 256 + 4, 512, 768
    cap_uw = (((n_rows + 63) // 64) + 1) & ~1
    return (cap_uw * 8 + red_slot + cap_uw * 4 + 16 + cap_h * 16 + cap_h * 8 * 2 + cap_r * 8 + 7 * kpad * 8
            + 2 * cap_r * 4 + 6 * kpad * 4 + cap_h * 2 * 2 + enum_lds + cap_h * 16 + cap_h * 4)


LDS_LIMIT = 158 * 1024      # launch_blp refuses more


def largest_accepted_rows():
    n = 64
    while blp_lds_bytes(n + 64) <= LDS_LIMIT:
        n += 64
    return n


def raw_blp(ctx, inst, nrows):
    """mht_solve_blp with a row count of the caller's choice and a poisoned output: (return code, selection as left by the call)."""
    cols, sizes, cost = inst["cols"], inst["sizes"], inst["cost"]
    nH, nT = len(cols), len(sizes)
    depth = max(1, max(len(c) for c in cols))
    rows = -np.ones((depth, nH), dtype=np.int32)
    for h, c in enumerate(cols):
        rows[:len(c), h] = c
    dev = ctx.device
    gp = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    rw, cs = torch.from_numpy(rows).to(dev), torch.from_numpy(np.asarray(cost, dtype=np.float64)).to(dev)
    sel = torch.full((nT,), -7, dtype=torch.int32, device=dev)
    obj, st, it, nd = C.c_double(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    torch.cuda.synchronize()
    rc = ctx.lib.mht_solve_blp(ctx.handle, nH, nT, nrows, depth, gp.data_ptr(), rw.data_ptr(), cs.data_ptr(), 200, 1 << 20, sel.data_ptr(),
                               C.byref(obj), C.byref(st), C.byref(it), C.byref(nd))
    torch.cuda.synchronize()
    return rc, sel.cpu().numpy().tolist()


@pytest.mark.parametrize("nx", [4, 6])
def test_rows_numbered_up_to_the_launch_capacity(ctx_of, sweep, nx):
    """Three small clusters (5, 9 and 12 targets, without a dual certificate) with their rows mapped injectively to the top of the range the
    launch accepts: the largest used id is nRows - 1, nRows the largest row count whose bitset fits the launch's LDS next to the default
    tier's tables (45 952 by the formula above).  nRows is accepted and gives the recorded optimum; nRows + 128 is refused with
    MHT_E_CAPACITY and the selection buffer is left alone."""
    n_rows = largest_accepted_rows()
    assert n_rows == 45952 and blp_lds_bytes(n_rows) <= LDS_LIMIT < blp_lds_bytes(n_rows + 1) == blp_lds_bytes(n_rows + 128)
    picked = []
    for K in (5, 9, 12):
        picked.append(next(i for i in sweep if i["family"] == "small" and i["K"] == K and i["gap"] and i["unique"] and i["variant"] == "grid" and i["PD"] >= 4))
    for inst in picked:
        used = sorted({int(r) for c in inst["cols"] for r in c})
        stride = (n_rows - 1) // max(1, len(used) - 1)      # (rank j of the used rows -> n_rows - 1 - j * stride: injective, spread over the whole range)
        to = {r: n_rows - 1 - j * stride for j, r in enumerate(used)}
        high = dict(inst)
        high["cols"] = [np.array([to[int(r)] for r in c], dtype=np.int64) for c in inst["cols"]]
        assert max(int(c.max()) for c in high["cols"] if len(c)) == n_rows - 1 and min(to.values()) < 64
        solve(ctx_of[nx], high, "rows up to %d" % (n_rows - 1))
        rc, left = raw_blp(ctx_of[nx], high, n_rows + 128)
        assert rc == _lib.MHT_E_CAPACITY and left == [-7] * len(inst["sizes"]), (rc, left)
