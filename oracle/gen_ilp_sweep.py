"""TEST INFRASTRUCTURE (development container only): tests/golden/g24_ilp_sweep.npz.

Synthetic 0-1 ILPs that sit ON the dispatch thresholds of pymht_amd/csrc/mht_blp.hip (targets K, columns nH, used rows nR, row depth
PD), with their exact optima.  The recorded tracker instances (G4 ... G20) fall where the scenarios put them; these fall where the
solver changes its path.

Instance model (tracker-like): target k has n_k columns, the last one empty with cost 0 (the missed-detection leaf: every instance is
feasible), every other column takes 1..PD distinct rows of a pool of R rows; with probability `dup` a target copies the row sets of
the previous target but not its costs (near-duplicate tracks: duality gaps).  Costs -(len(col) + U(0, 1.5)); every structure is
recorded twice, with these costs ("cont") and with the same costs rounded to a multiple of 2^-10 ("grid": every partial sum is exact
in float64, so the solver's objective has to equal the reference bit for bit).

Families (tag `family`), every shape in both cost variants:
  small    K in 1 2 3 4 5 8 9 10 11 12, n_k in 2..6, R = max(2, floor(1.2 K)), PD in 1 4 8, dup 0.5 (0.95 for K <= 4 where a gap is asked for)
  wide     K in 3 10 with 511, 512, 513 columns in all (the column copy's wrap, ENUM_WIDE)
  middle   K in 16 23 24 25 63 64 65: a hard core of 10 targets of the small family + targets of the same densities on private rows
  tier     core + padding at (K, nH) = (256, 2048) (256, 2049) (257, 2056), ~500 used rows
  rowedge  core + padding, K = 128, exactly 1022 1023 1024 1025 used rows
  depth    PD in 8 9 15 (longest column exactly that long) at K = 6 (flat) and K = 30 (core + padding)
A padding target's columns use rows private to that target, so the optimum is the core's plus the padding's per-target minimum --
exact, and milliseconds where HiGHS on the flat instance does not finish (257 targets / 2 056 columns, presolve off: > 1 minute).
The core LEADS (lowest target indices).  The forest hands the solver connected components only; a cluster with independent parts exists
at the stateless seam alone, where it is the vehicle that carries a hard core across the K / nH / nR thresholds.  The branch and
bound visits the targets whose minimiser touches a contested or priced row first and the others by index: padding in front of a core
with an LP gap would be branched on before the gap is closed, every padding column within the gap of its target's best doubling the
tree -- hardness made by the vehicle, not by the shape under test.  (Measured on an MI355X with the core of the PD 8 structures
trailing: 63 and 65 targets ran into the node limit of 2^20; 25 and 64 targets took 24 k .. 27 k nodes and 160 .. 220 ms where the
leading core takes 600 .. 1 600 nodes and 4 ms.)

References: HiGHS (oracle.solve_blp_exact, presolve off) for the optimum; a second HiGHS solve with the no-good cut
sum(tau[sel]) <= nT - 1 for uniqueness (unique: the second optimum is worse by more than 1e-9); scipy.optimize.linprog(method="highs")
for the LP relaxation; solve_blp_bruteforce wherever the instance has at most 10^5 combinations (and HiGHS on the whole instance for
the core + padding instances of up to 65 targets) as a cross-check of the references themselves.

Seeds: every (family, shape, slot) walks a fixed sequence of seeds; a slot that asks for an LP gap takes the first seed of its sequence
whose two cost variants both have obj - lp > 1e-6 (no dual certificate exists there: the solver has to enumerate or branch).  At least
30 % of the instances of every small / middle shape (a shape is a K) are such; K = 1 cannot be (one target: the LP is integral), nor can
PD = 1 (an assignment problem), so the gap slots are the PD 4 and 8 ones.

File layout: per instance i%03d_{col_ptr, col_rows, sizes, cost, sel, obj, unique} (what tests/test_cluster_blp_gpu.load_instances
reads) and, indexed by instance, the arrays lp, second, family, variant, K, nH, nR, PD, bf (brute force was run), bf_obj, bf_ties.
Written with fixed zip time stamps: a rerun gives the same bytes (SciPy 1.15.3).

Run:  python oracle/gen_ilp_sweep.py          (~half a minute)
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import mht_oracle as orc  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
GRID = 1024.0          # grid costs are multiples of 2^-10
GAP = 1e-6             # an instance "has an LP gap" when obj - lp exceeds this
BF_MAX = 100000        # brute force up to this many combinations

SMALL_K = (1, 2, 3, 4, 5, 8, 9, 10, 11, 12)
MIDDLE_K = (16, 23, 24, 25, 63, 64, 65)


# ---------------------------------------------------------------------------------------------------------------------------------
# the instance model
# ---------------------------------------------------------------------------------------------------------------------------------
def draw_targets(rng, K, R, PD, dup, n_lo=2, n_hi=6, row0=0, n_cols=None):
    """K targets over the row pool row0 .. row0 + R - 1.  Returns (cols, sizes); the first column of the first target is as long as the
    model allows (min(PD, R) rows), so that the depth the solver sees is the shape's.  n_cols: the column count of every target (wide)."""
    cols, sizes, prev = [], [], None
    top = min(PD, R)
    for k in range(K):
        n = int(rng.integers(n_lo, n_hi + 1)) if n_cols is None else int(n_cols[k])
        if prev is not None and rng.uniform() < dup and (n_cols is None or len(prev) == n - 1):
            mine = [list(c) for c in prev]
        else:
            mine = []
            for j in range(n - 1):
                ln = top if (k == 0 and j == 0) else int(rng.integers(1, top + 1))
                mine.append(sorted(int(r) + row0 for r in rng.choice(R, size=ln, replace=False)))
        prev = mine
        cols += mine + [[]]
        sizes.append(len(mine) + 1)
    return cols, sizes


def draw_padding(rng, n_targets, rows_of, n_cols_of, PD, row0):
    """Padding targets: target p owns rows_of[p] rows nobody else uses and has n_cols_of[p] columns (the last one empty); its first
    columns are consecutive chunks of at most four of its rows (every private row is used), the rest take 1..PD of them."""
    cols, sizes = [], []
    for p in range(n_targets):
        r, n = int(rows_of[p]), int(n_cols_of[p])
        mine = [list(range(row0 + b, row0 + min(b + 4, r))) for b in range(0, r, 4)]
        assert len(mine) <= n - 1, (r, n)
        top = min(PD, r)
        while len(mine) < n - 1:
            ln = int(rng.integers(1, top + 1))
            mine.append(sorted(int(x) + row0 for x in rng.choice(r, size=ln, replace=False)))
        row0 += r
        cols += mine + [[]]
        sizes.append(n)
    return cols, sizes


def draw_costs(rng, cols):
    c = np.array([-(len(col) + rng.uniform(0.0, 1.5)) if len(col) else 0.0 for col in cols], dtype=np.float64)
    grid = np.round(c * GRID) / GRID
    return c, grid


# ---------------------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------------------
def constraint_matrix(cols, sizes, extra=None):
    from scipy.sparse import csr_matrix
    nH, nT = len(cols), len(sizes)
    used = sorted({r for c in cols for r in c})
    rid = {r: i for i, r in enumerate(used)}
    rr, cc = [], []
    for h, c in enumerate(cols):
        rr += [rid[r] for r in c]
        cc += [h] * len(c)
    g = 0
    for t, s in enumerate(sizes):
        rr += [len(used) + t] * s
        cc += list(range(g, g + s))
        g += s
    n = len(used) + nT
    if extra is not None:
        rr += [n] * len(extra)
        cc += list(extra)
        n += 1
    return csr_matrix((np.ones(len(rr)), (rr, cc)), shape=(n, nH)), len(used)


def lp_value(cols, sizes, cost):
    from scipy.optimize import linprog
    A, nR = constraint_matrix(cols, sizes)
    res = linprog(np.asarray(cost, float), A_ub=A[:nR] if nR else None, b_ub=np.ones(nR) if nR else None, A_eq=A[nR:], b_eq=np.ones(len(sizes)),
                  bounds=(0, 1), method="highs", options={"presolve": False})
    assert res.status == 0, res.message
    return float(res.fun)


def second_best(cols, sizes, cost, sel):
    """Optimum under the no-good cut sum(tau[sel]) <= nT - 1: (selection, value), (None, inf) if `sel` is the only feasible point."""
    from scipy.optimize import milp, LinearConstraint, Bounds
    nT = len(sizes)
    A, nR = constraint_matrix(cols, sizes, extra=sel)
    lo = np.concatenate([np.full(nR, -np.inf), np.ones(nT), [-np.inf]])
    hi = np.concatenate([np.ones(nR + nT), [nT - 1]])
    f = np.asarray(cost, dtype=np.float64)
    res = milp(f, constraints=LinearConstraint(A, lo, hi), integrality=np.ones(len(cols)), bounds=Bounds(0, 1),
               options={"mip_rel_gap": 0.0, "presolve": False})
    if res.status != 0:
        return None, float("inf")
    s2 = [int(i) for i in np.nonzero(np.round(res.x) > 0.5)[0]]
    assert len(s2) == nT
    return s2, float(np.sum(f[s2]))


def exact(cols, sizes, cost):
    """(sel, obj, second): HiGHS, re-seated on the cut solve's point should that one be better (HiGHS stops at an absolute gap of 1e-6)."""
    sel, obj = orc.solve_blp_exact(cols, sizes, cost)
    for _ in range(4):
        s2, second = second_best(cols, sizes, cost, sel)
        if not second < obj - 1e-12:
            return sel, obj, second
        sel, obj = s2, second
    raise AssertionError("HiGHS does not settle")


def n_combinations(sizes):
    n = 1
    for s in sizes:
        n *= int(s)
        if n > BF_MAX:
            return n
    return n


def solve_flat(cols, sizes, cost):
    sel, obj, second = exact(cols, sizes, cost)
    out = dict(sel=sel, obj=obj, second=second, lp=lp_value(cols, sizes, cost), bf=False, bf_obj=np.nan, bf_ties=0)
    if n_combinations(sizes) <= BF_MAX:
        bs, bo, ties = orc.solve_blp_bruteforce(cols, sizes, cost)
        assert abs(bo - obj) <= 1e-12 * max(1.0, abs(obj)), (bo, obj)
        if second > obj + 1e-9:
            assert sorted(bs) == sel and ties == 1
        out.update(bf=True, bf_obj=bo, bf_ties=ties)
    return out


def solve_padded(core, pad, cost, check_whole):
    """core / pad = (cols, sizes) of the two parts, cost in the order of the assembled instance (the core leads)."""
    (ccols, csizes), (pcols, psizes) = core, pad
    nc = len(ccols)
    c_core, c_pad = cost[:nc], cost[nc:]
    r = solve_flat(ccols, csizes, c_core)
    sel = list(r["sel"])
    obj_pad, gap_pad, g = [], float("inf"), 0
    for s in psizes:
        seg = c_pad[g:g + s]
        order = np.argsort(seg, kind="stable")
        sel.append(int(order[0]) + g + nc)
        obj_pad.append(float(seg[order[0]]))
        gap_pad = min(gap_pad, float(seg[order[1]] - seg[order[0]]))
        g += s
    sel = sorted(sel)
    obj = float(np.sum(np.asarray(cost)[sel]))
    pad_sum = float(np.sum(obj_pad))
    second = min(r["second"] + pad_sum, obj + gap_pad)
    out = dict(sel=sel, obj=obj, second=second, lp=r["lp"] + pad_sum, bf=False, bf_obj=np.nan, bf_ties=0)
    if check_whole:
        cols, sizes = ccols + pcols, csizes + psizes
        ws, wo = orc.solve_blp_exact(cols, sizes, cost)
        assert abs(wo - obj) <= 1e-9 * max(1.0, abs(obj)), (wo, obj)
        if second > obj + 1e-9:
            assert ws == sel
        assert abs(lp_value(cols, sizes, cost) - out["lp"]) <= 1e-7 * max(1.0, abs(obj))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------------------------
class Sweep:
    def __init__(self):
        self.inst = []

    def add(self, family, cols, sizes, costs, solve):
        """costs = (cont, grid); solve(cost) -> reference dict.  Returns the two reference dicts."""
        refs = []
        for variant, cost in (("cont", costs[0]), ("grid", costs[1])):
            r = solve(cost)
            refs.append(r)
            self.inst.append(dict(family=family, variant=variant, cols=cols, sizes=sizes, cost=cost, ref=r))
        return refs


def small_structure(seed, K, PD, dup, R=None):
    rng = np.random.default_rng(seed)
    R = max(2, (12 * K) // 10) if R is None else R
    cols, sizes = draw_targets(rng, K, R, PD, dup)
    return cols, sizes, draw_costs(rng, cols)


def has_gap(cols, sizes, costs):
    """Both cost variants have an LP gap (cheap test first: the LP, then the exact solve)."""
    for c in costs:
        sel, obj = orc.solve_blp_exact(cols, sizes, c)
        if not obj - lp_value(cols, sizes, c) > 10 * GAP:
            return False
    return True


def pick_small(base_seed, K, PD, want_gap, R=None):
    """The first seed of the sequence base_seed, base_seed + 1, ... that gives what the slot asks for."""
    dup = 0.95 if (want_gap and K <= 4) else 0.5
    for seed in range(base_seed, base_seed + 400):
        cols, sizes, costs = small_structure(seed, K, PD, dup, R)
        if max(len(c) for c in cols) != min(PD, max(2, (12 * K) // 10) if R is None else R):
            continue
        if not want_gap or has_gap(cols, sizes, costs):
            return seed, cols, sizes, costs
    raise AssertionError("no seed with an LP gap for K=%d PD=%d" % (K, PD))


def gen_small(sw):
    # ten structures per K: PD 1 x 2, PD 4 x 4 (two with a gap), PD 8 x 4 (two with a gap); K = 1 has no gap to ask for
    for K in SMALL_K:
        for PD, n_any, n_gap in ((1, 2, 0), (4, 2, 2), (8, 2, 2)):
            for slot in range(n_any + n_gap):
                want = slot >= n_any and K >= 2
                seed, cols, sizes, costs = pick_small(100000 * K + 1000 * PD + 100 * slot, K, PD, want)
                sw.add("small", cols, sizes, costs, lambda c: solve_flat(cols, sizes, c))
        print("small K=%d done" % K, flush=True)


def gen_wide(sw):
    for K in (3, 10):
        for total in (511, 512, 513):
            rng = np.random.default_rng(7000000 + 1000 * K + total)
            n_cols = [total // K + (1 if k < total % K else 0) for k in range(K)]
            cols, sizes = draw_targets(rng, K, (12 * K) // 10 + 4, 4, 0.5, n_cols=n_cols)
            assert len(cols) == total
            sw.add("wide", cols, sizes, draw_costs(rng, cols), lambda c: solve_flat(cols, sizes, c))
    print("wide done", flush=True)


def padded(sw, family, seed, K, core, core_PD, rows_of, n_cols_of, check_whole):
    """core = (cols, sizes, costs) of pick_small: it keeps its costs (and with them its LP gap), the padding draws its own."""
    ccols, csizes, ccosts = core
    rng = np.random.default_rng(seed + 500)
    row0 = 1 + max(r for c in ccols for r in c)
    pcols, psizes = draw_padding(rng, K - len(csizes), rows_of, n_cols_of, core_PD, row0)
    pcosts = draw_costs(rng, pcols)
    cols, sizes = ccols + pcols, csizes + psizes
    costs = [np.concatenate([c, p]) for c, p in zip(ccosts, pcosts)]
    sw.add(family, cols, sizes, costs, lambda c: solve_padded((ccols, csizes), (pcols, psizes), c, check_whole))


def gen_middle(sw):
    # three structures per K: two whose core has an LP gap (PD 4 and 8), one as it comes
    for K in MIDDLE_K:
        n_pad = K - 10
        for slot, (want, PD) in enumerate(((True, 4), (True, 8), (False, 4))):
            seed, ccols, csizes, ccosts = pick_small(20000000 + 100000 * K + 1000 * slot, 10, PD, want)
            rng = np.random.default_rng(seed + 250)
            padded(sw, "middle", seed, K, (ccols, csizes, ccosts), PD, rng.integers(1, 4, size=n_pad), rng.integers(2, 7, size=n_pad), True)
        print("middle K=%d done" % K, flush=True)


def spread(total, n):
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


def gen_tier(sw):
    for i, (K, nH) in enumerate(((256, 2048), (256, 2049), (257, 2056))):
        seed, ccols, csizes, ccosts = pick_small(30000000 + 1000 * i, 10, 4, True)
        n_pad = K - 10
        padded(sw, "tier", seed, K, (ccols, csizes, ccosts), 4, [2] * n_pad, spread(nH - len(ccols), n_pad), False)
        assert len(sw.inst[-1]["cols"]) == nH and len(sw.inst[-1]["sizes"]) == K
    print("tier done", flush=True)


def gen_rowedge(sw):
    for i, nR in enumerate((1022, 1023, 1024, 1025)):
        base = 40000000 + 1000 * i
        while True:      # (a core that uses every row of its pool: the padding's rows follow on without a hole)
            seed, ccols, csizes, ccosts = pick_small(base, 10, 4, True)
            core_rows = len({r for c in ccols for r in c})
            if 1 + max(r for c in ccols for r in c) == core_rows:
                break
            base = seed + 1
        n_pad = 118
        padded(sw, "rowedge", seed, 128, (ccols, csizes, ccosts), 4, spread(nR - core_rows, n_pad), [9] * n_pad, False)
        assert len({r for c in sw.inst[-1]["cols"] for r in c}) == nR
    print("rowedge done", flush=True)


def gen_depth(sw):
    for PD in (8, 9, 15):
        R = PD + 3
        for slot in range(2):      # K = 6, flat: the second structure has an LP gap
            seed, cols, sizes, costs = pick_small(50000000 + 1000 * PD + 100 * slot, 6, PD, slot == 1, R)
            sw.add("depth", cols, sizes, costs, lambda c: solve_flat(cols, sizes, c))
        # K = 30: a core of 10 with a gap + 20 padding targets with PD .. PD + 2 private rows each
        seed, ccols, csizes, ccosts = pick_small(51000000 + 1000 * PD, 10, PD, True, R)
        rng = np.random.default_rng(seed + 250)
        padded(sw, "depth", seed, 30, (ccols, csizes, ccosts), PD, rng.integers(PD, PD + 3, size=20), rng.integers(7, 10, size=20), True)
    print("depth done", flush=True)


# ---------------------------------------------------------------------------------------------------------------------------------
def write_npz(path, fx):
    """np.savez_compressed with fixed time stamps (the same arrays give the same bytes)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, arr in fx.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    sw = Sweep()
    gen_small(sw)
    gen_wide(sw)
    gen_middle(sw)
    gen_tier(sw)
    gen_rowedge(sw)
    gen_depth(sw)
    fx, n = {}, len(sw.inst)
    tags = dict(lp=np.zeros(n), second=np.zeros(n), family=[], variant=[], K=np.zeros(n, np.int32), nH=np.zeros(n, np.int32),
                nR=np.zeros(n, np.int32), PD=np.zeros(n, np.int32), bf=np.zeros(n, bool), bf_obj=np.zeros(n), bf_ties=np.zeros(n, np.int32))
    for i, inst in enumerate(sw.inst):
        cols, sizes, cost, r = inst["cols"], inst["sizes"], inst["cost"], inst["ref"]
        p = "i%03d_" % i
        fx[p + "col_ptr"] = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
        fx[p + "col_rows"] = np.array([x for c in cols for x in c], dtype=np.int32)
        fx[p + "sizes"] = np.array(sizes, dtype=np.int32)
        fx[p + "cost"] = np.asarray(cost, dtype=np.float64)
        fx[p + "sel"] = np.array(r["sel"], dtype=np.int32)
        fx[p + "obj"] = np.float64(r["obj"])
        fx[p + "unique"] = np.bool_(r["second"] > r["obj"] + 1e-9)
        tags["lp"][i], tags["second"][i] = r["lp"], r["second"]
        tags["family"].append(inst["family"])
        tags["variant"].append(inst["variant"])
        tags["K"][i], tags["nH"][i] = len(sizes), len(cols)
        tags["nR"][i] = len({x for c in cols for x in c})
        tags["PD"][i] = max(len(c) for c in cols)
        tags["bf"][i], tags["bf_obj"][i], tags["bf_ties"][i] = r["bf"], r["bf_obj"], r["bf_ties"]
    fx["n_inst"] = np.int64(n)
    for k, v in tags.items():
        fx[k] = np.array(v)
    path = os.path.join(GOLD, "g24_ilp_sweep.npz")
    write_npz(path, fx)
    gap = (np.array([float(fx["i%03d_obj" % i]) for i in range(n)]) - tags["lp"]) > GAP
    fam = np.array(tags["family"])
    for f in ("small", "wide", "middle", "tier", "rowedge", "depth"):
        m = fam == f
        print("%-8s %3d instances, %3d with an LP gap, %3d unique, %3d brute-forced" % (
            f, m.sum(), (gap & m).sum(), sum(bool(fx["i%03d_unique" % i]) for i in np.nonzero(m)[0]), (tags["bf"] & m).sum()))
    print("wrote %s: %d instances, %d bytes" % (path, n, os.path.getsize(path)))


if __name__ == "__main__":
    main()
