"""The test-only probe library of the hot path's helper headers (tests/devprobe/probe.hip: csrc/mht_wave.h, csrc/mht_uf.h,
csrc/mht_vtab.h behind one small kernel per helper) and the plain host references its tests compare with: the balanced pairwise
tree of `wave_sum`, a ten-line union-find, a restatement of the value table's hash, and the generators of the graphs and values both
tests/test_devprobe_cpu.py (the references against each other, no GPU) and tests/test_devprobe_gpu.py (the helpers against them) use."""
import ctypes as C
import functools
import math
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "devprobe", "probe.hip")
M64 = (1 << 64) - 1


def build_command(so, nx):
    """The probe with the library's own flags (pymht_amd.build.FLAGS: -ffp-contract=off, --offload-arch=gfx950), -DMHT_NX=6 in the six-state build"""
    from pymht_amd import build as B
    return ([os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"] + list(B.FLAGS) + (["-DMHT_NX=%d" % nx] if nx != 4 else [])
            + ["-I", B.CSRC, SRC, "-o", so])


def build(directory, nx):
    """tests/devprobe/probe.hip compiled into `directory` for the nx-state build; the ctypes library (lib.nx, lib.NP, lib.VT_PW, lib.GKQ)"""
    assert nx in (4, 6)
    so = os.path.join(str(directory), "libdevprobe%d.so" % nx)
    subprocess.check_call(build_command(so, nx))
    try:
        import torch  # noqa: F401  (its HIP runtime first, as pymht_amd._lib does)
    except ImportError:
        pass
    lib = C.CDLL(so)
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    for name in ("scan_u32", "sum_i32", "min_i32", "max_i32", "sum_f64", "min_value", "row16_min_value", "scan_halves", "box_i32"):
        f = getattr(lib, "probe_" + name)
        f.restype, f.argtypes = C.c_int, [i32, i32, vp, vp]
    for name in ("min_pair", "row16_min_pair"):
        f = getattr(lib, "probe_" + name)
        f.restype, f.argtypes = C.c_int, [i32, i32, vp, vp, vp, vp]
    lib.probe_uf_link.restype, lib.probe_uf_link.argtypes = C.c_int, [vp, i32, u32, vp, vp, i32]
    lib.probe_uf_claim.restype, lib.probe_uf_claim.argtypes = C.c_int, [vp, i32, i32, vp, vp, u32, i32, vp]
    table = [vp] * 7 + [i32, u32]
    lib.probe_vt_insert.restype, lib.probe_vt_insert.argtypes = C.c_int, table + [i32, vp, i32, vp, vp, vp, vp]
    lib.probe_vt_load.restype, lib.probe_vt_load.argtypes = C.c_int, table + [i32, vp, vp, vp]
    lib.probe_constants.restype, lib.probe_constants.argtypes = C.c_int, [vp]
    k = np.zeros(4, dtype=np.int32)
    lib.probe_constants(k.ctypes.data)
    lib.nx, lib.NP, lib.VT_PW, lib.GKQ = (int(v) for v in k)
    assert lib.nx == nx and lib.NP == nx * nx and lib.VT_PW == nx * nx // 2
    return lib


# ---- wave_sum: the balanced pairwise tree over the lanes -----------------------------------------------------------------------------
def pairwise_tree(x):
    """six rounds of x = x[0::2] + x[1::2] over the last axis (64 lanes)"""
    x = np.asarray(x, dtype=np.float64)
    assert x.shape[-1] == 64
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(6):
            x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


FSUM_BOUND = 6 * 2.0 ** -53      # six additions deep: |tree - exact| <= 6 u sum|v| (to first order; the standard bound of pairwise summation)


def fsum_rows(x):
    return np.array([math.fsum(r) for r in x]), np.array([math.fsum(np.abs(r)) for r in x])


def sum_inputs(seed=11, n_random=96):
    """finite rows for wave_sum: 64 one-hot rows, random rows spanning 16 decades, rows of cancelling pairs, all -0.0, all equal"""
    rng = np.random.default_rng(seed)
    rows = [np.eye(64)]
    rows.append(rng.standard_normal((n_random, 64)) * 10.0 ** rng.uniform(-8, 8, (n_random, 64)))
    c = rng.standard_normal((16, 32)) * 10.0 ** rng.uniform(-8, 8, (16, 32))
    canc = np.concatenate([c, -c], axis=1)
    rows.append(canc)                                                   # v and -v 32 lanes apart
    rows.append(np.stack([rng.permutation(r) for r in canc]))           # ... and anywhere
    rows.append(np.full((1, 64), -0.0))
    rows.append(np.full((1, 64), 0.1))
    big = rng.standard_normal((2, 64))
    big[:, 5] = 1e300
    big[0, 40] = -1e300
    rows.append(big)
    return np.concatenate(rows)


# ---- union-find ---------------------------------------------------------------------------------------------------------------------
def host_uf(T, ex, ey):
    """label[t] = the smallest member of t's component"""
    parent = list(range(T))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for x, y in zip(ex.tolist(), ey.tolist()):
        a, b = find(x), find(y)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(t) for t in range(T)], dtype=np.int64)


def labels_of_clusters(clusters, T):
    lab = np.full(T, -1, dtype=np.int64)
    for c in clusters:
        lab[c] = c.min()
    assert (lab >= 0).all()
    return lab


def edges_as_sets(T, ex, ey):
    """an edge list as association sets for mht_oracle.find_clusters: edge e is a node shared by its two ends"""
    sets = [[] for _ in range(T)]
    for e, (x, y) in enumerate(zip(ex.tolist(), ey.tolist())):
        sets[x].append(e)
        if y != x:
            sets[y].append(e)
    return sets


def sets_as_edges(sets):
    """association sets as an edge list for host_uf: every node chains the targets that hold it"""
    last, ex, ey = {}, [], []
    for t, s in enumerate(sets):
        for m in s:
            if m in last:
                ex.append(last[m])
                ey.append(t)
            last[m] = t
    return np.array(ex, dtype=np.int32), np.array(ey, dtype=np.int32)


def sets_as_bits(sets, AW):
    a = np.zeros((len(sets), AW), dtype=np.uint64)
    for t, s in enumerate(sets):
        for m in s:
            assert 0 <= m < AW * 64
            a[t, m >> 6] |= np.uint64(1 << (m & 63))
    return a


def read_parents(words, epoch):
    """(has, par): which targets hold a parent word of `epoch`, and the parent it names"""
    words = np.asarray(words, dtype=np.uint64)
    has = (words >> np.uint64(32)) == np.uint64(epoch)
    par = (np.uint64(0xffffffff) - (words & np.uint64(0xffffffff))).astype(np.int64)
    return has, par


def check_forest(words, epoch, ref_label):
    """The three properties of a finished union-find under `epoch` against the reference labels (smallest member of the component)"""
    T = len(ref_label)
    has, par = read_parents(words[:T], epoch)
    idx = np.arange(T)
    assert (par[has] < idx[has]).all(), "a parent word of this epoch names an index that is not smaller"
    lab = np.where(has, par, idx)
    for _ in range(40):      # parents only go down: pointer doubling ends within log2(T) rounds
        nxt = lab[lab]
        if (nxt == lab).all():
            break
        lab = nxt
    bad = np.flatnonzero(lab != ref_label)
    assert bad.size == 0, "%d walks end elsewhere than at the smallest member, first: target %d ends at %d, component's smallest %d" % (
        bad.size, bad[0], lab[bad[0]], ref_label[bad[0]])
    root = ref_label == idx
    assert has[~root].all(), "a member that is not the smallest holds no parent word of this epoch"
    assert not has[root].any(), "a smallest member holds a parent word of this epoch"


@functools.lru_cache(maxsize=None)
def link_graphs():
    """name -> (T, ex, ey) of the uf_link tests: T <= 20 000 targets, E <= 200 000 edges"""
    rng = np.random.default_rng(5)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    g = {}
    g["no_edges"] = (1000, i32([]), i32([]))
    g["self_loops"] = (1000, i32(np.arange(1000)), i32(np.arange(1000)))
    p = np.arange(4999)
    g["path_ascending"] = (5000, i32(p), i32(p + 1))
    g["path_descending"] = (5000, i32(p[::-1] + 1), i32(p[::-1]))
    q = rng.permutation(4999)
    flip = rng.random(4999) < 0.5
    g["path_shuffled"] = (5000, i32(np.where(flip, q, q + 1)), i32(np.where(flip, q + 1, q)))
    leaves = rng.permutation(10000) + 1
    g["star_at_0"] = (10001, i32(np.zeros(10000)), i32(leaves))
    g["star_at_last"] = (10001, i32(leaves - 1), i32(np.full(10000, 10000)))
    g["one_edge_1000_times"] = (100, i32(np.full(1000, 63)), i32(np.full(1000, 17)))
    a, b = np.triu_indices(96, 1)
    o = rng.permutation(len(a))
    members = np.sort(rng.choice(300, 96, replace=False))      # (the 96 sit among 300 targets, the others stay alone)
    g["complete_96"] = (300, i32(members[a[o]]), i32(members[b[o]]))
    T, E, groups = 20000, 200000, 300
    grp = rng.integers(0, groups, T)
    order = np.argsort(grp, kind="stable")
    start = np.searchsorted(grp[order], np.arange(groups))
    size = np.bincount(grp, minlength=groups)
    ge = rng.integers(0, groups, E)
    x = order[start[ge] + rng.integers(0, 1 << 30, E) % size[ge]]
    y = order[start[ge] + rng.integers(0, 1 << 30, E) % size[ge]]
    g["sparse_random"] = (T, i32(x), i32(y))
    return g


def epoch_graphs():
    """(epoch, T, ex, ey) run one after the other on ONE parent array of 20 000 words prefilled under epoch 3"""
    g = link_graphs()
    T = 20000
    return [(6, T) + g["sparse_random"][1:], (7, T) + g["path_shuffled"][1:], (8, T, g["star_at_last"][1] + 9999, g["star_at_last"][2] + 9999)]


CLAIM_AW = (1, 63, 64, 65, 130)
CLAIM_CAP = (0, 1, 3, 64)


@functools.lru_cache(maxsize=None)
def claim_scenes(AW):
    """name -> association sets (lists of node numbers in [0, 64 AW)) of the uf_claim tests, T <= 3 000"""
    rng = np.random.default_rng(100 + AW)
    N = AW * 64
    sc = {}
    # rows with more than four and with all 64 bits of a word set
    sets = []
    for t in range(200):
        w = int(rng.integers(0, AW))
        kind = t % 4
        if kind == 0:
            s = set(range(w * 64, w * 64 + 64))                                        # a full word
        elif kind == 1:
            s = set((w * 64 + rng.choice(64, int(rng.integers(5, 40)), replace=False)).tolist())      # more than four in one word
        elif kind == 2:
            s = set(rng.choice(N, min(N, int(rng.integers(1, 12))), replace=False).tolist())
        else:
            s = set()                                                                  # a target without measurements
        sets.append(sorted(s))
    sc["dense_rows"] = sets
    # one node shared by every target
    shared = int(rng.integers(0, N))
    sc["one_shared_node"] = [sorted({shared} | set(rng.choice(N, 2).tolist())) if AW > 1 else [shared] for _ in range(3000)]
    # disjoint sets: nobody meets anybody
    T = min(3000, N)
    per = max(1, min(3, N // T))
    perm = rng.permutation(N)
    sc["disjoint"] = [sorted(perm[t * per:(t + 1) * per].tolist()) for t in range(T)]
    # sparse: targets pick nodes near their own place -> many components of several targets
    T = 3000 if AW > 1 else 400
    sets = []
    for t in range(T):
        centre = (t * N) // T
        k = int(rng.integers(0, 4))
        sets.append(sorted(set(((centre + rng.integers(-2, 3, k)) % N).tolist())) if t % 50 else [])
    sc["sparse"] = sets
    return sc


# ---- the value table ----------------------------------------------------------------------------------------------------------------
VT_PENDING = 0xffffffff
VT_TAG64 = 0x80000000


def vt_hash(words, pd_bits, f64):
    """mht_vtab.h's hash restated: words [V][NW] uint64, pd_bits [V] uint64 -> (tag [V], h & 0xffffffff [V]); the start slot is the second & hmask"""
    words = np.atleast_2d(np.asarray(words, dtype=np.uint64))
    h = np.uint64(0x9e3779b97f4a7c15) ^ np.asarray(pd_bits, dtype=np.uint64).reshape(-1)
    h = np.broadcast_to(h, (max(words.shape[0], h.size),)).copy()      # (one value under many P_d, or one P_d for many values)
    for q in range(words.shape[1]):
        h ^= words[:, q]
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(29)
    h *= np.uint64(0xc4ceb9fe1a85ec53)
    h ^= h >> np.uint64(32)
    top = (h >> np.uint64(32)).astype(np.uint32)
    tag = (top | np.uint32(VT_TAG64)) if f64 else (top & np.uint32(VT_TAG64 - 1))
    return tag, (h & np.uint64(0xffffffff)).astype(np.uint32)


def table_size(vcap):
    """the forest's rule: the power of two >= 4 vcap"""
    n = 4
    while n < 4 * vcap:
        n *= 2
    return n


class Values:
    """A list of values for the table: kind [V] (0 float32, 1 float64), words [V][2 VT_PW] uint64 (a float32 value fills the first
    VT_PW), pd [V] float64"""

    def __init__(self, nx, kind, words, pd):
        self.nx, self.pw = nx, nx * nx // 2
        self.kind = np.ascontiguousarray(kind, dtype=np.int32)
        self.words = np.ascontiguousarray(words, dtype=np.uint64)
        self.pd = np.ascontiguousarray(pd, dtype=np.float64)
        assert self.words.shape == (len(self.kind), 2 * self.pw) and self.pd.shape == self.kind.shape

    def __len__(self):
        return len(self.kind)

    def key(self, v):
        """(kind, value bits, P_d bits): what the table tells values apart by"""
        nw = self.pw * (2 if self.kind[v] else 1)
        return (int(self.kind[v]), self.words[v, :nw].tobytes(), self.pd[v:v + 1].tobytes())

    def keys(self):
        return [self.key(v) for v in range(len(self))]

    def n_ids(self):
        """ids the distinct values take: one per float32 value, two per float64 one"""
        return sum(1 + k[0] for k in set(self.keys()))

    def hash(self, v):
        f64 = bool(self.kind[v])
        tag, lo = vt_hash(self.words[v:v + 1, :self.pw * (2 if f64 else 1)], self.pd[v:v + 1].view(np.uint64), f64)
        return int(tag[0]), int(lo[0])

    def tags(self):
        """the slot tag of every value of the list"""
        out = np.zeros(len(self), dtype=np.int64)
        for kind in (0, 1):
            sel = np.flatnonzero(self.kind == kind)
            if len(sel):
                out[sel] = vt_hash(self.words[sel, :self.pw * (kind + 1)], self.pd[sel].view(np.uint64), bool(kind))[0]
        return out

    @staticmethod
    def concat(a, b):
        return Values(a.nx, np.concatenate([a.kind, b.kind]), np.concatenate([a.words, b.words]), np.concatenate([a.pd, b.pd]))


def f32_words(P):
    """[V][NP] float32 -> [V][2 VT_PW] words"""
    P = np.ascontiguousarray(P, dtype=np.float32)
    w = P.view(np.uint64)
    return np.concatenate([w, np.zeros_like(w)], axis=1)


def f64_words(P):
    return np.ascontiguousarray(P, dtype=np.float64).view(np.uint64).copy()


def random_f32_values(nx, V, seed):
    """V distinct float32 covariances under three P_d"""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((V, nx * nx)).astype(np.float32) * 50.0
    return Values(nx, np.zeros(V), f32_words(P), rng.choice([0.9, 0.8, 0.7], V))


def random_f64_values(nx, V, seed):
    rng = np.random.default_rng(seed)
    return Values(nx, np.ones(V), f64_words(rng.standard_normal((V, nx * nx)) * 50.0), rng.choice([0.9, 0.8], V))


def near_values(nx):
    """(values, distinct): requests that differ in the least possible way -- one bit of the first word, one bit of the last word, the
    same P under two P_d, +0.0 against -0.0 -- and two requests of one NaN bit pattern, which are ONE value (the table compares bits)"""
    rng = np.random.default_rng(3)
    NP = nx * nx
    base = rng.standard_normal(NP).astype(np.float32)
    rows = [base.copy() for _ in range(8)]
    rows[1].view(np.uint32)[0] ^= 1                      # lowest bit of the first word
    rows[2].view(np.uint32)[NP - 1] ^= 0x80000000        # highest bit of the last word
    # rows[3]: base again, under another P_d
    rows[4][7] = 0.0
    rows[5][7] = -0.0
    rows[6][3] = np.float32(np.nan)
    rows[7][3] = np.float32(np.nan)                      # the same bit pattern: the same value as rows[6]
    assert rows[6].tobytes() == rows[7].tobytes()
    pd = np.full(8, 0.9)
    pd[3] = 0.8
    return Values(nx, np.zeros(8), f32_words(np.stack(rows)), pd), 7


COLLISION_SLOTS, COLLISION_VALUES = 64, 40


def _twins(tag, slot):
    """two candidates with one tag and one start slot, away from the crowd at the ends of the table: their indices"""
    key = (tag.astype(np.uint64) << np.uint64(6)) | slot.astype(np.uint64)
    order = np.argsort(key, kind="stable")
    same = [s for s in np.flatnonzero(key[order][1:] == key[order][:-1]) if 16 <= int(slot[order[s]]) < 48]
    assert same, "no two candidates with one tag and one start slot in the middle of the table"
    return int(order[same[0]]), int(order[same[0] + 1])


@functools.lru_cache(maxsize=None)
def collision_values(nx):
    """(values, pairs): 40 float32 values for a table of 64 slots, picked with the restated hash.  pairs[0]: two values that carry one
    31-bit tag and start at one slot and differ in their LAST word only (found among 4 M candidates: ~60 such pairs are expected);
    pairs[1]: the same for ONE covariance under two P_d (4 M candidate P_d) -- the table can tell neither pair apart by its tag.
    Twelve values start in the last three slots, so their chains run over the end of the table, three in the first three, the rest
    anywhere."""
    rng = np.random.default_rng(77 + nx)
    pw, N = nx * nx // 2, 1 << 22
    head = rng.standard_normal(nx * nx - 2).astype(np.float32).view(np.uint64)      # the first VT_PW - 1 words: the same for all
    last = rng.integers(0, 1 << 63, N, dtype=np.int64).astype(np.uint64) | (rng.integers(0, 2, N).astype(np.uint64) << np.uint64(63))
    last = np.unique(last)
    pd = np.float64(0.9)
    pre = np.uint64(0x9e3779b97f4a7c15) ^ np.array([pd]).view(np.uint64)
    for q in range(pw - 1):      # (the hash of the common head once, the last round for all candidates)
        pre ^= head[q:q + 1]
        pre *= np.uint64(0xff51afd7ed558ccd)
        pre ^= pre >> np.uint64(29)
    h = pre[0] ^ last
    h *= np.uint64(0xff51afd7ed558ccd)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xc4ceb9fe1a85ec53)
    h ^= h >> np.uint64(32)
    tag = (h >> np.uint64(32)) & np.uint64(VT_TAG64 - 1)
    slot = h & np.uint64(COLLISION_SLOTS - 1)
    pick = list(_twins(tag, slot))
    for s, n in ((63, 5), (62, 4), (61, 3), (0, 1), (1, 1), (2, 1)):
        pick += [int(i) for i in np.flatnonzero(slot == np.uint64(s))[:n]]
    rest = [int(i) for i in rng.choice(len(last), 200, replace=False) if int(i) not in pick]
    pick += rest[:COLLISION_VALUES - 2 - len(pick)]
    assert len(pick) == COLLISION_VALUES - 2 == len(set(pick))
    words = np.zeros((COLLISION_VALUES, 2 * pw), dtype=np.uint64)
    words[:, :pw - 1] = head
    words[:-2, pw - 1] = last[pick]
    words[-2:, pw - 1] = np.array([1.5, -2.5], dtype=np.float32).view(np.uint64)[0]
    pds = np.full(COLLISION_VALUES, pd)
    cand = 0.5 + np.arange(N) * 2.0 ** -30      # distinct detection probabilities in [0.5, 0.504)
    t2, l2 = vt_hash(words[-1:, :pw], cand.view(np.uint64), False)
    a, b = _twins(t2, l2 & np.uint32(COLLISION_SLOTS - 1))
    pds[-2:] = cand[[a, b]]
    vals = Values(nx, np.zeros(COLLISION_VALUES), words, pds)
    # (the shortcut above against the plain restatement)
    t3, l3 = vt_hash(words[:-2, :pw], pds[:-2].view(np.uint64), False)
    assert (t3 == tag[pick].astype(np.uint32)).all() and ((l3 & np.uint32(63)) == slot[pick].astype(np.uint32)).all()
    return vals, ((0, 1), (COLLISION_VALUES - 2, COLLISION_VALUES - 1))


def probe_slots(values, n_slots):
    """linear probing on the host, values inserted in list order: the slot each one ends in (which SET of slots is taken does not depend
    on the order)"""
    taken, out = set(), []
    for v in range(len(values)):
        p = values.hash(v)[1] & (n_slots - 1)
        while p in taken:
            p = (p + 1) & (n_slots - 1)
        taken.add(p)
        out.append(p)
    return out


def requests(V, times, seed):
    """every value of a list `times` times, shuffled"""
    return np.random.default_rng(seed).permutation(np.repeat(np.arange(V, dtype=np.int32), times)).astype(np.int32)
