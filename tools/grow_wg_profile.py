"""Development aid: the phases of a target workgroup of an OVERLAPPING grow launch (replay of the headline stream), from the stamps of
wavefront 0 and of a second wavefront -- wavefront 1, or with -DMHT_GROW_STAMPS_LAST the last one (union-find links, the tail).
Needs a stamped library, e.g.
  MHT_LIB_VARIANT=.stampsl MHT_EXTRA_HIPCC_FLAGS="-DMHT_GROW_STAMPS -DMHT_GROW_STAMPS_LAST" python -c "from pymht_amd.build import build_library; build_library(force=True)"
  MHT_LIB_VARIANT=.stampsl python tools/grow_wg_profile.py [rounds] [last]
`last`: the library was built with -DMHT_GROW_STAMPS_LAST (slot 0 of the second row is then the end of the tail).
With -DMHT_GROW_STAMPS_PREBAR on top, stamp 5 is taken in FRONT of the barrier behind the counts: `counts` is then each wavefront's own work
(wavefront 0: popcounts, prefix, child map; last wavefront: uf_claim) and its wait for the other sits in `links`."""
import ctypes as C, os, sys
os.environ["MHT_GROW_DEBUG"] = "1"; os.environ["MHT_OVL_FORCE"] = "1"; os.environ["MHT_OVL_STAMPS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from pymht_amd.utils.scenario import make_config
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
last_wave = len(sys.argv) > 2 and sys.argv[2] == "last"
sc = make_config('cfg3', seed=5446, n_scans=400, confine=True)
births, stats, final, trk0, _ = bench.prepass(sc, 0)
rp = bench.Replay(sc, births, 0)
NAMES = ['stage+record', 'phase1', 'cands', 'gate', 'counts', 'links', 'emit']
acc = {k: [] for k in ('w0', 'w1', 'w0_tail', 'w1_tail', 'tail', 'tail_tail', 'work', 'work_tail', 'span', 't5', 'n')}
for r in range(rounds):
    for _ in range(9 if r else 40):
        rp.step()
    rp._lib_mod.check(rp.lib.mht_synchronize(rp.h))
    a = np.zeros(2 * 8, dtype=np.uint64)
    rp._lib_mod.check(rp.lib.mht_forest_debug_read(rp.h, b"status2", a.ctypes.data_as(C.c_void_p), a.nbytes))
    w = a.reshape(2, 8)[:, 2:].astype(np.int64)
    k = rp.k
    new, old = w[k & 1], w[(k - 1) & 1]
    g = np.zeros(32 + 16 * 4000, dtype=np.uint64)
    rp._lib_mod.check(rp.lib.mht_forest_debug_read(rp.h, b"grow_dbg", g.ctypes.data_as(C.c_void_p), g.nbytes))
    ts = g[32:].reshape(4000, 16).astype(np.int64)
    t_ilp0, t_ilp1 = old[1], old[4]
    sel = (ts[:, 0] > t_ilp0) & (ts[:, 7] > ts[:, 0]) & (ts[:, 7] < t_ilp0 + 20000) & np.all(np.diff(ts[:, :8], axis=1) >= 0, axis=1)
    m = ts[sel]
    if len(m) < 100:
        continue
    end = m[:, 7]
    tail_sel = np.argsort(end)[-25:]      # the workgroups the launch ends with
    d0 = np.diff(m[:, :8], axis=1) / 100.0
    acc['w0'].append(np.median(d0, axis=0)); acc['w0_tail'].append(np.median(d0[tail_sel], axis=0))
    ok1 = np.all(m[:, 9:16] > 0, axis=1) & np.all(np.diff(m[:, 9:16], axis=1) >= 0, axis=1)
    if ok1.sum() > 50:
        d1 = np.diff(m[:, 9:16], axis=1) / 100.0      # stamps 1..7 of the second row
        acc['w1'].append(np.median(d1[ok1], axis=0))
        okt = ok1[tail_sel]
        if okt.sum() > 5:
            acc['w1_tail'].append(np.median(d1[tail_sel][okt], axis=0))
    if last_wave:
        tl = (m[:, 8] - np.maximum(m[:, 7], m[:, 15])) / 100.0
        okl = m[:, 8] > 0
        if okl.sum() > 50:
            acc['tail'].append(np.median(tl[okl])); acc['tail_tail'].append(np.median(tl[tail_sel][okl[tail_sel]]))
    work = (m[:, 7] - m[:, 1]) / 100.0
    acc['work'].append(np.median(work)); acc['work_tail'].append(np.median(work[tail_sel]))
    acc['span'].append((end.max() - t_ilp1) / 100.0); acc['t5'].append((new[5] - end.max()) / 100.0); acc['n'].append(len(m))
fmt = lambda v: '  '.join('%s %.2f' % (n, x) for n, x in zip(NAMES, v))
print('overlapping grow launches: %d rounds, %d target workgroups (median); us, medians over the rounds of per-launch medians' % (len(acc['n']), int(np.median(acc['n']))))
print('  wavefront 0, all workgroups      : ' + fmt(np.median(np.array(acc['w0']), axis=0)))
print('  wavefront 0, the 25 ending last  : ' + fmt(np.median(np.array(acc['w0_tail']), axis=0)))
if acc['w1'] and last_wave:      # (without `last` the second row is shared with thread 0's emission detail, tools/grow_profile.py: not phases)
    who = 'last wavefront'
    print('  %s, all (from stamp 1) : ' % who + fmt([float('nan')] + list(np.median(np.array(acc['w1']), axis=0))))
    if acc['w1_tail']:
        print('  %s, the 25 ending last : ' % who + fmt([float('nan')] + list(np.median(np.array(acc['w1_tail']), axis=0))))
if acc['tail']:
    print('  tail (later of stamp 7 of both wavefronts -> tchild / tcend written): all %.2f, the 25 ending last %.2f' % (np.median(acc['tail']), np.median(acc['tail_tail'])))
print('  work behind the record (stamp 1 -> 7, wavefront 0): all %.2f, the 25 ending last %.2f | last stamp 7 behind the overlapped ILP launch\'s end %.2f | t[5] behind the last stamp 7 %.2f' % (
    np.median(acc['work']), np.median(acc['work_tail']), np.median(acc['span']), np.median(acc['t5'])))
