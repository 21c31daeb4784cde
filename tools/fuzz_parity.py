"""Development aid: randomised parity runs -- the drop-in Tracker (device forest, device initiator) against the oracle on random
small scenarios (tests/fuzz_util.py), scan by scan.   python tools/fuzz_parity.py [n_cases] [first_seed] [similar] [ca] [streamed]
("similar": with similar-state pruning switched on and off at random; "ca": the linear six-state forest, Tracker(models.ca, ...), with
random acceleration tails -- fuzz_util.run_case_ca, which also takes "streamed": nothing looked at between the scans -- and prints the
campaign's census: ILPs, largest cluster, terminations, largest scan, sizes of the fused groups)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'oracle')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from fuzz_util import run_case, run_case_ca, add_census, group_histogram

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 20
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
similar, ca, streamed = ('similar' in sys.argv[3:]), ('ca' in sys.argv[3:]), ('streamed' in sys.argv[3:])
bad, census = 0, {}
for case in range(n_cases):
    try:
        if ca:
            ok, desc, msg, c = run_case_ca(seed0 + case, similar=similar, streamed=streamed)
            add_census(census, c)
        else:
            ok, desc, msg = run_case(seed0 + case, similar=similar)
    except Exception as e:
        ok, desc, msg = False, 'seed %d' % (seed0 + case), 'ERROR ' + repr(e)[:300]
    if not ok or not ca or case % 50 == 0:
        print(desc, 'ok' if ok else 'BAD', msg, flush=True)
    bad += 0 if ok else 1
    if ca and 'ERROR' in msg and 'error -3' not in msg:      # (anything but a capacity error: start nothing more on a device that may have faulted)
        print('stopped after case %d' % case)
        break
print('%d cases%s from seed %d, %d bad' % (n_cases, (' (ca%s%s)' % (' similar' if similar else '', ' streamed' if streamed else '')) if ca else '', seed0, bad))
if census:
    print('census: %d ILPs, largest cluster %d targets, %d terminations, largest scan %d leaves, fused groups by size %s'
          % (census["ilp"], census["cluster"], census["dead"], census["L"], group_histogram(census["groups"])))
