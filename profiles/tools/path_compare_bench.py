#!/usr/bin/env python3
"""Path comparison against the fold-back arm profile: python3 profiles/tools/path_compare_bench.py [units=4096] [rounds=8] [n_pairs=4096] [dmax=64]

The bench batch of profiles/tools/fold_profile_bench.py (synth: 256 segments, 512 junctions, wide K = 19, every 8th unit with two
deletions and a duplication).  Per round, in ONE process and interleaved: ambi_batch_path_compare over `n_pairs` pairs -- pair i is
the path of unit i mod units before indelBFB against the path after it -- and ambi_batch_fold_profile (which = 1), each between two
HIP events on the caller's stream (the kernels, the pairs' upload and the waits in front of them; the device-to-host copy of the
block runs on the engine's copy stream and is outside the events), each waited for before the next is queued.  Seven of eight units
have no SV: their two paths are equal and the pair ends in the trim, so the request should cost about two reads of the paths.
Prints one JSON line with the rounds, the two medians, their ratio, and what the pairs were."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ambigram_amd import api, synth

n_units = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 8
n_pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
dmax = int(sys.argv[4]) if len(sys.argv) > 4 else 64
lib = api.load(); lib.ambi_set_device(0); torch.cuda.set_device(0)

tmp = tempfile.mkdtemp(); b = api.Batch(lib); keep = []
for i in range(n_units):
    edits = i % 8 == 7
    s = synth.make_sample(256, 512, "wide", 19, seed=2000 + i, n_del=2 if edits else 0, n_dup=1 if edits else 0)
    lh, sols = s.write(tmp, "j%d" % i)
    g = api.Graph(lib, lh); keep.append(g)
    b.add_chromosome_sol(g, 0, sols[0])
stream = torch.cuda.Stream(); st = stream.cuda_stream
b.upload(); b.run(0, st); b.wait(); b.download()
res = [b.unit_result(u) for u in range(n_units)]
assert all(r["status"] == 0 for r in res)
pairs = np.array([(api.compare_unit(i % n_units, 0), api.compare_unit(i % n_units, 1)) for i in range(n_pairs)], np.int32)

e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(queue, wait):
    with torch.cuda.stream(stream):
        e0.record(stream)
        queue()
        e1.record(stream)
    wait()
    e1.synchronize()
    return e0.elapsed_time(e1)


pc, fo = [], []
for r in range(rounds + 2):
    x = timed(lambda: b.path_compare(pairs, dmax, st), b.path_compare_wait)
    y = timed(lambda: b.fold_profile(1, st), b.fold_profile_wait)
    if r >= 2:   # (two warm-up rounds: the planes and the offsets travel with the first request)
        pc.append(x); fo.append(y)
got = b.path_compare_results()
d, d1 = got["dist"][:, 0], got["dist"][:, 1]
n_mid = got["len_a"][:, None] - got["prefix"] - got["suffix"]      # [pair, orientation]: the middle windows after the trim
m_mid = got["len_b"][:, None] - got["prefix"] - got["suffix"]
ran = (n_mid > 0) & (m_mid > 0) & (np.abs(n_mid - m_mid) <= dmax)
med = lambda v: float(np.median(v))
print(json.dumps(dict(device=torch.cuda.get_device_name(0), units=n_units, rounds=rounds, n_pairs=n_pairs, dmax=dmax,
                      cells_a=int(got["len_a"].sum()), cells_b=int(got["len_b"].sum()), equal=int((d == 0).sum()), capped=int((d < 0).sum()),
                      in_rounds=int((d > 0).sum()), max_dist=int(d.max()), dists=sorted(set(int(v) for v in d))[:40],
                      middle_max=int((got["len_a"] - got["prefix"][:, 0] - got["suffix"][:, 0]).max()),
                      # the reverse-complement orientation, and how many pairs go through rounds in it: a pair runs rounds when both
                      # middle windows are non-empty and their lengths differ by at most dmax; it runs all dmax + 1 when it ends at -1
                      equal_rc=int((d1 == 0).sum()), capped_rc=int((d1 < 0).sum()), in_rounds_rc=int((d1 > 0).sum()), max_dist_rc=int(d1.max()),
                      rounds_run=[int(v) for v in ran.sum(axis=0)], all_rounds_run=[int(v) for v in (ran & (got["dist"] < 0)).sum(axis=0)],
                      all_rounds_run_in_both=int((ran & (got["dist"] < 0)).all(axis=1).sum()),
                      path_compare_ms=[round(v, 4) for v in pc], fold_profile_ms=[round(v, 4) for v in fo],
                      path_compare_med_ms=med(pc), fold_profile_med_ms=med(fo), ratio_to_fold=med(pc) / med(fo))))
