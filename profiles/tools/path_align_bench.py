#!/usr/bin/env python3
"""Path alignment against the path comparison: python3 profiles/tools/path_align_bench.py [units=4096] [rounds=8] [n_pairs=4096] [dmaxs=0,64,1024]

The bench batch of profiles/tools/path_compare_bench.py (synth: 256 segments, 512 junctions, wide K = 19, every 8th unit with two
deletions and a duplication).  Per cap and round, in ONE process and interleaved: ambi_batch_path_align over `n_pairs` entries -- entry
i is the path of unit i mod units before indelBFB against the path after it, in the orientation as is -- and ambi_batch_path_compare
of the same pairs (both orientations: that is what the comparison computes), each between two HIP events on the caller's stream (the
kernel, the entries' upload and the waits in front of them; the device-to-host copy of the block runs on the engine's copy stream and
is outside the events), each waited for before the next is queued.  Prints one JSON line per cap with the rounds, the two medians,
their ratio, and what the entries were: distances, runs, the longest traceback."""
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
dmaxs = [int(v) for v in (sys.argv[4] if len(sys.argv) > 4 else "0,64,1024").split(",")]
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
assert all(b.unit_result(u)["status"] == 0 for u in range(n_units))
pairs = np.array([(api.compare_unit(i % n_units, 0), api.compare_unit(i % n_units, 1)) for i in range(n_pairs)], np.int32)
triples = np.concatenate([pairs, np.zeros((n_pairs, 1), np.int32)], axis=1)

e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(queue, wait):
    with torch.cuda.stream(stream):
        e0.record(stream)
        queue()
        e1.record(stream)
    wait()
    e1.synchronize()
    return e0.elapsed_time(e1)


med = lambda v: float(np.median(v))
for dmax in dmaxs:
    al, pc = [], []
    for r in range(rounds + 2):
        x = timed(lambda: b.path_align(triples, dmax, st), b.path_align_wait)
        y = timed(lambda: b.path_compare(pairs, dmax, st), b.path_compare_wait)
        if r >= 2:   # (two warm-up rounds: the history areas and the blocks are leased with the first request of a cap)
            al.append(x); pc.append(y)
    head, runs = b.path_align_results()
    cmp_ = b.path_compare_results()
    d = head["dist"]
    assert (d == cmp_["dist"][:, 0]).all() and (head["prefix"] == cmp_["prefix"][:, 0]).all() and (head["suffix"] == cmp_["suffix"][:, 0]).all()
    assert all(int(r["len"].sum()) == max(int(k), 0) for r, k in zip(runs, d))
    longest = max([int(r["len"].max()) for r in runs if len(r)] or [0])
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), units=n_units, rounds=rounds, n_pairs=n_pairs, dmax=dmax,
                          equal=int((d == 0).sum()), capped=int((d < 0).sum()), traced=int((d > 0).sum()), max_dist=int(d.max()),
                          runs_total=int(head["n_runs"].sum()), runs_max=int(head["n_runs"].max()), longest_run=longest,
                          block_bytes=b.path_align_device()[1],
                          path_align_ms=[round(v, 4) for v in al], path_compare_ms=[round(v, 4) for v in pc],
                          path_align_med_ms=med(al), path_compare_med_ms=med(pc), ratio_to_compare=med(al) / med(pc))), flush=True)
