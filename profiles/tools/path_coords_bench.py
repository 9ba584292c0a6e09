#!/usr/bin/env python3
"""Path coordinates beside the fold profile: python3 profiles/tools/path_coords_bench.py [units=4096] [rounds=8] [queries=0,4096,1048576]

The bench batch of profiles/tools/path_align_bench.py (synth: 256 segments, 512 junctions, wide K = 19, every 8th unit with two
deletions and a duplication); the segments' lengths are end - start of the synthetic .lh.  Per number of queries and round, in ONE
process and interleaved: ambi_batch_path_coords -- the scan of every unit and that many lift-over queries, units and positions drawn
uniformly (seeded), positions over 0 .. the unit's amplicon length -- and ambi_batch_fold_profile for scale, each between two HIP
events on the caller's stream (the kernels, the uploads of queries and images and the waits in front of them; the device-to-host copy
of the block runs on the engine's copy stream and is outside the events), each waited for before the next is queued.  Prints one JSON
line per number of queries with the rounds, the two medians and their ratio, the plane's memory, and what the batch was: cells, the
longest path, base pairs.  A last line times the scan of the longest path alone (a batch of that one unit: one workgroup)."""
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
counts = [int(v) for v in (sys.argv[3] if len(sys.argv) > 3 else "0,4096,1048576").split(",")]
lib = api.load(); lib.ambi_set_device(0); torch.cuda.set_device(0)

tmp = tempfile.mkdtemp(); b = api.Batch(lib); keep = []; files = []
for i in range(n_units):
    edits = i % 8 == 7
    s = synth.make_sample(256, 512, "wide", 19, seed=2000 + i, n_del=2 if edits else 0, n_dup=1 if edits else 0)
    lh, sols = s.write(tmp, "j%d" % i)
    g = api.Graph(lib, lh); keep.append(g); files.append((lh, sols[0]))
    b.add_chromosome_sol(g, 0, sols[0])
stream = torch.cuda.Stream(); st = stream.cuda_stream
b.upload(); b.run(0, st); b.wait(); b.download()
assert all(b.unit_result(u)["status"] == 0 for u in range(n_units))

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
b.path_coords(1, None, st); b.path_coords_wait()
summ = b.path_coords_summaries()
assert (summ["status"] == 0).all() and (summ["bp_len"] > 0).all()
longest = int(np.argmax(summ["cells"]))
rng = np.random.default_rng(1)
for n in counts:
    units = rng.integers(0, n_units, n)
    q = api.lift_queries(units, (rng.random(n) * summ["bp_len"][units]).astype(np.int64)) if n else None
    pc, fold = [], []
    for r in range(rounds + 2):
        x = timed(lambda: b.path_coords(1, q, st), b.path_coords_wait)
        y = timed(lambda: b.fold_profile(1, st), b.fold_profile_wait)
        if r >= 2:   # (two warm-up rounds: the plane, the blocks and the images are leased with the first request of a size)
            pc.append(x); fold.append(y)
    if n:   # spot checks against the plane itself
        got = b.path_coords_results()
        assert (got["status"] == 0).all() and (got["cell"] >= 0).all()
        for i in rng.integers(0, n, 16):
            two = b.path_coords_copy(int(units[i]), int(got["cell"][i]), 2)
            assert two[0] == got["cell_start"][i] and two[0] <= q["pos"][i] < two[1]
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), units=n_units, rounds=rounds, queries=n, cells=int(summ["cells"].sum()),
                          longest_path=int(summ["cells"].max()), bp=int(summ["bp_len"].sum()), plane_bytes=b.path_coords_plane_device()[1],
                          fold_planes_bytes=b.fold_planes_device()[1], block_bytes=b.path_coords_device()[1],
                          path_coords_ms=[round(v, 4) for v in pc], fold_profile_ms=[round(v, 4) for v in fold],
                          path_coords_med_ms=med(pc), fold_profile_med_ms=med(fold), ratio_to_fold=med(pc) / med(fold))), flush=True)
b.close()
# the longest path alone: one unit, one workgroup
one = api.Batch(lib)
one.add_chromosome_sol(keep[longest], 0, files[longest][1])
one.upload(); one.run(0, st); one.wait()
t = []
for r in range(rounds + 2):
    x = timed(lambda: one.path_coords(1, None, st), one.path_coords_wait)
    if r >= 2:
        t.append(x)
s1 = one.path_coords_summaries()[0]
print(json.dumps(dict(device=torch.cuda.get_device_name(0), unit=longest, cells=int(s1["cells"]), bp=int(s1["bp_len"]),
                      scan_one_group_ms=[round(v, 4) for v in t], scan_one_group_med_ms=med(t))), flush=True)
one.close()
